#!/usr/bin/env python3
"""
Generate tests/golden/fm_<case>.npz by running the REFERENCE's decode_fm.getAudio, imported read-only and unmodified, on the seeded
recordings of tests/_fm.py, and tests/golden/sink_csv.txt with its sink.csv.  Only data is written: the reference's outputs, the
recording's sha256 and a few measured figures.  Runs where the reference is (DD_REFERENCE, or a checkout beside this repository);
the tests never need it.

Shims, all on this side (the reference is untouched):
  install_shim() of tools/gen_golden.py     the SciPy / NumPy names the reference's day had
  constants.PROC_CHUNKSIZE = _fm.CHUNK      set BEFORE directdemod.chunker is imported: its default argument is bound at import
  decode_fm.sigsrc = src                    the module global getAudio reads (decode_fm.py:57; it exists only under its __main__)

A file holds, per case: the audio (float64), its sample rate, the audio samples each chunk contributed, the sha256 of the recording,
and the figures of the assertion below.

The generator runs the same chain by hand with the reference's classes to look at y, the discriminator's input, and asserts on
|y[n] conj(y[n-1])|: beyond the first chunk every product is at least 0.1 of the median, and in the first chunk at most
ceil(150 / M) + 1 products -- the start-up of the 151-tap filter over its history of ones -- are below that.  (An angle of a small
product is ill-conditioned; tests/test_gpu_decode_fm.py holds the chunks after the first to a tighter bound on this ground.)
"""
import math
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("DD_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")      # a checkout beside this one
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import _fm  # noqa: E402
import gen_golden  # noqa: E402

SMALL = 0.1


def load_reference():
    gen_golden.install_shim()
    from directdemod import constants
    constants.PROC_CHUNKSIZE = _fm.CHUNK
    from directdemod import chunker, comm, decode_fm, demod_fm, filters, sink
    assert chunker.chunker.__init__.__defaults__ == (_fm.CHUNK,)
    return constants, chunker, comm, decode_fm, demod_fm, filters, sink


def run_case(ref, name):
    constants, chunker, comm, decode_fm, demod_fm, filters, sink = ref
    raw = _fm.case(name)
    fs, offset, bw, audioFreq = _fm.told(name)
    src = gen_golden.ArraySource(raw, fs)
    decode_fm.sigsrc = src
    audio = decode_fm.decode_fm(src, offset, bw, audioFreq).getAudio
    sig = np.asarray(audio.signal, dtype=np.float64)

    # the same chain by hand (decode_fm.py:54-70), looking at the discriminator's input
    bw_, af_ = (30000 if bw is None else bw), (15000 if audioFreq is None else audioFreq)
    M = int(fs / bw_)
    ck = chunker.chunker(src)
    flt, fm = filters.blackmanHarris(151), demod_fm.demod_fm()
    ys, lens, pieces = [], [], []

    def look(y):
        ys.append(np.array(y))
        return fm.demod(y)
    for a, b in ck.getChunks:
        s = comm.commSignal(fs, src.read(a, b), ck).offsetFreq(offset).filter(flt).bwLim(bw_, uniq="First").funcApply(look).bwLim(af_, True)
        lens.append(s.length)
        pieces.append(np.asarray(s.signal, dtype=np.float64))
    assert np.array_equal(np.concatenate(pieces), sig), "the chain by hand is not getAudio's"
    y = np.concatenate(ys)
    prod = np.abs(y[1:] * np.conj(y[:-1]))
    med = float(np.median(prod))
    first = len(ys[0]) - 1                               # products whose later sample lies in the first chunk
    small_first = int(np.sum(prod[:first] < SMALL * med))
    small_later = int(np.sum(prod[first:] < SMALL * med))
    allowed = math.ceil(150 / M) + 1
    print("fm_%s: %d samples, /%d, %d chunks -> %d audio samples at %d Hz; products below %.1f median: %d in chunk 0 (allowed %d), "
          "%d later; smallest ratio %.3g (chunk 0), %.3g (later)" %
          (name, raw.shape[0], M, len(lens), len(sig), audio.sampRate, SMALL, small_first, allowed, small_later,
           prod[:first].min() / med, prod[first:].min() / med))
    assert small_later == 0, "case %s: a small product beyond the first chunk: tune its amplitude or seed" % name
    assert small_first <= allowed, "case %s: %d small products in the first chunk" % (name, small_first)
    np.savez_compressed(os.path.join(OUT, "fm_%s.npz" % name), sha256=_fm.sha(raw), audio=sig, sampRate=int(audio.sampRate),
                        chunk_len=np.array(lens, dtype=np.int64), decim=M, small_first=small_first,
                        min_ratio_first=prod[:first].min() / med, min_ratio_later=prod[first:].min() / med)


def run_csv(ref):
    sink = ref[-1]
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.csv")
        sink.csv(p, CSV_DATA, titles=CSV_TITLES).write
        import gc
        gc.collect()                                     # (sink.py:103 leaves the file to the collector)
        txt = open(p).read()
    with open(os.path.join(OUT, "sink_csv.txt"), "w") as f:
        f.write(txt)
    print("sink_csv.txt: %d bytes" % len(txt))


# the two-column ragged input of tests/test_fm_host.py
CSV_TITLES = ["sample", "value"]
CSV_DATA = [[0, 1, 2, 3], [0.5, -1.25, "x"]]


def main():
    ref = load_reference()
    for name in (sys.argv[1:] or sorted(_fm.CASES)):
        t0 = time.time()
        run_case(ref, name)
        print("   %.1f s" % (time.time() - t0))
    run_csv(ref)


if __name__ == "__main__":
    main()
