#!/usr/bin/env python3
"""
Generate tests/golden/*.npz by running the REFERENCE ITSELF (imported read-only
from /root/reference) on small seeded inputs.

Runs only in the build container (the reference does not exist on the GPU box and
never travels).  Only data -- inputs' seeds and the reference's outputs -- is
written.  The inputs are regenerated in the tests from the seeds through
oracle/dd_oracle.py's synthetic generators (numpy's PCG64 stream is stable).

Compat shim (harness side, the reference is untouched):
  scipy.signal.{blackmanharris,hamming,gaussian} := scipy.signal.windows.*
  scipy.signal.remez(..., Hz=Fs)                 := scipy.signal.remez(..., fs=Fs)
  scipy.ifft                                     := scipy.fft.ifft
  numpy.int                                      := int
"""
import os
import re
import sys
import time

import numpy as np
import scipy
import scipy.fft
import scipy.signal
import scipy.signal.windows as _w
try:
    import scipy.misc  # noqa: F401  (decode_noaa.py:13 imports scipy.misc)
except Exception:
    pass

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")


def install_shim():
    scipy.signal.blackmanharris = _w.blackmanharris
    scipy.signal.hamming = _w.hamming
    scipy.signal.gaussian = _w.gaussian
    _remez = scipy.signal.remez

    def remez(numtaps, bands, desired, weight=None, Hz=None, **kw):
        if Hz is not None:
            kw["fs"] = Hz
        return _remez(numtaps, bands, desired, weight=weight, **kw)
    scipy.signal.remez = remez
    scipy.ifft = scipy.fft.ifft
    np.int = int


class ArraySource:
    """Duck-typed stand-in for source.IQwav: same .read() arithmetic is the
    reference's own (source.py:117-118) applied to an in-memory uint8[N,2]."""

    def __init__(self, raw, fs):
        self._d = raw
        self.sampFreq = fs
        self.length = raw.shape[0]
        self.sourceType = 0

    def read(self, a, b=None):
        if b is None:
            b = a + 1
        s = self._d[a:b, 0] + 1j * self._d[a:b, 1]
        return np.array(s).astype("complex64") - (127.5 + 1j * 127.5)


def gen_afsk(O, filters):
    # ------------------------------------------------------------------ AFSK1200 correlators (decode_afsk1200.py:58-158)
    # The correlators live inline in decode_afsk1200.getMsg.  Run the reference's getMsg on a small
    # synthetic AFSK recording and capture (a) the audio it hands to the correlator loop -- the output of
    # its butter band-pass -- and (b) the arguments/result of its single np.correlate call, i.e.
    # sign(binary_filter) and the bit-edge signal; then stop it (the frame decoder behind is host logic).
    from directdemod import decode_afsk1200 as dafsk
    fs_iq = 22050 * 40
    raw = O.synth_afsk_iq(64, fs_iq, 5)
    cap = {}

    class _Stop(Exception):
        pass
    _apply = filters.filter.applyOn

    def _butter_tap(self, x):          # butter inherits applyOn: shadow it on the subclass only
        y = _apply(self, x)
        cap["audio"] = np.array(y, dtype=np.float64)
        return y
    _corr = np.correlate

    def _correlate_tap(a, v, mode="valid"):
        r = _corr(a, v, mode=mode)
        cap["sign"], cap["kernel"], cap["changes"] = np.array(a), np.array(v), np.array(r)
        raise _Stop()
    filters.butter.applyOn = _butter_tap
    dafsk.np.correlate = _correlate_tap
    try:
        dafsk.decode_afsk1200(ArraySource(raw, fs_iq), 0, 22050).getMsg
    except _Stop:
        pass
    finally:
        del filters.butter.applyOn
        dafsk.np.correlate = _corr
    spb = 22050 // 1200
    g = {"fs_iq": np.int64(fs_iq), "n_bits": np.int64(64), "seed": np.int64(5), "bw": np.int64(22050),
         "audio": cap["audio"], "sign": cap["sign"].astype(np.int8), "kernel": cap["kernel"].astype(np.int8),
         "edge_sums": np.round(cap["changes"]).astype(np.int16)}     # np.correlate output; the reference divides it by spb (:156)
    assert np.array_equal(g["edge_sums"].astype(np.float64), cap["changes"])
    np.savez_compressed(os.path.join(OUT, "afsk.npz"), **g)
    print("afsk: audio", cap["audio"].shape, "sign +/0/-", int(np.sum(cap["sign"] > 0)), int(np.sum(cap["sign"] == 0)),
          int(np.sum(cap["sign"] < 0)))


def gen_c4_60s():
    """config 4 at BENCH duration ("duration 8 s (smoke) and 60 s (bench) ... Pass = identical index
    lists"): the reference's own getCrudeSync + getAccurateSync (decode_noaa.py:769-880) over a 60 s synthetic APT
    recording (seed 1); only the index lists (a few KB) are stored.  ~10 minutes of the reference's time (its accurate
    sync is ~2 s per window), so it has its own switch:  gen_golden.py --c4-60s"""
    install_shim()
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    from directdemod import decode_noaa
    from oracle import dd_oracle as O
    dur = 60.0
    raw = O.synth_apt_iq(dur, 2048000, seed=1)
    src = ArraySource(raw, 2048000)
    nobj = decode_noaa.decode_noaa(src, 30000.0)
    sa, sb = nobj.getCrudeSync()
    g = {"dur": np.float64(dur), "seed": np.int64(1), "useful": np.int64(nobj.useful),
         "crude_syncA": np.asarray(sa, dtype=np.int64), "crude_syncB": np.asarray(sb, dtype=np.int64)}
    acc = nobj.getAccurateSync()
    g["acc_syncA"] = np.asarray(acc[0], dtype=np.int64)
    g["acc_syncB"] = np.asarray(acc[4], dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "noaa_c4_60s.npz"), **g)
    print("noaa_c4_60s: crude A %d B %d, accurate A %d B %d, useful %d" % (len(sa), len(sb), len(acc[0]), len(acc[4]), nobj.useful))


def _apt_run(raw, fs):
    """the reference's getImage (and what it needs from its own run: the envelope it extracted the lines from) on one recording"""
    import time
    from directdemod import decode_noaa
    src = ArraySource(raw, fs)
    nobj = decode_noaa.decode_noaa(src, 30000.0)
    cap = []
    get_am = nobj._decode_noaa__getAM

    def _am_tap(sig):
        out = get_am(sig)
        cap.append(np.array(out.signal))
        return out
    nobj._decode_noaa__getAM = _am_tap
    nobj.getCrudeSync()
    t0 = time.perf_counter()
    img = nobj.getImage
    dt = time.perf_counter() - t0
    return nobj, np.asarray(img), cap[-1], dt


def _apt_line_inputs(nobj, env, rate):
    """per decoded line, from the reference's envelope: the two strip medians and the two sync FIFO medians (:348-377), with the
    package's host line table; the inputs of the host calibration state machine"""
    import scipy.signal as ss
    from directdemod_amd import decode_noaa as dn, constants as C
    n = len(env)
    sa, sb = nobj.getCrudeSync()
    unc = dn.to_rate(sa, rate, rate)
    fa, fb = dn.fill_sync(unc, n), dn.fill_sync(dn.to_rate(sb, rate, rate), n)
    a, b = dn.pair_syncs(fa, fb, rate)
    rows = dn.line_table(a, b, unc, rate, n)
    L1 = int((len(C.NOAA_SYNCA) * C.NOAA_T) * rate)
    low, high, s1, s2, ml, mh, use = [], [], [], [], [], [], []
    for (s_a, e_a, s_b, e_b, u) in rows:
        x = env[s_a:e_a]
        num = (len(x) // 1040) * 1040
        la = np.reshape(ss.resample(x, num), (1040, num // 1040))
        if u:
            for j in range(len(C.NOAA_SYNCA)):
                (low if C.NOAA_SYNCA[j] == 0 else high).extend(la[j])
                low, high = low[-C.NOAA_COLORCORRECT_FIFOLEN:], high[-C.NOAA_COLORCORRECT_FIFOLEN:]
        ml.append(np.median(low) if u else np.nan)
        mh.append(np.median(high) if u else np.nan)
        s1.append(np.median(env[s_a - L1:s_a]))
        s2.append(np.median(env[s_b - L1:s_b]))
        use.append(u)
    return {"line_strip_a": np.array(s1), "line_strip_b": np.array(s2), "line_sync_low": np.array(ml),
            "line_sync_high": np.array(mh), "line_use": np.array(use, dtype=bool)}


def gen_apt_image():
    """getImage / channelID / getColor of the reference on two synthetic recordings (decode_noaa.py:255-598):
      apt_image_plain.npz      synth_apt_iq(20 s, seed 1): no telemetry, backupImage; low / high, the __fillSync lists
      apt_image_telemetry.npz  tests/_apt_telemetry.py (44 s): the calibrated path; slope / intercept, channel IDs, getColor,
                               and the per-line inputs of the calibration state machine
    gen_golden.py --apt-image"""
    install_shim()
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import dd_oracle as O
    from _apt_telemetry import synth_apt_telemetry_iq
    fs = 2048000

    dur = 20.0
    nobj, img, env, dt = _apt_run(O.synth_apt_iq(dur, fs, seed=1), fs)
    sa, sb = nobj.getCrudeSync()
    rate = nobj._decode_noaa__syncCrudeSampRate
    ca = np.asarray(sa) / rate
    ca *= rate
    cb = np.asarray(sb) / rate
    cb *= rate
    g = {"dur": np.float64(dur), "seed": np.int64(1), "image": img.astype(np.uint8),
         "channel_id": np.array([-1 if v is None else v for v in nobj.channelID], dtype=np.int64),
         "low": np.float64(nobj._decode_noaa__low), "high": np.float64(nobj._decode_noaa__high),
         "crude_syncA": np.asarray(sa, dtype=np.int64), "crude_syncB": np.asarray(sb, dtype=np.int64), "rate": np.int64(rate),
         "n_env": np.int64(len(env)),
         "fill_syncA": np.asarray(nobj._decode_noaa__fillSync(ca, len(env)), dtype=np.float64),
         "fill_syncB": np.asarray(nobj._decode_noaa__fillSync(cb, len(env)), dtype=np.float64),
         "ref_getimage_s": np.float64(dt)}
    assert nobj._decode_noaa__slope is None
    np.savez_compressed(os.path.join(OUT, "apt_image_plain.npz"), **g)
    print("apt_image_plain: image", img.shape, "low %.6g high %.6g" % (g["low"], g["high"]), "getImage %.3f s" % dt)

    dur = 44.0
    nobj, img, env, dt = _apt_run(synth_apt_telemetry_iq(dur, fs), fs)
    rate = nobj._decode_noaa__syncCrudeSampRate
    assert nobj._decode_noaa__slope is not None, "the calibrated path was not taken"
    ch = nobj.channelID
    assert ch[0] is not None and ch[1] is not None, ch
    t0 = __import__("time").perf_counter()
    col = np.asarray(nobj.getColor)
    dtc = __import__("time").perf_counter() - t0
    g = {"dur": np.float64(dur), "seed": np.int64(3), "image": img.astype(np.uint8), "channel_id": np.array(ch, dtype=np.int64),
         "slope": np.float64(nobj._decode_noaa__slope), "intercept": np.float64(nobj._decode_noaa__intercept), "color": col,
         "rate": np.int64(rate), "ref_getimage_s": np.float64(dt), "ref_getcolor_s": np.float64(dtc)}
    m = len(env) // 2080
    meds = np.median(np.reshape(env[:m * 2080], (2080, m)), axis=-1)
    g["low0"], g["high0"] = [np.float64(v) for v in np.percentile(meds, (0.5, 99.5))]
    g.update(_apt_line_inputs(nobj, env, rate))
    np.savez_compressed(os.path.join(OUT, "apt_image_telemetry.npz"), **g)
    print("apt_image_telemetry: image", img.shape, "channelID", ch, "slope %.6g intercept %.6g" % (g["slope"], g["intercept"]),
          "getImage %.3f s getColor %.3f s" % (dt, dtc))


C1_NAME = "synth_20180101_120000Z_145825000Hz_IQ.wav"       # (the name pattern lets main.py:167-173 parse the centre frequency)
C1_FREQ = 145835000                                         # what a user would pass as -f: the signal sits 10 kHz above the centre


def gen_c1():
    """config 1 in its stated shape (VERDICT r5 "what's missing" 3): a synthetic 8-bit stereo IQ.wav at 2.4 MS/s whose NAME
    carries the centre frequency, read by the reference's own source.IQwav, through the reference's AFSK front end exactly as getMsg runs it
    (decode_afsk1200.py:67-94: chunker -> offsetFreq -> blackmanHarris(151) -> bwLim(22050) [M = 108] -> extend; demod_fm over the whole).
    Captured: what getMsg hands to its Butterworth band-pass, i.e. the FM output.  Stored: seed and shape, the first and last 2048 angles,
    every 4th angle in between (float64) -- ~110 KB.   gen_golden.py --c1"""
    install_shim()
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tempfile
    from directdemod import decode_afsk1200 as dafsk, filters, source
    from oracle import dd_oracle as O
    from _wav import write_iq_wav
    fs, nbits, seed = 2400000, 2400, 11                      # 2 s of AFSK1200
    # the offset main.py would hand to the decoder: -f minus the "...Hz" field of the file name (main.py:167-173)
    centre = int([i for i in C1_NAME.split("_") if i[-2:] == "Hz"][0][:-2])
    offset = C1_FREQ - centre
    raw = O.synth_afsk_iq(nbits, fs, seed, f_carrier=float(offset))
    cap = {}

    class _Stop(Exception):
        pass

    def _butter_tap(self, x):
        cap["fm"] = np.array(x, dtype=np.float64)
        raise _Stop()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, C1_NAME)
        write_iq_wav(path, raw, fs)
        src = source.IQwav(path)
        assert src.sampFreq == fs and src.length == raw.shape[0]
        filters.butter.applyOn = _butter_tap
        try:
            dafsk.decode_afsk1200(src, offset, 22050).getMsg
        except _Stop:
            pass
        finally:
            del filters.butter.applyOn
    fm = cap["fm"]
    M = int(fs / 22050)
    assert M == 108 and len(fm) == len(range(0, raw.shape[0], M)) - 1
    g = {"fs": np.int64(fs), "n_bits": np.int64(nbits), "seed": np.int64(seed), "offset": np.int64(offset), "bw": np.int64(22050),
         "n_out": np.int64(len(fm)), "rate_out": np.int64(int(fs / M)), "head": fm[:2048], "tail": fm[-2048:], "every4": fm[::4]}
    np.savez_compressed(os.path.join(OUT, "c1_afsk_front.npz"), **g)
    print("c1: %d samples @%d -> %d angles @%d S/s (M = %d), offset %d Hz, fixture %d bytes" %
          (raw.shape[0], fs, len(fm), int(fs / M), M, offset, os.path.getsize(os.path.join(OUT, "c1_afsk_front.npz"))))


def _afsk_frames_run(src, offset):
    """the reference's getMsg on `src` with taps: the np.correlate output, peakdetect's input and output, decode_nrzi's argument and
    result, bits_to_msg's arguments, the redirected stdout, the return value and useful"""
    import contextlib
    import io
    from directdemod import decode_afsk1200 as dafsk, peakdetect
    cap = {"msg_bits": []}
    _corr, _pd, _nrzi, _b2m = dafsk.np.correlate, peakdetect.peakdetect, dafsk.decode_afsk1200.decode_nrzi, dafsk.decode_afsk1200.bits_to_msg

    def corr_tap(a, v, mode="valid"):
        r = _corr(a, v, mode)
        cap["edge_sums"] = np.array(r)
        return r

    def pd_tap(y, *a, **k):
        r = _pd(y, *a, **k)
        cap["pd_in"], cap["pd_out"], cap["pd_kw"] = np.array(y), r, k
        return r

    def nrzi_tap(x):
        r = _nrzi(x)
        cap["nrzi_in"], cap["bitstream"] = np.array(x), np.array(r, dtype=np.int8)
        return r

    def b2m_tap(bits):
        cap["msg_bits"].append(np.array(bits, dtype=np.int8))
        return _b2m(bits)
    dafsk.np.correlate, dafsk.peakdetect.peakdetect = corr_tap, pd_tap
    dafsk.decode_afsk1200.decode_nrzi, dafsk.decode_afsk1200.bits_to_msg = nrzi_tap, b2m_tap
    out = io.StringIO()
    t0 = time.process_time()
    try:
        with contextlib.redirect_stdout(out):
            obj = dafsk.decode_afsk1200(src, offset, 22050)
            msg = obj.getMsg
    finally:
        dafsk.np.correlate, dafsk.peakdetect.peakdetect = _corr, _pd
        dafsk.decode_afsk1200.decode_nrzi, dafsk.decode_afsk1200.bits_to_msg = _nrzi, _b2m
    cap["cpu_s"] = time.process_time() - t0
    cap["stdout"], cap["msg"], cap["useful"] = out.getvalue(), msg, obj.useful
    return cap


def _save_afsk_frames(name, cap, extra):
    from directdemod import framechecksequence
    es = cap["edge_sums"]
    assert np.array_equal(np.abs(np.round(es) / (22050 // 1200)), cap["pd_in"])     # peakdetect's input is |edge sums| / spb
    bs = cap["bitstream"]
    flags = [k for k in range(len(bs) - 8) if "".join(map(str, bs[k:k + 8])) == "01111110"]      # (:217-224, from the captured bits)
    starts = [int(m) for m in re.findall(r"starts at (\d+)", cap["stdout"])]
    fidx = [int(m) for m in re.findall(r"# (\d+) starts", cap["stdout"])]
    mb = cap["msg_bits"]
    g = dict(extra)
    g.update({"edge_sums": np.round(es).astype(np.int16), "pd_lookahead": np.int64(cap["pd_kw"]["lookahead"]),
              "pd_max_x": np.array([p[0] for p in cap["pd_out"][0]], dtype=np.int32),
              "pd_max_y": np.array([p[1] for p in cap["pd_out"][0]], dtype=np.float64),
              "pd_min_x": np.array([p[0] for p in cap["pd_out"][1]], dtype=np.int32),
              "pd_min_y": np.array([p[1] for p in cap["pd_out"][1]], dtype=np.float64),
              "nrzi_sign": cap["nrzi_in"].astype(np.int8), "bitstream": bs, "bit_startflag": np.array(flags, dtype=np.int32),
              "frame_flag": np.array(fidx, dtype=np.int32), "frame_start": np.array(starts, dtype=np.int32),
              "frame_bits_len": np.array([len(b) for b in mb], dtype=np.int32),
              "frame_bits": np.concatenate(mb) if mb else np.zeros(0, np.int8),
              "stdout": np.array(cap["stdout"]), "msg": np.array("" if cap["msg"] is None else cap["msg"]),
              "useful": np.int64(cap["useful"]), "ref_cpu_s": np.float64(cap["cpu_s"])})
    if name == "afsk_frames_a.npz":         # fcs_crc16 of seeded random bit strings of assorted lengths
        rng = np.random.default_rng(77)
        lens = rng.integers(1, 600, 200)
        strs = [rng.integers(0, 2, k).astype(np.int8) for k in lens]
        g["crc_lens"] = lens.astype(np.int32)
        g["crc_bits"] = np.concatenate(strs)
        g["crc_values"] = np.array([framechecksequence.fcs_crc16("".join(map(str, s))) for s in strs])
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **g)
    print("%s: %d peaks, %d bits, %d flags, %d frames, msg %r, useful %d, reference %.2f s CPU, %d bytes" %
          (name, len(g["pd_max_x"]), len(bs), len(flags), len(mb), cap["msg"], cap["useful"], cap["cpu_s"], os.path.getsize(path)))


def gen_afsk_frames():
    """AFSK1200 frame logic (decode_afsk1200.py:160-269) on two recordings rebuilt from tests/_ax25.py: (a) 882 kS/s through an
    in-memory source, (b) config 1's shape, a 2.4 MS/s WAV read by the reference's source.IQwav.   gen_golden.py --afsk-frames"""
    install_shim()
    np.Inf = np.inf                         # peakdetect.py still uses it; NumPy 2 dropped it
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tempfile
    import matplotlib
    matplotlib.use("Agg")
    from directdemod import source
    import _ax25
    raw, fs, offset, _ = _ax25.fixture_a()
    _save_afsk_frames("afsk_frames_a.npz", _afsk_frames_run(ArraySource(raw, fs), offset), {"fs": np.int64(fs)})
    raw, fs, offset, _ = _ax25.fixture_b()
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, _ax25.C1_NAME)
        _ax25.write_wav(path, raw, fs)
        cap = _afsk_frames_run(source.IQwav(path), offset)
    _save_afsk_frames("afsk_frames_b.npz", cap, {"fs": np.int64(fs), "offset": np.int64(offset)})


def _walk_taps(walk, agc=None, costas=None):
    """--symbolwalk: `walk` = dict(x = the complex128 samples the tapped loop reads in place of the front end's, amean, pmean, lock =
    the values agc.mean, costas.mean and costas.plllock start from).  Nothing changes without it."""
    if walk is None:
        return
    if agc is not None:
        agc.mean = walk["amean"]
    if costas is not None:
        costas.mean = walk["pmean"]
        if walk["lock"]:
            costas.plllock = True
            costas.compAlphaBeta(costas.damping, costas.bw / 2.0)


def _meteor_patterns():
    """sync72khz, sync72khz1, sync72khz2 (decode_meteorm2.py:163-189)"""
    import _meteor
    s = _meteor.sync_bits()
    alt = np.arange(len(s)) % 2
    return s, np.where(alt == 0, s, 1 - s), np.where(alt == 1, s, 1 - s)


def _meteor_run(raw, offset, walk=None):
    """The reference's decode_meteorm2.getSyncs on an in-memory recording, tapped (walk: see _walk_taps): the sample index of every agc.adjust call (B or
    A: an A call is the one costas.loop follows), the AGC'd values, costas phase / freq after each loop, the sample of every lim call
    (the MAXSYNC buffers), each np.correlate's buffer length, template and argmax, and the MINSYNC / MAXSYNC log records; with
    each loop the corrected symbol it returns (gardnerA after pllObj.loop), which the LRPT fixture reads."""
    import logging
    import types
    from directdemod import comm
    from directdemod import decode_meteorm2 as dmet
    cur = {"base": 0, "j": -1}
    agc_rec, loop_rec, lim_rec, corr_rec, logs = [], [], [], [], []

    class TapSig(comm.commSignal):
        tapped = False

        def filter(self, f):
            r = comm.commSignal.filter(self, f)
            self.tapped = True
            return r

        @property
        def signal(self):
            arr = comm.commSignal.signal.fget(self)
            if not self.tapped:
                return arr
            return self._walk(arr if walk is None else walk["x"])

        def _walk(self, arr):
            base = cur["base"]
            for j, v in enumerate(arr):
                cur["j"] = base + j
                yield v
            cur["base"] = base + len(arr)

    class TapAgc(dmet.agc):
        def __init__(self):
            super().__init__()
            _walk_taps(walk, agc=self)

        def adjust(self, inp):
            out = super().adjust(inp)
            agc_rec.append((cur["j"], out))
            return out

    class TapCostas(dmet.costas):
        def __init__(self):
            super().__init__()
            _walk_taps(walk, costas=self)

        def loop(self, samp):
            out = super().loop(samp)
            loop_rec.append((len(agc_rec) - 1, self.phase, self.freq, out))
            return out

    _lim = dmet.lim

    def lim_tap(x):
        lim_rec.append(cur["j"])
        return _lim(x)
    _corr = dmet.np.correlate

    class NpTap(types.ModuleType):
        def __getattr__(self, k):
            return getattr(np, k)

    def corr_tap(a, v, mode="valid"):
        r = _corr(a, v, mode)
        t = [np.repeat(np.where(p == 1, 127, -128), 28) for p in _meteor_patterns()]
        corr_rec.append((len(a), int(np.argmax(np.abs(r))), 0 if np.array_equal(v, t[0]) else (1 if np.array_equal(v, t[2]) else 2)))
        return r
    nptap = NpTap("np")
    nptap.correlate = corr_tap

    class H(logging.Handler):
        def emit(self, rec):
            logs.append((rec.msg, rec.args))
    h = H()
    root = logging.getLogger()
    old_level = root.level
    root.addHandler(h)
    root.setLevel(logging.INFO)
    saved = (dmet.comm, dmet.agc, dmet.costas, dmet.lim, dmet.np)
    dmet.comm = types.SimpleNamespace(commSignal=TapSig)
    dmet.agc, dmet.costas, dmet.lim, dmet.np = TapAgc, TapCostas, lim_tap, nptap
    try:
        obj = dmet.decode_meteorm2(ArraySource(raw, 2048000), offset, None)
        t0 = time.process_time()
        err = None
        try:
            syncs = obj.getSyncs
        except ValueError as e:               # one MAXSYNC: np.min of an empty diff
            syncs, err = None, str(e)
        cpu = time.process_time() - t0
    finally:
        dmet.comm, dmet.agc, dmet.costas, dmet.lim, dmet.np = saved
        root.removeHandler(h)
        root.setLevel(old_level)
    return dict(syncs=syncs, useful=obj.useful, err=err, cpu=cpu, agc=agc_rec, loop=loop_rec, lim=lim_rec, corr=corr_rec, logs=logs)


def _small_int(v):
    """int8 where the values fit, else int16 (the per-symbol index steps: the fixtures stay under 300 KB)"""
    v = np.asarray(v, dtype=np.int64)
    assert np.abs(v).max(initial=0) < 32767
    return v.astype(np.int8 if np.abs(v).max(initial=0) < 127 else np.int16)


def _meteor_store(name, raw, offset, cap, trace_stride, trace_head):
    import _meteor
    agc, loop = cap["agc"], cap["loop"]
    a_call = np.array([r[0] for r in loop], dtype=np.int64)              # agc call index of each symbol's A
    is_a = np.zeros(len(agc), dtype=bool)
    is_a[a_call] = True
    j = np.array([r[0] for r in agc], dtype=np.int64)
    # B of symbol k: the last non-A call before its A call (-1 if none since the start)
    last_b = np.where(~is_a, np.arange(len(agc)), -1)
    last_b = np.maximum.accumulate(last_b) if len(agc) else last_b
    b_call = np.array([last_b[c - 1] if c > 0 else -1 for c in a_call], dtype=np.int64)
    b_idx = np.where(b_call >= 0, j[np.maximum(b_call, 0)], -1)
    a_idx = j[a_call] if len(a_call) else np.zeros(0, dtype=np.int64)
    nsym = len(a_call)
    sel = np.unique(np.concatenate((np.arange(min(nsym, trace_head)), np.arange(0, nsym, trace_stride)))).astype(np.int64)
    agc_a = np.array([agc[c][1] for c in a_call[sel]], dtype=np.complex128)
    phase = np.array([loop[k][1] for k in sel], dtype=np.float64)
    freq = np.array([loop[k][2] for k in sel], dtype=np.float64)
    mins = [int(a[0]) for m, a in cap["logs"] if m.startswith("MINSYNC")]
    maxs = [float(a[0]) for m, a in cap["logs"] if m.startswith("MAXSYNC")]
    # each correlation's buffer: lim's record (two calls per appended sample) from the buffer's first sample (maxBuffStart, the
    # MAXSYNC value minus argmax / 2) on, len / 2 samples; cut into contiguous stretches
    lim = np.array(cap["lim"], dtype=np.int64)[::2]
    ivs, starts, args, tmpl = [], [], [], []
    pos = 0
    for (L, am, tm), ms in zip(cap["corr"], maxs):
        start = int(ms - am / 2.0)
        k = pos + int(np.argmax(lim[pos:] == start))
        smp = lim[k:k + L // 2]
        cuts = [0] + [int(c) + 1 for c in np.nonzero(np.diff(smp) != 1)[0]] + [len(smp)]
        ivs.append([(int(smp[cuts[i]]), cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1)])
        starts.append(start)
        args.append(am)
        tmpl.append(tm)
        pos = k + L // 2
    iv_flat = np.array([[i, a, b] for i, iv in enumerate(ivs) for a, b in iv], dtype=np.int64).reshape(-1, 3)
    g = dict(sha256=np.array(_meteor.sha256(raw)), offset=np.int64(offset), n=np.int64(raw.shape[0]),
             syncs=np.array(cap["syncs"] if cap["syncs"] is not None else [], dtype=np.float64),
             one_maxsync=np.int64(cap["syncs"] is None), useful=np.int64(cap["useful"]),
             minsync=np.array(mins, dtype=np.int64), maxsync=np.array(maxs, dtype=np.float64),
             buf_intervals=iv_flat, buf_start=np.array(starts, dtype=np.int64), argmax=np.array(args, dtype=np.int64),
             template=np.array(tmpl, dtype=np.int64), nsym=np.int64(nsym),
             a_first=np.int64(a_idx[0] if nsym else -1), a_diff=_small_int(np.diff(a_idx)), ab_gap=_small_int(a_idx - b_idx),
             trace_sel=sel, trace_agc=agc_a, trace_phase=phase, trace_freq=freq, trace_stride=np.int64(trace_stride),
             ref_cpu_s=np.float64(cap["cpu"]))
    path = os.path.join(OUT, "meteor_%s.npz" % name)
    np.savez_compressed(path, **g)
    print("meteor %s: n %d, %d symbols, MINSYNC %s, templates %s, syncs %s, useful %d, cpu %.1f s, %d bytes" %
          (name, raw.shape[0], nsym, mins, tmpl, g["syncs"].tolist(), cap["useful"], cap["cpu"], os.path.getsize(path)))


def gen_meteor():
    """Meteor-M2 sync detection (decode_meteorm2.py:229-324) on the recordings of tests/_meteor.py.   gen_golden.py --meteor [names]"""
    install_shim()
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _meteor
    names = [a for a in sys.argv[2:] if a in _meteor.CASES] or sorted(_meteor.CASES)
    for name in names:
        raw, off = _meteor.case(name)
        big = raw.shape[0] > 20000000
        _meteor_store(name, raw, off, _meteor_run(raw, off), 2048 if big else 64, 1024 if big else 4096)


def gen_lrpt():
    """The int8 soft pairs of the reference's own symbol walk (agc / Gardner / costas, tapped by _meteor_run) over the LRPT recording
    of tests/_lrpt.py, halved and limited as decode_meteorm2.py:238-239 does: what the frame decoder's restatement starts from.
    gen_golden.py --lrpt [names]"""
    install_shim()
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _lrpt
    from directdemod import decode_meteorm2 as dmet
    names = [a for a in sys.argv[2:] if a in _lrpt.CASES] or sorted(_lrpt.CASES)
    for name in names:
        raw, _, start = _lrpt.case(name)
        cap = _meteor_run(raw, 0)
        sym = np.array([r[3] for r in cap["loop"]], dtype=np.complex128)
        soft = np.array([dmet.lim(v / 2) for s in sym for v in (s.real, s.imag)], dtype=np.int8)
        path = os.path.join(OUT, "lrpt_%s.npz" % name)
        np.savez_compressed(path, sha256=np.array(_lrpt.sha256(raw)), n=np.int64(raw.shape[0]), nsym=np.int64(len(sym)), soft=soft,
                            ref_cpu_s=np.float64(cap["cpu"]))
        print("lrpt %s: n %d, start bit %d, %d symbols, syncs %s, cpu %.1f s, %d bytes" %
              (name, raw.shape[0], start, len(sym), cap["syncs"], cap["cpu"], os.path.getsize(path)))


def gen_lrpt_rs():
    """gen_lrpt for the recording of tests/_rs.py that carries RS-encoded frames and two fades (case b): tests/golden/lrpt_rs_b.npz.
    gen_golden.py --lrpt-rs"""
    install_shim()
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _rs
    from directdemod import decode_meteorm2 as dmet
    for name in sorted(_rs.CASES):
        raw, _, start = _rs.case(name)
        cap = _meteor_run(raw, 0)
        sym = np.array([r[3] for r in cap["loop"]], dtype=np.complex128)
        soft = np.array([dmet.lim(v / 2) for s in sym for v in (s.real, s.imag)], dtype=np.int8)
        path = os.path.join(OUT, "lrpt_rs_%s.npz" % name)
        np.savez_compressed(path, sha256=np.array(_rs.sha256(raw)), n=np.int64(raw.shape[0]), nsym=np.int64(len(sym)), soft=soft,
                            ref_cpu_s=np.float64(cap["cpu"]))
        print("lrpt_rs %s: n %d, start bit %d, %d symbols, syncs %s, cpu %.1f s, %d bytes" %
              (name, raw.shape[0], start, len(sym), cap["syncs"], cap["cpu"], os.path.getsize(path)))


def _funcube_run(raw, offset, corrfreq, center, channel, walk=None):
    """The reference's decode_funcube.getSyncs on an in-memory recording, tapped like _meteor_run (walk: see _walk_taps): the sample index of every
    agc.adjust call (B or A: an A call is the one costas.loop follows), the AGC'd values, costas phase / freq after each loop, the
    samples of each np.correlate's buffer and its argmax, each chunk's mixer frequencies, and the log records."""
    import logging
    import types
    import scipy.fft as _sfft
    if not callable(scipy.fft):
        scipy.fft = _sfft.fft                # `from scipy import fft` (sandbox/frequency_shift.py:2) meant the function
    from directdemod import comm
    from directdemod import decode_funcube as dfc
    cur = {"base": 0, "j": -1}
    agc_rec, loop_rec, lim_rec, corr_rec, mix_rec, logs = [], [], [], [], [], []

    class TapSig(comm.commSignal):
        tapped = False

        def offsetFreq(self, f):
            if np.ndim(f) != 0:
                mix_rec.append((float(f[0]), float(f[1] - f[0]), float(f[-1]), len(f)))
            return comm.commSignal.offsetFreq(self, f)

        def filter(self, f):
            r = comm.commSignal.filter(self, f)
            self.tapped = True
            return r

        @property
        def signal(self):
            arr = comm.commSignal.signal.fget(self)
            if not self.tapped:
                return arr
            return self._walk(arr if walk is None else walk["x"])

        def _walk(self, arr):
            base = cur["base"]
            for j, v in enumerate(arr):
                cur["j"] = base + j
                yield v
            cur["base"] = base + len(arr)

    class TapAgc(dfc.agc):
        def __init__(self):
            super().__init__()
            _walk_taps(walk, agc=self)

        def adjust(self, inp):
            out = super().adjust(inp)
            agc_rec.append((cur["j"], out))
            return out

    class TapCostas(dfc.costas):
        def __init__(self):
            super().__init__()
            _walk_taps(walk, costas=self)

        def loop(self, samp):
            out = super().loop(samp)
            loop_rec.append((len(agc_rec) - 1, self.phase, self.freq, out))
            return out

    _lim = dfc.lim

    def lim_tap(x):
        lim_rec.append(cur["j"])
        return _lim(x)
    _corr = dfc.np.correlate

    class NpTap(types.ModuleType):
        def __getattr__(self, k):
            return getattr(np, k)

    def corr_tap(a, v, mode="valid"):
        r = _corr(a, v, mode)
        smp = np.array(lim_rec[-len(a):], dtype=np.int64)       # the buffer holds the last len(a) lim values (pops leave from the front)
        cuts = [0] + [int(c) + 1 for c in np.nonzero(np.diff(smp) != 1)[0]] + [len(smp)]
        corr_rec.append((len(a), int(np.argmax(np.abs(r))), [(int(smp[cuts[i]]), cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1)]))
        del lim_rec[:]
        return r
    nptap = NpTap("np")
    nptap.correlate = corr_tap

    class H(logging.Handler):
        def emit(self, rec):
            logs.append((rec.msg, rec.args))
    h = H()
    root = logging.getLogger()
    old_level = root.level
    root.addHandler(h)
    root.setLevel(logging.INFO)
    saved = (dfc.comm, dfc.agc, dfc.costas, dfc.lim, dfc.np)
    dfc.comm = types.SimpleNamespace(commSignal=TapSig)
    dfc.agc, dfc.costas, dfc.lim, dfc.np = TapAgc, TapCostas, lim_tap, nptap
    try:
        src = ArraySource(raw, 2048000)
        src.memmap = np.ascontiguousarray(raw).reshape(-1).astype(np.int16)     # `-127 + uint8` was promoted by the NumPy of its day
        obj = dfc.decode_funcube(src, offset, None, center, channel, corrfreq)
        t0 = time.process_time()
        err = None
        try:
            with np.errstate(divide="ignore"):
                syncs = obj.getSyncs
        except ValueError as e:               # one MAXSYNC: np.min of an empty diff
            syncs, err = None, str(e)
        cpu = time.process_time() - t0
    finally:
        dfc.comm, dfc.agc, dfc.costas, dfc.lim, dfc.np = saved
        root.removeHandler(h)
        root.setLevel(old_level)
    return dict(syncs=syncs, useful=obj.useful, err=err, cpu=cpu, agc=agc_rec, loop=loop_rec, corr=corr_rec, mix=mix_rec, logs=logs)


def _funcube_store(name, raw, offset, corrfreq, cap, trace_stride, trace_head):
    import _funcube
    agc, loop = cap["agc"], cap["loop"]
    a_call = np.array([r[0] for r in loop], dtype=np.int64)              # agc call index of each symbol's A
    is_a = np.zeros(len(agc), dtype=bool)
    is_a[a_call] = True
    j = np.array([r[0] for r in agc], dtype=np.int64)
    last_b = np.where(~is_a, np.arange(len(agc)), -1)
    last_b = np.maximum.accumulate(last_b) if len(agc) else last_b
    b_call = np.array([last_b[c - 1] if c > 0 else -1 for c in a_call], dtype=np.int64)
    b_idx = np.where(b_call >= 0, j[np.maximum(b_call, 0)], -1)
    a_idx = j[a_call] if len(a_call) else np.zeros(0, dtype=np.int64)
    nsym = len(a_call)
    sel = np.unique(np.concatenate((np.arange(min(nsym, trace_head)), np.arange(0, nsym, trace_stride)))).astype(np.int64)
    agc_a = np.array([agc[c][1] for c in a_call[sel]], dtype=np.complex128)
    phase = np.array([loop[k][1] for k in sel], dtype=np.float64)
    freq = np.array([loop[k][2] for k in sel], dtype=np.float64)
    mins = [int(a[0]) for m, a in cap["logs"] if m.startswith("MINSYNC")]
    maxs = [int(a[0]) for m, a in cap["logs"] if m.startswith("MAXSYNC")]
    shifts = [float(a[0]) for m, a in cap["logs"] if m.startswith("doppler shift")]
    assert len(maxs) == len(cap["corr"]) and len(shifts) == len(cap["mix"])
    ivs = [c[2] for c in cap["corr"]]
    args = [c[1] for c in cap["corr"]]
    starts = [ms - am for ms, am in zip(maxs, args)]
    assert all(sum(c for _, c in iv) == L for iv, (L, _, _) in zip(ivs, cap["corr"]))
    iv_flat = np.array([[i, a, b] for i, iv in enumerate(ivs) for a, b in iv], dtype=np.int64).reshape(-1, 3)
    one = cap["syncs"] is None
    g = dict(sha256=np.array(_funcube.sha256(raw)), offset=np.int64(offset), corrfreq=np.int64(corrfreq), n=np.int64(raw.shape[0]),
             syncs=np.array([] if one else cap["syncs"], dtype=np.int64), one_maxsync=np.int64(one), useful=np.int64(cap["useful"]),
             minsync=np.array(mins, dtype=np.int64), maxsync=np.array(maxs, dtype=np.int64),
             buf_intervals=iv_flat, buf_start=np.array(starts, dtype=np.int64), argmax=np.array(args, dtype=np.int64),
             nsym=np.int64(nsym), a_first=np.int64(a_idx[0] if nsym else -1), a_diff=_small_int(np.diff(a_idx)),
             ab_gap=_small_int(a_idx - b_idx),
             trace_sel=sel, trace_agc=agc_a, trace_phase=phase, trace_freq=freq, trace_stride=np.int64(trace_stride),
             chunk_offset=np.array(shifts, dtype=np.float64),
             dopp_start=np.array([m[0] for m in cap["mix"]], dtype=np.float64),
             dopp_delta=np.array([m[1] for m in cap["mix"]], dtype=np.float64),
             dopp_current=np.array([m[2] for m in cap["mix"]], dtype=np.float64),
             dopp_target=np.array([offset + s for s in shifts], dtype=np.float64),
             ref_cpu_s=np.float64(cap["cpu"]))
    if not one and cap["syncs"] is not None:
        assert all(isinstance(s, np.integer) for s in cap["syncs"])
    path = os.path.join(OUT, "funcube_%s.npz" % name)
    np.savez_compressed(path, **g)
    print("funcube %s: n %d, %d symbols, MINSYNC %s, MAXSYNC %s (buffers %s), syncs %s%s, useful %d, chunk offsets %s, cpu %.1f s, "
          "%d bytes" % (name, raw.shape[0], nsym, mins, maxs, [c[0] for c in cap["corr"]], g["syncs"].tolist(),
                        " (the reference raised: %s)" % cap["err"] if one else "", cap["useful"], shifts, cap["cpu"],
                        os.path.getsize(path)))


def gen_funcube():
    """Funcube sync detection (decode_funcube.py:148-306) on the recordings of tests/_funcube.py.   gen_golden.py --funcube [names]"""
    install_shim()
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import matplotlib
    matplotlib.use("Agg")
    import _funcube
    names = [a for a in sys.argv[2:] if a in _funcube.CASES] or sorted(_funcube.CASES)
    for name in names:
        raw, off, corr = _funcube.case(name)
        big = raw.shape[0] > 20000000
        _funcube_store(name, raw, off, corr, _funcube_run(raw, off, corr, _funcube.CENTER, _funcube.CHANNEL),
                       256 if big else 16, 1024 if big else 2048)


def gen_symbolwalk():
    """The reference's own agc / Gardner / costas loop (both decoders') over the seeded samples of tests/_symbolwalk.py, read in place
    of the front end's output, from the start values each case states: every symbol's B and A sample index, agc.adjust's output,
    the corrected symbol, and phase and freq after the loop.   gen_golden.py --symbolwalk [names]"""
    install_shim()
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import matplotlib
    matplotlib.use("Agg")
    import _funcube
    import _symbolwalk as sw
    fixtures = [k for k, c in sw.CASES.items() if c.get("fixture")]
    for name in [a for a in sys.argv[2:] if a in fixtures] or fixtures:
        policy, x, st = sw.case(name)
        assert all(st[f] == 0 for f in ("timing", "b_re", "b_im", "c_re", "c_im", "dc_re", "dc_im", "phase", "ctr")) and st["freq"] == 0.001
        walk = dict(x=x, amean=st["amean"], pmean=st["pmean"], lock=st["lock"])
        raw = np.full((len(x), 2), 128, dtype=np.uint8)               # what the front end reads; the loop never sees it
        if policy == "meteor":
            cap = _meteor_run(raw, 0, walk)
        else:
            cap = _funcube_run(raw, 0, False, _funcube.CENTER, _funcube.CHANNEL, walk)
        agc, loop = cap["agc"], cap["loop"]
        a_call = np.array([r[0] for r in loop], dtype=np.int64)
        is_a = np.zeros(len(agc), dtype=bool)
        is_a[a_call] = True
        j = np.array([r[0] for r in agc], dtype=np.int64)
        last_b = np.maximum.accumulate(np.where(~is_a, np.arange(len(agc)), -1))
        b_call = np.array([last_b[c - 1] if c > 0 else -1 for c in a_call], dtype=np.int64)
        g = dict(sha256=np.array(sw.sha256(x)), n=np.int64(len(x)), amean=np.float64(st["amean"]), pmean=np.float64(st["pmean"]),
                 lock=np.int64(st["lock"]), aidx=j[a_call].astype(np.int32),
                 bidx=np.where(b_call >= 0, j[np.maximum(b_call, 0)], -1).astype(np.int32),      # -1: no B sample yet
                 agc=np.array([agc[c][1] for c in a_call], dtype=np.complex128),
                 sym=np.array([r[3] for r in loop], dtype=np.complex128),
                 phase=np.array([r[1] for r in loop], dtype=np.float64), freq=np.array([r[2] for r in loop], dtype=np.float64))
        path = os.path.join(OUT, "symbolwalk_%s.npz" % name)
        np.savez_compressed(path, **g)
        print("symbolwalk %s: n %d, %d symbols, %d B calls, %d bytes" % (name, len(x), len(a_call), int((~is_a).sum()), os.path.getsize(path)))


def main():
    if "--symbolwalk" in sys.argv:
        return gen_symbolwalk()
    if "--funcube" in sys.argv:
        return gen_funcube()
    if "--meteor" in sys.argv:
        return gen_meteor()
    if "--lrpt-rs" in sys.argv:
        return gen_lrpt_rs()
    if "--lrpt" in sys.argv:
        return gen_lrpt()
    if "--afsk-frames" in sys.argv:
        return gen_afsk_frames()
    if "--c4-60s" in sys.argv:
        return gen_c4_60s()
    if "--c1" in sys.argv:
        return gen_c1()
    if "--apt-image" in sys.argv:
        return gen_apt_image()
    only_afsk = "--afsk-only" in sys.argv
    install_shim()
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    import matplotlib
    matplotlib.use("Agg")
    from directdemod import comm, filters, demod_fm, demod_am, chunker, constants, decode_noaa
    from oracle import dd_oracle as O

    os.makedirs(OUT, exist_ok=True)
    if only_afsk:
        gen_afsk(O, filters)
        return

    # ------------------------------------------------------------------ per-op vectors
    for seed, L in ((0, 2048), (1, 1024), (2, 1024)):
        g = {}
        raw = O.synth_iq_noise(L, 100 + seed)
        x = O.grid_c64(raw)
        g["seed"] = np.int64(100 + seed)
        g["L"] = np.int64(L)

        # N1 offsetFreq: start index 0 (no chunker) and 19 999 000 (chunker var preset)
        s = comm.commSignal(2400000, x).offsetFreq(25000.0)
        g["nco_start0"] = s.signal.copy()

        class _Src:
            length = L
        ck = chunker.chunker(_Src())
        ck.set(constants.CHUNK_FREQOFFSET, 19999000)
        s = comm.commSignal(2400000, x, ck).offsetFreq(25000.0)
        g["nco_start19999000"] = s.signal.copy()
        assert ck.get(constants.CHUNK_FREQOFFSET) == 19999000 + L

        # F1 stateful FIR over 3 uneven chunks (one shorter than ntaps-1)
        cuts = [0, L // 2 - 37, L // 2 + 60, L]
        for name, flt in (("hamming255", filters.hamming(255)),
                          ("bh151", filters.blackmanHarris(151)),
                          ("remez127", filters.remez(10000000, [[0, 100e3], [150e3, 4999999]], [1, 0], ntaps=127)),
                          ("gauss51", filters.gaussian(51, 5)),
                          ("rollavg3", filters.rollingAverage(3))):
            outs = [flt.applyOn(x[cuts[i]:cuts[i + 1]]) for i in range(3)]
            g["fir_" + name] = np.concatenate(outs)
            g["taps_" + name] = np.asarray(flt.getB, dtype=np.float64)
        g["fir_cuts"] = np.array(cuts, dtype=np.int64)

        # F3 plain (stateless) and initOut paths
        g["fir_plain_hamming255"] = filters.hamming(255, storeState=False).applyOn(x)
        fi = filters.rollingAverage(4, initOut=[1.0, 2.0, 3.0])
        g["fir_initout_rollavg4"] = np.concatenate([fi.applyOn(x[:100].real), fi.applyOn(x[100:300].real)])

        # F2 zero-phase
        g["filtfilt_bh151"] = filters.blackmanHarris(151, zeroPhase=True).applyOn(x)
        if L > 1476:   # filtfilt needs len(x) > 3*ntaps
            g["filtfilt_hamming492_real"] = filters.hamming(492, zeroPhase=True).applyOn(x.real.astype(np.float64))
        g["filtfilt_hamming101_real"] = filters.hamming(101, zeroPhase=True).applyOn(x.real.astype(np.float64))

        # F4 butter (IIR): state carried over chunks (real + complex), plain, zero-phase
        bt = filters.butter(60235, 4160.0)
        g["iir_b"], g["iir_a"] = np.asarray(bt.getB), np.asarray(bt.getA)
        xr = x.real.astype(np.float64)
        g["iir_lp_real_chunks"] = np.concatenate([bt.applyOn(xr[cuts[i]:cuts[i + 1]]) for i in range(3)])
        btc = filters.butter(2048000, 20000.0)
        g["iir_lp_cplx_chunks"] = np.concatenate([btc.applyOn(x[cuts[i]:cuts[i + 1]]) for i in range(3)])
        g["iir_bp_plain"] = filters.butter(60235, 1000.0, 3000.0, n=4, typeFlt=constants.FLT_BP, storeState=False).applyOn(xr)
        g["iir_lp_filtfilt"] = filters.butter(60235, 4160.0, zeroPhase=True).applyOn(xr)

        # R1 decimation with carry over uneven chunks, M=34 and 50
        for fs, t, tag in ((2048000, 60000, "m34"), (10000000, 200000, "m50")):
            ck = chunker.chunker(_Src())
            outs = []
            rate = None
            for i in range(3):
                s = comm.commSignal(fs, x[cuts[i]:cuts[i + 1]], ck).bwLim(t, uniq="First")
                outs.append(np.array(s.signal))
                rate = s.sampRate
            g["decim_" + tag] = np.concatenate(outs)
            g["decim_" + tag + "_rate"] = np.int64(rate)

        # D1 FM demod with carry, on FIR output
        y = g["fir_hamming255"]
        fm = demod_fm.demod_fm()
        g["fm_carry"] = np.concatenate([fm.demod(y[cuts[i]:cuts[i + 1]]) for i in range(3)])
        g["fm_nostate"] = demod_fm.demod_fm(storeState=False).demod(y)

        # R2 strict bwLim (FFT resample) of the FM output, one chunk
        ang = g["fm_nostate"]
        s = comm.commSignal(60235, ang).bwLim(40960, True)
        g["resample_60235_40960"] = np.array(s.signal)
        s = comm.commSignal(200000, ang).bwLim(11025, True)
        g["resample_200000_11025"] = np.array(s.signal)

        # A1 AM envelope on a power-of-2 block and on a non-power-of-2 block
        am = demod_am.demod_am()
        g["am_env_full"] = am.demod(ang[:L - 1 if (L - 1) % 2 == 0 else L - 2])
        g["am_env_3000"] = am.demod(np.resize(ang, 3000)) if L >= 3000 else am.demod(ang[:750])

        # fused chain through the public API, chunked (tutorial/3_chunking.py:24-38 +
        # offsetFreq, decode_noaa.py:623), chunks of 600
        class _Src2:
            length = L
        ck = chunker.chunker(_Src2(), 600)
        out = comm.commSignal(2048000)
        bh = filters.blackmanHarris(151)
        fm = demod_fm.demod_fm()
        for a, b in ck.getChunks:
            s = comm.commSignal(2048000, x[a:b], ck).offsetFreq(30000.0).filter(bh) \
                .bwLim(60000, uniq="First").funcApply(fm.demod)
            out.extend(s)
        g["chain_bh151_m34"] = np.array(out.signal)
        g["chain_bh151_m34_rate"] = np.int64(out.sampRate)
        g["chain_chunks"] = np.array(ck.getChunks, dtype=np.int64)

        # un-decimated headline chain (C2 shape): NCO 25 kHz + hamming255 + FM, one chunk
        s = comm.commSignal(2400000, x).offsetFreq(25000.0).filter(filters.hamming(255)) \
            .funcApply(demod_fm.demod_fm().demod)
        g["chain_c2"] = np.array(s.signal)

        np.savez_compressed(os.path.join(OUT, "ops_seed%d.npz" % seed), **g)
        print("ops_seed%d: %d arrays" % (seed, len(g)))

    # ------------------------------------------------------------------ C3-shaped chain
    g = {}
    L = 40000
    raw = O.synth_iq_fm(L, 1e7, 2235, f_carrier=250e3, f_mod=1e3, dev=5.0)
    x = O.grid_c64(raw)

    class _Src3:
        length = L
    ck = chunker.chunker(_Src3(), 8192)
    out = comm.commSignal(11025)
    rz = filters.remez(10000000, [[0, 100e3], [150e3, 4999999]], [1, 0], ntaps=127)
    fm = demod_fm.demod_fm()
    for a, b in ck.getChunks:
        s = comm.commSignal(10000000, x[a:b], ck).offsetFreq(250000.0).filter(rz) \
            .bwLim(200000, uniq="First").funcApply(fm.demod).bwLim(11025, True)
        out.extend(s)
    g["seed"] = np.int64(2235)
    g["L"] = np.int64(L)
    g["chain_c3"] = np.array(out.signal)
    g["chain_c3_rate"] = np.int64(out.sampRate)
    g["taps_remez127"] = np.asarray(rz.getB, dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "chain_c3.npz"), **g)
    print("chain_c3:", len(g["chain_c3"]))

    # ------------------------------------------------------------------ C4: NOAA sync
    g = {}
    dur = 6.0
    raw = O.synth_apt_iq(dur, 2048000, seed=1)
    src = ArraySource(raw, 2048000)
    nobj = decode_noaa.decode_noaa(src, 30000.0)
    sa, sb = nobj.getCrudeSync()
    g["dur"] = np.float64(dur)
    g["crude_syncA"] = np.asarray(sa, dtype=np.int64)
    g["crude_syncB"] = np.asarray(sb, dtype=np.int64)
    g["useful"] = np.int64(nobj.useful)
    acc = nobj.getAccurateSync()
    g["acc_syncA"] = np.asarray(acc[0], dtype=np.int64)
    g["acc_syncA_pk"] = np.asarray(acc[2], dtype=np.float64)
    g["acc_syncA_time"] = np.asarray([np.nan if v is None else v for v in acc[3]], dtype=np.float64)
    g["acc_syncB"] = np.asarray(acc[4], dtype=np.int64)
    g["acc_syncB_pk"] = np.asarray(acc[6], dtype=np.float64)
    g["acc_syncB_time"] = np.asarray([np.nan if v is None else v for v in acc[7]], dtype=np.float64)

    # X1/X2 on the crude-rate envelope: store the envelope-stage outputs at reduced
    # length (3 s) for the op-level test
    aud = nobj._decode_noaa__audio(constants.NOAA_CRUDESYNCSAMPRATE, False)
    g["audio_rate"] = np.int64(aud.sampRate)
    n3 = 3 * aud.sampRate
    a3 = np.array(aud.signal[:n3])
    g["audio_3s_head"] = a3.astype(np.float64)[:20000]
    g["audio_3s_sum"] = np.float64(np.sum(a3.astype(np.float64)))
    amsig = nobj._decode_noaa__getAM(comm.commSignal(aud.sampRate, a3))
    g["am_3s_head"] = np.array(amsig.signal)[:20000]
    g["am_3s_sum"] = np.float64(np.sum(np.array(amsig.signal)))
    needle = ((np.repeat(constants.NOAA_SYNCA, round(aud.sampRate * constants.NOAA_T)) * 233) + 11) / 255
    xc = np.array(nobj._decode_noaa__correlate(np.array(amsig.signal), needle))
    g["xcorr_3s_syncA_head"] = xc[:20000]
    g["xcorr_3s_syncA_tail"] = xc[-2000:]
    g["xcorr_3s_syncA_sum"] = np.float64(np.sum(xc))
    g["peaks_3s_syncA"] = np.asarray(nobj._decode_noaa__correlateAndFindPeaks(amsig, constants.NOAA_SYNCA), dtype=np.int64)
    g["peaks_3s_syncB"] = np.asarray(nobj._decode_noaa__correlateAndFindPeaks(amsig, constants.NOAA_SYNCB), dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "noaa_c4.npz"), **g)
    print("noaa_c4: crude A", g["crude_syncA"][:4], "acc A", g["acc_syncA"][:4], "useful", g["useful"])

    gen_afsk(O, filters)


if __name__ == "__main__":
    main()
