"""Sensitivity of the POCSAG decoder by the NumPy restatement (no GPU): the share of pages decoded against Eb/N0 and carrier error,
for fix = 0, 1 and 2 repaired bits per codeword, at --baud (1200) on a 240 kS/s recording cut to 48 kS/s audio.  Each recording holds
ten transmissions of one batch with two pages (ten random digits; twenty random letters) 25 kHz above the centre; a page counts
when its address, function and text are among the complete decoded pages.  Eb/N0 = A^2 fs / (2 sigma^2 baud) for amplitude A and
noise sigma per rail.  Prints the table INTEGRATION.md quotes.

    python tools/sens_pocsag.py [--pages 100] [--baud 1200]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from directdemod_amd import pocsag  # noqa: E402

FS, BW, OFFSET = 240000, 48000.0, 25000.0
EBN0 = range(6, 22, 2)
ERRORS = (0, 500, -500, 1000, -1000)
AMPLITUDE = 40.0
PREAMBLE = 64                                                         # the decoder does not use it


def point(baud, ebn0_db, error, pages, seed):
    """pages found per fix of 0, 1, 2"""
    sigma = AMPLITUDE * np.sqrt(FS / (2.0 * baud * 10.0 ** (ebn0_db / 10.0)))
    rng = np.random.default_rng(seed)
    found = [0, 0, 0]
    span = (PREAMBLE + pocsag.BATCH_BITS + 40) * FS / float(baud)
    for rec in range(pages // 20):
        txs = []
        for _ in range(10):
            digits = "".join(str(d) for d in rng.integers(0, 10, 10))
            letters = "".join(chr(c) for c in rng.integers(97, 123, 20))
            txs.append([(int(rng.integers(0, 1 << 18)) << 3, 0, digits), (int(rng.integers(0, 1 << 18)) << 3 | 4, 3, letters)])
        starts = 1000.0 + np.arange(10) * span + rng.uniform(0.0, 50.0, 10)
        raw = pocsag.encode(txs, FS, starts, baud, 0, OFFSET, AMPLITUDE, sigma, seed=int(rng.integers(1 << 31)),
                            carrier_offsets=float(error), n=int(starts[-1] + span), preamble=PREAMBLE)
        audio, rate = pocsag.audio_host(raw, FS, OFFSET, BW)
        for fix in (0, 1, 2):
            got = {(p["address"], p["function"], p["text"]) for p in pocsag.decode(audio, rate, (baud,), fix=fix)[0] if p["complete"]}
            found[fix] += sum(1 for tx in txs for page in tx if page in got)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=100)
    ap.add_argument("--baud", type=int, default=1200)
    a = ap.parse_args()
    pages = a.pages // 20 * 20
    sps, w, _, _ = pocsag.params(BW, a.baud)
    print("%d S/s recording, %g S/s audio, %d baud, %g samples per bit, w = %d; decoded of %d pages for fix = 0 / 1 / 2"
          % (FS, BW, a.baud, sps, w, pages))
    print("| Eb/N0 dB | " + " | ".join("%+g kHz" % (e / 1000.0) if e else "0" for e in ERRORS) + " |")
    print("|---|" + "---|" * len(ERRORS))
    for db in EBN0:
        row = [point(a.baud, db, e, pages, 1000 * db + i) for i, e in enumerate(ERRORS)]
        print("| %d | " % db + " | ".join("%d / %d / %d" % tuple(v) for v in row) + " |", flush=True)


if __name__ == "__main__":
    main()
