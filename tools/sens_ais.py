"""Sensitivity of the AIS decoder by the NumPy restatement (no GPU): decode rate against Eb/N0 and carrier error, 200 bursts per point,
at 5 and at 4.27 samples per bit.  Each recording holds 20 bursts of 168 random message bits on the channel 25 kHz below the centre;
a burst counts when its bytes are among the decoded messages.  Eb/N0 = A^2 fs / (2 sigma^2 9600) for amplitude A and noise sigma
per rail.  Prints the table INTEGRATION.md quotes.

    python tools/sens_ais.py [--bursts 200]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from directdemod_amd import ais, decode_ais  # noqa: E402

RATES = ((240000, 48000.0), (204800, 40960.0))            # (recording rate, bw): 5 and 4.2667 samples per bit
EBN0 = range(8, 26, 2)
ERRORS = (0, 1000, -1000, 2000, -2000, 3000, -3000)
AMPLITUDE = 40.0


def point(fs, bw, ebn0_db, error, bursts, seed):
    sigma = AMPLITUDE * np.sqrt(fs / (2.0 * ais.BAUD * 10.0 ** (ebn0_db / 10.0)))
    rng = np.random.default_rng(seed)
    found = 0
    for rec in range(bursts // 20):
        msgs = [rng.integers(0, 256, 21).astype(np.uint8).tobytes() for _ in range(20)]
        starts = 1000.0 + np.arange(20) * fs * 0.03 + rng.uniform(0.0, fs * 0.002, 20)
        raw = ais.encode(msgs, fs, starts, -25000.0, AMPLITUDE, sigma, seed=int(rng.integers(1 << 31)), carrier_offsets=float(error),
                         n=int(starts[-1] + fs * 0.03))
        got = {m["raw"] for m in decode_ais.decode_host(raw, fs, (-25000.0,), bw)[0]}
        found += sum(1 for m in msgs if m in got)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bursts", type=int, default=200)
    a = ap.parse_args()
    for fs, bw in RATES:
        rate = fs / int(fs / bw)
        print("\n%d S/s recording, %g S/s audio, %.4f samples per bit, w = %d; decoded of %d" % (fs, rate, rate / ais.BAUD,
                                                                                               ais.params(rate)[1], a.bursts))
        print("| Eb/N0 dB | " + " | ".join("%+d kHz" % (e // 1000) if e else "0" for e in ERRORS) + " |")
        print("|---|" + "---|" * len(ERRORS))
        for db in EBN0:
            row = [point(fs, bw, db, e, a.bursts, 1000 * db + i) for i, e in enumerate(ERRORS)]
            print("| %d | " % db + " | ".join(str(v) for v in row) + " |", flush=True)


if __name__ == "__main__":
    main()
