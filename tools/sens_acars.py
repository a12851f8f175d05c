"""Sensitivity of the ACARS decoder by the NumPy restatement (no GPU): the share of blocks decoded against carrier-to-noise ratio and
baud-rate error, for fix = 0, 1 and 2 repaired bits per block, on a 240 kS/s recording cut to 48 kS/s audio.  Each recording holds
ten blocks of --chars (40) random text characters 25 kHz above the centre, AM of depth 0.8; a block counts when its bytes are
among the decoded blocks'.  C/N = A^2 / (2 sigma^2) over the audio filter's two-sided bandwidth of 2 x 5 kHz, that is
C/N0 = A^2 fs / (2 sigma^2) less 40 dB, for carrier amplitude A and noise sigma per rail.  A baud-rate error of e ppm stretches the
transmitter's bit time by 1 + e / 10^6: the decoder times every bit from the template alone, so bit k lands k e / 10^6 bit times
late.  Prints the table INTEGRATION.md quotes.

    python tools/sens_acars.py [--blocks 100] [--chars 40]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from directdemod_amd import acars  # noqa: E402

FS, BW, OFFSET = 240000, 48000.0, 25000.0
CN = range(4, 20, 2)
PPM = (0, 100, -100, 200, -200, 400)
AMPLITUDE = 40.0


def point(cn_db, ppm, blocks, chars, seed):
    """blocks found per fix of 0, 1, 2"""
    sigma = AMPLITUDE * np.sqrt(FS / (2.0 * 2.0 * acars.CUT * 10.0 ** (cn_db / 10.0)))
    rng = np.random.default_rng(seed)
    found = [0, 0, 0]
    fs_tx = FS * (1.0 + ppm * 1e-6)                                   # the transmitter's bits, a little long or short
    span = (8 * (acars.PREKEY + 5 + 17 + chars) + 40) * FS / float(acars.BAUD)
    for rec in range(blocks // 10):
        blks = [acars.block_bytes("2", "N%05d" % rng.integers(0, 100000), None, "H1", str(rng.integers(0, 10)),
                                  "".join(chr(c) for c in rng.integers(32, 127, chars))) for _ in range(10)]
        starts = 1000.0 + np.arange(10) * span + rng.uniform(0.0, 100.0, 10)
        raw = acars.encode(blks, fs_tx, starts, OFFSET * fs_tx / FS, 0.8, AMPLITUDE, sigma, seed=int(rng.integers(1 << 31)),
                           n=int(starts[-1] + span))
        audio, rate = acars.audio_host(raw, FS, OFFSET, BW)
        for fix in (0, 1, 2):
            got = {b["bytes"] for b in acars.decode([audio], rate, ["A"], fix=fix)[0]}
            found[fix] += sum(1 for b in blks if b[:-1] in got)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=100)
    ap.add_argument("--chars", type=int, default=40)
    a = ap.parse_args()
    blocks = a.blocks // 10 * 10
    sps, w, _, _ = acars.params(BW)
    print("%d S/s recording, %g S/s audio, %g samples per bit, w = %d, %d text characters (%d bits behind the template); decoded of "
          "%d blocks for fix = 0 / 1 / 2" % (FS, BW, sps, w, a.chars, 8 * (17 + a.chars), blocks))
    print("| C/N dB | " + " | ".join("%+d ppm" % e if e else "0" for e in PPM) + " |")
    print("|---|" + "---|" * len(PPM))
    for db in CN:
        row = [point(db, e, blocks, a.chars, 1000 * db + i) for i, e in enumerate(PPM)]
        print("| %d | " % db + " | ".join("%d / %d / %d" % tuple(v) for v in row) + " |", flush=True)


if __name__ == "__main__":
    main()
