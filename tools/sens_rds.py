"""Sensitivity of the RDS decoder: the groups decoded, word for word as sent, against the IQ noise level and against the RDS
injection level, by the float64 NumPy restatement (decode_rds.decode_host; no GPU) and, with --device, by the device chain
(decode_rds.decode_rds) over the same recordings.  Each recording is --groups groups of random content at 1.2 MS/s, the station
150 kHz above the centre at amplitude 60 of the u8 range, a 1 kHz tone at 30 % and the pilot at 9 % of the 75 kHz deviation beside
the RDS signal, the sample clock 40 ppm fast.  No threshold is fixed in advance: the tables are printed, and the level at which 90 %
of the groups still decode is read off them (INTEGRATION.md quotes both).

--taps compares lengths of the front end's Blackman-Harris window in the restatement (rds.window_taps is where the choice is kept);
--miscorrection prints the share of random 26-bit words that the burst repair takes for a block, per offset word and `fix`.

    python tools/sens_rds.py [--groups 40] [--device] [--taps 9 13 19 25 37] [--miscorrection]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from directdemod_amd import decode_rds, rds  # noqa: E402

FS, OFFSET, AMPLITUDE = 1200000, 150000.0, 60.0
SIGMAS = (4.0, 8.0, 12.0, 14.0, 16.0, 18.0, 20.0, 24.0)               # per rail, at the nominal injection
LEVELS = (0.04, 0.03, 0.02, 0.0175, 0.015, 0.0125, 0.01, 0.005)        # of the deviation (0.04 is +-3 kHz), at sigma 2
NOMINAL_LEVEL, LEVEL_SIGMA = 0.04, 2.0


def recording(groups, sigma, level, seed):
    rng = np.random.default_rng(seed)
    sent = [tuple(int(v) for v in rng.integers(0, 1 << 16, 4)) for _ in range(groups)]
    sent = [(0xD318, w1 & 0xF7FF, w2, w3) for _, w1, w2, w3 in sent]     # version A: the third block carries C
    raw = rds.encode(sent, FS, offset=OFFSET, amplitude=AMPLITUDE, sigma=sigma, seed=int(rng.integers(1 << 31)), level=level,
                     start=0.01 + rng.uniform(0.0, 1e-3), clock_ppm=40.0)
    return raw, sent


def kept(found, sent):
    """groups decoded word for word as sent (each sent group counted once)"""
    left = list(sent)
    n = 0
    for g in found:
        w = tuple(g["words"])
        if w in left:
            left.remove(w)
            n += 1
    return n


def point(raw, sent, device, taps=None):
    mpx, rate = rds.audio_host(raw, FS, OFFSET, decode_rds.BW, taps)
    out = [kept(decode_rds.decode_audio_host(mpx, rate)[0], sent)]
    if device:
        from directdemod_amd import source
        out.append(kept(decode_rds.decode_rds(source.IQarray(np.array(raw), FS), OFFSET).getGroups, sent))
    return out


def sweep(name, values, groups, device, make):
    print("\n%s: groups decoded of %d, %s" % (name, groups, "host / device" if device else "host (float64 restatement)"))
    print("| %s | decoded |" % name)
    print("|---|---|")
    for k, v in enumerate(values):
        raw, sent = make(v, 100 + k)
        print("| %g | %s |" % (v, " / ".join(str(n) for n in point(raw, sent, device))), flush=True)


def miscorrection(words=200000, seed=7):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 26, words)
    rem = rds.remainder(w)
    print("\nrandom 26-bit words taken for a block (clean or repaired), of %d per offset word" % words)
    print("| fix | " + " | ".join("ABCcD"[o] if o != 3 else "C'" for o in range(5)) + " | expected |")
    print("|---|" + "---|" * 6)
    for fix in (0, 2, 5):
        ok = {r for _, r, ln, _ in rds.bursts() if ln <= fix} | {0}
        row = [int(np.isin(rem ^ rds.OFFSETS[o], list(ok)).sum()) for o in range(5)]
        print("| %d | " % fix + " | ".join("%.4f" % (n / words) for n in row) + " | %.4f |" % (len(ok) / 1024.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=40)
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--taps", type=int, nargs="*", default=None)
    ap.add_argument("--miscorrection", action="store_true")
    a = ap.parse_args()
    if a.device:
        from directdemod_amd import _hip
        _hip.require_gpu()
    d, sps, _ = rds.params(FS / int(FS / decode_rds.BW))
    print("%d S/s recording, multiplex at %g S/s, D = %d, %.3f samples per bit, window of %d taps" %
          (FS, FS / int(FS / decode_rds.BW), d, sps, rds.window_taps(FS)))
    sweep("noise sigma per rail", SIGMAS, a.groups, a.device, lambda v, s: recording(a.groups, v, NOMINAL_LEVEL, s))
    sweep("injection level", LEVELS, a.groups, a.device, lambda v, s: recording(a.groups, LEVEL_SIGMA, v, s))
    if a.taps:
        print("\nwindow length (restatement): groups decoded of %d at noise sigma 16 / 24" % a.groups)
        recs = [recording(a.groups, s, NOMINAL_LEVEL, 300 + k) for k, s in enumerate((16.0, 24.0))]
        print("| taps | null to null, kHz | decoded |")
        print("|---|---|---|")
        for taps in a.taps:
            print("| %d | +-%.0f | %s |" % (taps, 4e-3 * FS / taps, " / ".join(str(point(raw, sent, False, taps)[0]) for raw, sent in recs)),
                  flush=True)
    if a.miscorrection:
        miscorrection()


if __name__ == "__main__":
    main()
