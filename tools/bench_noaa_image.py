#!/usr/bin/env python3
"""
Side benchmark of the APT image stage (decode_noaa.getImage after getCrudeSync): wall time of the first call in the process
and warm (median of --reps, each on a fresh decoder object whose crude sync is done before the clock starts), for a 60 s
recording and a 900 s one.  The long recording is whole 0.5 s lines of a short synthesis, tiled (1 024 000 samples per line
at 2.048 MS/s).  Prints one JSON line per duration.

    python tools/bench_noaa_image.py [--reps 5] [--durations 60,900]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def recording(dur, fs=2048000):
    from oracle import dd_oracle as O
    if dur <= 60:
        return O.synth_apt_iq(dur, fs, seed=1)
    base = O.synth_apt_iq(10.0, fs, seed=1)                   # 20 whole lines
    line = fs // 2
    reps = int(dur / 10.0)
    return np.tile(base[:20 * line], (reps, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--durations", default="60,900")
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from directdemod_amd import decode_noaa, source, _hip
    _hip.require_gpu()
    for dur in [float(d) for d in a.durations.split(",")]:
        src = source.IQarray(recording(dur), 2048000)
        obj = decode_noaa.decode_noaa(src, 30000.0)
        obj.getCrudeSync()
        t0 = time.perf_counter()
        img = obj.getImage
        first = time.perf_counter() - t0
        warm = []
        for _ in range(a.reps):
            o = decode_noaa.decode_noaa(src, 30000.0)
            o.getCrudeSync()
            _hip.sync()
            t0 = time.perf_counter()
            im2 = o.getImage
            warm.append(time.perf_counter() - t0)
            assert np.array_equal(im2, img)
        print(json.dumps({"stage": "getImage", "duration_s": dur, "lines": int(img.shape[0]), "first_ms": round(first * 1e3, 3),
                          "warm_ms": round(float(np.median(warm)) * 1e3, 3), "warm_min_ms": round(min(warm) * 1e3, 3),
                          "device": _hip.device_name()}), flush=True)
        del src, obj


if __name__ == "__main__":
    main()
