#!/usr/bin/env python3
"""
Side benchmark of Meteor-M2 sync detection (decode_meteorm2.getSyncs): first call in the process and warm (median of --reps, a
fresh decoder object each time) on a 2.048 MS/s u8 IQ recording tiled from tests/_meteor.py's case (b) synthesis (the signal 30 kHz
above the centre), with the time per stage of the warm runs (front end, walk, lim, MINSYNC, MAXSYNC).  Prints one JSON line.

    python tools/bench_meteor.py [--reps 3] [--duration 60]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def recording(dur):
    import _meteor
    base, off = _meteor.case("b")
    return np.tile(base, (int(np.ceil(dur * _meteor.FS / base.shape[0])), 1))[:int(dur * _meteor.FS)], _meteor.FS, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=float, default=60.0)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from directdemod_amd import _hip, decode_meteorm2, source
    _hip.require_gpu()
    raw, fs, offset = recording(a.duration)
    src = source.IQarray(raw, fs)
    t0 = time.perf_counter()
    obj = decode_meteorm2.decode_meteorm2(src, offset, None)
    syncs = obj.getSyncs
    first = time.perf_counter() - t0
    nsym = obj.walker().nsym
    warm, stages = [], []
    for _ in range(a.reps):
        o = decode_meteorm2.decode_meteorm2(src, offset, None)
        _hip.sync()
        t0 = time.perf_counter()
        assert o.getSyncs == syncs
        warm.append(time.perf_counter() - t0)
        stages.append(o.timings)
    st = {k: round(float(np.median([s[k] for s in stages])) * 1e3, 3) for k in stages[0]}
    wm = float(np.median(warm))
    print(json.dumps({"stage": "meteorm2.getSyncs", "duration_s": a.duration, "samples": int(raw.shape[0]), "symbols": nsym,
                      "syncs": len(syncs), "useful": o.useful, "first_ms": round(first * 1e3, 3), "warm_ms": round(wm * 1e3, 3),
                      "warm_min_ms": round(min(warm) * 1e3, 3), "us_per_symbol": round(wm * 1e6 / max(nsym, 1), 4),
                      "warm_stage_ms": st, "device": _hip.device_name()}), flush=True)


if __name__ == "__main__":
    main()
