#!/usr/bin/env python3
"""
Side benchmark of Funcube sync detection (decode_funcube.getSyncs): first call in the process and warm (median of --reps, a fresh
decoder object each time) on a 2.048 MS/s u8 IQ recording tiled from tests/_funcube.py's case (b) synthesis (the signal 30 kHz
above the centre), with the time per stage of the warm runs (mixer, low-pass, walk, lim, MINSYNC, MAXSYNC).  Prints one JSON line.

    python tools/bench_funcube.py [--reps 3] [--duration 60] [--no-build]
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
    import _funcube
    base, off, _ = _funcube.case("b")
    return np.tile(base, (int(np.ceil(dur * _funcube.FS / base.shape[0])), 1))[:int(dur * _funcube.FS)], _funcube.FS, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=float, default=60.0)
    ap.add_argument("--no-build", action="store_true", help="use the library as it stands")
    a = ap.parse_args()
    if not a.no_build:
        import __graft_entry__ as ge
        ge.build()
    import _funcube
    from directdemod_amd import _hip, decode_funcube, source
    _hip.require_gpu()
    raw, fs, offset = recording(a.duration)
    src = source.IQarray(raw, fs)

    def decoder():
        return decode_funcube.decode_funcube(src, offset, None, _funcube.CENTER, _funcube.CHANNEL)
    t0 = time.perf_counter()
    obj = decoder()
    syncs = obj.getSyncs
    first = time.perf_counter() - t0
    nsym = obj.walker().nsym
    warm, stages = [], []
    for _ in range(a.reps):
        o = decoder()
        _hip.sync()
        t0 = time.perf_counter()
        assert o.getSyncs == syncs
        warm.append(time.perf_counter() - t0)
        stages.append(o.timings)
    st = {k: round(float(np.median([s[k] for s in stages])) * 1e3, 3) for k in stages[0]}
    wm = float(np.median(warm))
    print(json.dumps({"stage": "funcube.getSyncs", "duration_s": a.duration, "samples": int(raw.shape[0]), "symbols": nsym,
                      "minsyncs": len(o.minsyncs), "maxsyncs": len(o.argmax), "syncs": len(syncs), "useful": o.useful,
                      "first_ms": round(first * 1e3, 3), "warm_ms": round(wm * 1e3, 3), "warm_min_ms": round(min(warm) * 1e3, 3),
                      "us_per_symbol": round(wm * 1e6 / max(nsym, 1), 4), "warm_stage_ms": st, "device": _hip.device_name()}),
          flush=True)


if __name__ == "__main__":
    main()
