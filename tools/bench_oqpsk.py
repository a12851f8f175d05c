#!/usr/bin/env python3
"""
Side benchmark of Meteor-M N2-x decoding from IQ (decode_meteorm2x.getFrames): the time per stage -- the front
end (NCO and low-pass), the OQPSK walk, and decode_lrpt's stages behind them, the stagger search among them -- on a 2.048 MS/s u8 IQ
recording tiled from tests/_oqpsk.py's 0.9 s recordings at 72 and at 80 ksym/s (differential, not interleaved: the interleaver
would spread every bit far beyond a tile).  A tile holds a whole number of symbols and of carrier cycles, so timing and carrier run
through the seams; the frames break there and the decoder finds the whole ones.  First call in the process and warm (median of
--reps, a fresh decoder object each time); the walk's time per symbol is the figure to set beside tools/bench_meteor.py's.  Prints
one JSON line per symbol rate.  The library must have been built (python __graft_entry__.py).

    python tools/bench_oqpsk.py [--reps 3] [--duration 60] [--rates 72000 80000]
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


def recording(dur, rate):
    import _oqpsk
    rec = _oqpsk.recording(**_oqpsk.RECORDINGS["72k_s0" if rate == 72000 else "80k_s0"])
    n = int(dur * _oqpsk.FS)
    return np.tile(rec["raw"], (-(-n // rec["raw"].shape[0]), 1))[:n], _oqpsk.FS, rec["carrier"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=float, default=60.0)
    ap.add_argument("--rates", type=int, nargs="+", default=[72000, 80000])
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_meteorm2x, source
    _hip.require_gpu()
    for rate in a.rates:
        raw, fs, offset = recording(a.duration, rate)
        src = source.IQarray(raw, fs)

        def run():
            o = decode_meteorm2x.decode_meteorm2x(src, offset, symbol_rate=rate)
            _hip.sync()
            t0 = time.perf_counter()
            frames = o.getFrames
            return o, frames, time.perf_counter() - t0
        obj, frames, first = run()
        runs = [run() for _ in range(a.reps)]
        assert all(np.array_equal(r[1], frames) for r in runs)
        nsym = obj.walker().nsym
        st = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
        print(json.dumps({"stage": "meteorm2x.getFrames", "symbol_rate": rate, "duration_s": a.duration, "samples": int(raw.shape[0]),
                          "symbols": nsym, "stagger": obj.stagger, "frames": int(len(frames)),
                          "frames_asm_clean": int(np.sum(obj.frameInfo["asm_errors"] == 0)),
                          "first_ms": round(first * 1e3, 3), "warm_ms": round(float(np.median([r[2] for r in runs])) * 1e3, 3),
                          "warm_stage_ms": st, "walk_us_per_symbol": round(st["walk"] * 1e3 / max(nsym, 1), 4),
                          "walk_ns_per_sample": round(st["walk"] * 1e6 / raw.shape[0], 3), "device": _hip.device_name()}), flush=True)


if __name__ == "__main__":
    main()
