#!/usr/bin/env python3
"""
Side benchmark of Meteor-M2 LRPT frame decoding (decode_meteorm2.getFrames): the time per stage of the frame decoder (lrpt_soft,
lrpt_asm, lrpt_viterbi, lrpt_finish) beside the stages of the decode pass it starts from (front end, walk, lim, MINSYNC, MAXSYNC), on
a 2.048 MS/s u8 IQ recording tiled from tests/_lrpt.py's case (a) (frames break at the tile seams; the decoder simply finds the
whole ones).  First call in the process and warm (median of --reps, a fresh decoder object each time).  Prints one JSON line.
The library must have been built (python __graft_entry__.py).

    python tools/bench_lrpt.py [--reps 3] [--duration 60]
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
    import _lrpt
    base = _lrpt.case("a")[0]
    n = int(dur * _lrpt.FS)
    return np.tile(base, (-(-n // base.shape[0]), 1))[:n], _lrpt.FS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=float, default=60.0)
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_meteorm2, source
    _hip.require_gpu()
    raw, fs = recording(a.duration)
    src = source.IQarray(raw, fs)

    def run():
        o = decode_meteorm2.decode_meteorm2(src, 0, None)
        _hip.sync()
        t0 = time.perf_counter()
        o.getSyncs
        t1 = time.perf_counter()
        frames = o.getFrames
        return o, frames, t1 - t0, time.perf_counter() - t1
    obj, frames, first_pass, first_frames = run()
    runs = [run() for _ in range(a.reps)]
    assert all(np.array_equal(r[1], frames) for r in runs)
    st = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    info = obj.frameInfo
    print(json.dumps({"stage": "meteorm2.getFrames", "duration_s": a.duration, "samples": int(raw.shape[0]), "symbols": obj.walker().nsym,
                      "frames": int(len(frames)), "frames_asm_clean": int(np.sum(info["asm_errors"] == 0)),
                      "first_pass_ms": round(first_pass * 1e3, 3), "first_frames_ms": round(first_frames * 1e3, 3),
                      "warm_pass_ms": round(float(np.median([r[2] for r in runs])) * 1e3, 3),
                      "warm_frames_ms": round(float(np.median([r[3] for r in runs])) * 1e3, 3),
                      "warm_stage_ms": st, "device": _hip.device_name()}), flush=True)


if __name__ == "__main__":
    main()
