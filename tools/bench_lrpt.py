#!/usr/bin/env python3
"""
Side benchmark of Meteor-M2 LRPT decoding (decode_meteorm2.getFrames, getPackets): the time per stage of the frame decoder (lrpt_soft,
lrpt_asm, lrpt_viterbi, lrpt_finish), of Reed-Solomon correction (lrpt_rs) and of packet reassembly (lrpt_packets) beside the stages of
the decode pass they start from (front end, walk, lim, MINSYNC, MAXSYNC), on a 2.048 MS/s u8 IQ recording tiled from tests/_lrpt.py's
case (a) (random bodies: no codeword is decodable, the Reed-Solomon stage's longest way) or tests/_rs.py's case (b) (real frames and
packets, two fades per tile).  Frames break at the tile seams; the decoder simply finds the whole ones.  First call in the process and
warm (median of --reps, a fresh decoder object each time).  Prints one JSON line.  The library must have been built
(python __graft_entry__.py).

A tiled case (b) repeats its frames' counters: each tile delivers the same packets again, and whatever packet is under way at a seam
is dropped there, by the counter's jump back or by the broken frame.  "packets" counts them all, "packets_distinct" the different ones.

    python tools/bench_lrpt.py [--reps 3] [--duration 60] [--case a|b]
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


def recording(dur, case="a"):
    import _lrpt
    import _rs
    base = (_lrpt if case == "a" else _rs).case(case)[0]
    n = int(dur * _lrpt.FS)
    return np.tile(base, (-(-n // base.shape[0]), 1))[:n], _lrpt.FS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=float, default=60.0)
    ap.add_argument("--case", choices=("a", "b"), default="a")
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_meteorm2, source
    _hip.require_gpu()
    raw, fs = recording(a.duration, a.case)
    src = source.IQarray(raw, fs)

    def run():
        o = decode_meteorm2.decode_meteorm2(src, 0, None)
        _hip.sync()
        t0 = time.perf_counter()
        o.getSyncs
        t1 = time.perf_counter()
        frames = o.getFrames
        t2 = time.perf_counter()
        o.getPackets
        return o, frames, t1 - t0, t2 - t1, time.perf_counter() - t2
    obj, frames, first_pass, first_frames, first_packets = run()
    runs = [run() for _ in range(a.reps)]
    assert all(np.array_equal(r[1], frames) for r in runs)
    st = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    info = obj.frameInfo
    assert all(r[0].getPackets == obj.getPackets for r in runs)
    print(json.dumps({"stage": "meteorm2.getFrames", "case": a.case, "duration_s": a.duration, "samples": int(raw.shape[0]), "symbols": obj.walker().nsym,
                      "frames": int(len(frames)), "frames_asm_clean": int(np.sum(info["asm_errors"] == 0)),
                      "frames_rs_ok": int(np.sum(obj.rsInfo["ok"])), "frames_rs_corrected": int(np.sum(obj.rsInfo["ok"] & (obj.rsInfo["errors"].max(axis=1) > 0))),
                      "packets": len(obj.getPackets), "packets_distinct": len(set(obj.getPackets)),
                      "first_pass_ms": round(first_pass * 1e3, 3), "first_frames_ms": round(first_frames * 1e3, 3),
                      "first_packets_ms": round(first_packets * 1e3, 3),
                      "warm_pass_ms": round(float(np.median([r[2] for r in runs])) * 1e3, 3),
                      "warm_frames_ms": round(float(np.median([r[3] for r in runs])) * 1e3, 3),
                      "warm_packets_ms": round(float(np.median([r[4] for r in runs])) * 1e3, 3),
                      "warm_stage_ms": st, "device": _hip.device_name()}), flush=True)


if __name__ == "__main__":
    main()
