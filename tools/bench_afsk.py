#!/usr/bin/env python3
"""
Side benchmark of AFSK1200 decoding (decode_afsk1200.getMsg): first call in the process and warm (median of --reps, a fresh decoder
object each time) on a config-1-shape recording (2.4 MS/s u8 IQ, the signal 10 kHz above the centre, AX.25 frames back to back),
with the time per stage of the warm runs (front end, band-pass, correlators, peaks, bits, frames).  The recording is a 5 s
synthesis (tests/_ax25.py) tiled to --duration.  Prints one JSON line.

    python tools/bench_afsk.py [--reps 5] [--duration 60]
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


def recording(dur, fs=2400000, offset=10000):
    import _ax25
    frames = [(("APRS", 0), ("N0CALL", k % 16), _ax25.INFO + " #%02d" % k, (("WIDE1", 1),)) for k in range(13)]
    base, _ = _ax25.recording(frames, fs, 31, lead_flags=20, f_carrier=float(offset))
    base = base[:5 * fs]
    return np.tile(base, (int(np.ceil(dur / 5.0)), 1))[:int(dur * fs)], fs, offset


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--duration", type=float, default=60.0)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from directdemod_amd import _hip, decode_afsk1200, source
    _hip.require_gpu()
    raw, fs, offset = recording(a.duration)
    src = source.IQarray(raw, fs)
    t0 = time.perf_counter()
    obj = decode_afsk1200.decode_afsk1200(src, offset, 22050)
    msg = obj.getMsg
    first = time.perf_counter() - t0
    nframes = len(obj.getFrames)
    warm, stages = [], []
    for _ in range(a.reps):
        o = decode_afsk1200.decode_afsk1200(src, offset, 22050)
        _hip.sync()
        t0 = time.perf_counter()
        assert o.getMsg == msg
        warm.append(time.perf_counter() - t0)
        stages.append(o.timings)
        assert len(o.getFrames) == nframes
    st = {k: round(float(np.median([s[k] for s in stages])) * 1e3, 3) for k in stages[0]}
    print(json.dumps({"stage": "afsk1200.getMsg", "duration_s": a.duration, "samples": int(raw.shape[0]), "frames": nframes,
                      "first_ms": round(first * 1e3, 3), "warm_ms": round(float(np.median(warm)) * 1e3, 3),
                      "warm_min_ms": round(min(warm) * 1e3, 3), "warm_stage_ms": st, "device": _hip.device_name()}), flush=True)


if __name__ == "__main__":
    main()
