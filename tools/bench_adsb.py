#!/usr/bin/env python3
"""
Side benchmark of Mode S / ADS-B decoding (decode_adsb): the time per stage -- upload of the raw pairs,
the preamble candidates, the demodulation of the survivors, the host's acceptance -- on a synthesised recording at 2.4 MS/s: one
second holding --frames published frames at random fractional starts, amplitudes 25 to 80 and carrier offsets within +-50 kHz
over noise of sigma 3 per rail, tiled --duration times (60: 144 000 000 samples, a few thousand frames).

First call in the process and warm (median of --reps, a fresh decoder object each time over an IQarray whose pairs stay resident
on the device, a device synchronisation after every stage).  Nothing is gated on the numbers; DESIGN.md section 4.22 sets each
kernel's bytes and operations beside what was measured.  Prints one JSON line.  The library must have been built
(python __graft_entry__.py).

    python tools/bench_adsb.py [--reps 3] [--duration 60] [--frames 50]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

RATE = 2400000
FRAMES = ["8D4840D6202CC371C32CE0576098", "8D40621D58C382D690C8AC2863A7", "8D40621D58C386435CC412692AD6", "8D485020994409940838175B284F",
          "8DA05F219B06B6AF189400CBC33F", "8D40058B58C901375147EFD09357", "8D40058B58C904A87F402D3B8C59", "5D4840D6F8740F"]


def second(frames, seed=31):
    """one second of recording with `frames` frames, none starting inside another"""
    from directdemod_amd import adsb
    rng = np.random.default_rng(seed)
    slot = (RATE - 400) // frames
    starts = slot * np.arange(frames) + rng.uniform(0.0, slot - 300.0, frames)
    sent = [FRAMES[i % len(FRAMES)] for i in range(frames)]
    raw = adsb.encode(sent, RATE, starts, rng.uniform(25.0, 80.0, frames), 3.0, seed, rng.uniform(-50e3, 50e3, frames), n=RATE)
    return raw, sent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=int, default=60)
    ap.add_argument("--frames", type=int, default=50)
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_adsb, source
    _hip.require_gpu()
    one, sent = second(a.frames)
    raw = np.tile(one, (a.duration, 1))

    def run(src):
        o = decode_adsb.decode_adsb(src)
        _hip.sync()
        t0 = time.perf_counter()
        msgs = o.getMsgs
        return o, msgs, time.perf_counter() - t0
    obj, msgs, first = run(source.IQarray(raw, RATE))                # (the first call uploads the recording)
    src = source.IQarray(raw, RATE)
    src.read_device_raw(0, len(raw))
    runs = [run(src) for _ in range(a.reps)]
    assert all([m["raw"] for m in r[1]] == [m["raw"] for m in msgs] for r in runs)
    info = obj.frameInfo
    stages = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    warm = float(np.median([r[2] for r in runs]))
    print(json.dumps({"stage": "decode_adsb", "samples": int(len(raw)), "seconds": a.duration, "rate": RATE, "phases": info["phases"],
                      "frames_sent": a.frames * a.duration, "messages": len(msgs), "candidates": info["candidates"],
                      "passed": info["passed"], "clean": info["clean"], "repaired": info["repaired"], "duplicates": info["duplicates"],
                      "first_ms": round(first * 1e3, 3), "first_stage_ms": {k: round(v * 1e3, 3) for k, v in obj.timings.items()},
                      "warm_ms": round(warm * 1e3, 3), "warm_stage_ms": stages,
                      "candidates_ns_per_sample": round(stages["candidates"] * 1e6 / len(raw), 4),
                      "demod_us_per_survivor": round(stages["demod"] * 1e3 / max(info["passed"], 1), 4),
                      "device": _hip.device_name()}), flush=True)


if __name__ == "__main__":
    main()
