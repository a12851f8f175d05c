#!/usr/bin/env python3
"""
Side benchmark of SSTV image decoding (decode_sstv): the time per stage -- front end, lag product, tone
classes, the two run searches, the header parse, the pixel sums, the colour conversion -- on

  * one complete PD120 image (VIS header and 248 line pairs of sstv.card, 127 s) as audio at 24 kS/s through fromAudio, and
  * the same transmission as FM (+-3 kHz) on a carrier 12.5 kHz above the centre of a 240 kS/s u8 IQ recording, tiled --tiles
    times into a recording as long as a pass, through decode_sstv(IQarray, 12500).

First call in the process and warm (median of --reps, a fresh decoder object each time, a device synchronisation after every
stage).  Nothing is gated on the numbers; DESIGN.md section 4.21 sets each kernel's bytes and operations beside what was measured
(one image from audio: lag 0.11 ms against an LDS bound of 61 us, classes 0.03 ms, both run searches 0.31 ms of launch and copy
latency, pixels 0.09 ms, colour 0.08 ms; 1.5 ms in all).  Prints one JSON line per workload.  The library must have been built
(python __graft_entry__.py).

    python tools/bench_sstv.py [--reps 3] [--tiles 4]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

RATE, FS, OFFSET, DEV = 24000, 240000, 12500, 3000.0


def fm_iq(audio, seed=41, amp=60.0, sigma=2.0):
    n = len(audio)
    rng = np.random.default_rng(seed)
    ph = 2 * np.pi * DEV * np.cumsum(audio) / FS + 2 * np.pi * ((OFFSET / FS * np.arange(n)) % 1.0)
    raw = np.empty((n, 2), dtype=np.uint8)
    raw[:, 0] = np.clip(np.round(amp * np.cos(ph) + sigma * rng.standard_normal(n) + 127.5), 0, 255).astype(np.uint8)
    raw[:, 1] = np.clip(np.round(amp * np.sin(ph) + sigma * rng.standard_normal(n) + 127.5), 0, 255).astype(np.uint8)
    return raw


def measure(make, reps, what, extra):
    from directdemod_amd import _hip

    def run():
        o = make()
        _hip.sync()
        t0 = time.perf_counter()
        images = o.getImages
        return o, images, time.perf_counter() - t0
    obj, images, first = run()
    runs = [run() for _ in range(reps)]
    assert all(len(r[1]) == len(images) and all(np.array_equal(a, b) for a, b in zip(r[1], images)) for r in runs)
    st = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    info = obj.imageInfo
    out = {"stage": what, "audio_samples": obj.audio().n, "audio_rate": obj.audioRate, "images": len(images),
           "rows": [i["rows"] for i in info], "syncs_matched": [i["syncs_matched"] for i in info],
           "slant_ppm": [round(i["slant_ppm"], 1) for i in info], "empty_pixels": [i["empty_pixels"] for i in info],
           "first_ms": round(first * 1e3, 3), "warm_ms": round(float(np.median([r[2] for r in runs])) * 1e3, 3),
           "warm_stage_ms": st, "device": _hip.device_name()}
    out.update(extra)
    print(json.dumps(out), flush=True)
    return images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=4)
    ap.add_argument("--mode", default="PD120")
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_sstv, source, sstv
    _hip.require_gpu()
    m = sstv.MODES[a.mode]
    y, cr, cb = sstv.card(m, m.height // 2)
    tones = sstv.tones(y, cr, cb, m)
    want = sstv.color_host(np.stack((y[0::2], cr, cb, y[1::2]), axis=1))

    def err(images):
        return [round(float(np.abs(i.astype(int) - want[:len(i)].astype(int))[:, 16:-16].mean()), 3) for i in images]
    audio = sstv.synth(*tones, RATE)
    images = measure(lambda: decode_sstv.decode_sstv.fromAudio(audio, RATE), a.reps, "sstv.fromAudio", {"mode": a.mode})
    print(json.dumps({"mean_abs_error_levels": err(images)}), flush=True)
    raw = np.tile(fm_iq(sstv.synth(*tones, FS)), (a.tiles, 1))
    src = source.IQarray(raw, FS)
    images = measure(lambda: decode_sstv.decode_sstv(src, OFFSET), a.reps, "sstv.decode_sstv",
                     {"mode": a.mode, "samples": int(raw.shape[0]), "tiles": a.tiles, "seconds": round(raw.shape[0] / FS, 1)})
    print(json.dumps({"mean_abs_error_levels": err(images)}), flush=True)


if __name__ == "__main__":
    main()
