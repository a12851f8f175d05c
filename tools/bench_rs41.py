#!/usr/bin/env python3
"""
Side benchmark of RS41 radiosonde decoding (decode_rs41): the time per stage -- the front end, the header
candidates, the demodulation and Reed-Solomon correction of the survivors, the host's merge, follow and parse -- on a synthesised
recording at 2.4 MS/s: five seconds holding five frames of one sonde a second apart, the third extended (25 kHz above the centre,
amplitude 40, noise of sigma 6 per rail), tiled --duration / 5 times (60: a minute, 60 frames, 144 000 000 samples).  The frames
decoded are checked against what was encoded.

The candidates stage and the candidate kernel alone (between two events) are printed beside the memory bound, one float64 read and
one mask byte written per audio sample at 8 TB/s; the frame kernel beside its own, the 2 h + 1 float64 samples of each of a
survivor's bits read once and two 518-byte frames written.  First call in the process and warm (median of --reps, a fresh decoder
object each time over an IQarray whose pairs stay resident on the device, a device synchronisation after every stage).  Nothing is
gated on the numbers.  Prints one JSON line.  The library must have been built (python __graft_entry__.py).

    python tools/bench_rs41.py [--reps 3] [--duration 60]
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
OFFSET = 25000.0
BLOCK = 5                                                             # seconds synthesised
HBM = 8.0e12                                                          # bytes per second
FIELDS = dict(serial="S1234567", battery=2.7, gps_week=2337, lat=48.2082, lon=16.3738, alt=18234.56, speed=23.4, heading=271.0,
              climb=5.2, sats=9, meas_raw=[100000 + 4099 * i for i in range(12)])


def fields():
    out = [dict(FIELDS, frame_number=4000 + k, subframe=k, gps_tow=302400000 + 1000 * k, alt=18234.56 + 5.2 * k) for k in range(BLOCK)]
    out[2]["xdata"] = bytes(range(40))
    return out


def block(seed=43):
    """five seconds of recording with the five frames a second apart"""
    from directdemod_amd import rs41
    return rs41.encode_iq(fields(), RATE, OFFSET, start=5000.3, amplitude=40.0, sigma=6.0, seed=seed, n=BLOCK * RATE)


def kernel_us(audio, rate, lst, m, reps=5):
    """(k_rs41_sync alone over the audio, with the memset of its masks; k_rs41_frame alone over the m survivors), each between two
    events, the least of `reps` in microseconds"""
    import ctypes as C
    from directdemod_amd import _hip, rs41
    L = _hip.lib()
    a, b = C.c_void_p(), C.c_void_p()
    _hip.check(L.dd_event_create(C.byref(a)), "dd_event_create")
    _hip.check(L.dd_event_create(C.byref(b)), "dd_event_create")
    sps, w, slack = rs41.params(rate)
    mask = _hip.DevArray(audio.n, np.uint8)
    fixed, recv, meta = _hip.DevArray(rs41.EXT * m, np.uint8), _hip.DevArray(rs41.EXT * m, np.uint8), _hip.DevArray(6 * m, np.int32)
    calls = {"sync": lambda: L.dd_debug_rs41_masks(audio.ptr, audio.n, sps, w, slack, mask.ptr, None),
             "frame": lambda: L.dd_rs41_frames(audio.ptr, audio.n, sps, w, lst.ptr, m, fixed.ptr, recv.ptr, meta.ptr, None)}
    out = {}
    for name, call in calls.items():
        times = []
        for _ in range(reps + 1):                                     # (the first is a warm-up)
            L.dd_event_record(a, None)
            _hip.check(call(), name)
            L.dd_event_record(b, None)
            ms = C.c_float(0.0)
            _hip.check(L.dd_event_elapsed_ms(a, b, C.byref(ms)), "dd_event_elapsed_ms")
            times.append(ms.value)
        out[name] = round(min(times[1:]) * 1e3, 2)
    L.dd_event_destroy(a)
    L.dd_event_destroy(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=int, default=60)
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_rs41, rs41, source
    _hip.require_gpu()
    tiles = max(1, a.duration // BLOCK)
    raw = np.tile(block(), (tiles, 1))
    want = [(f["frame_number"], "xdata" in f) for f in fields()] * tiles

    def run(src):
        o = decode_rs41.decode_rs41(src, OFFSET)
        _hip.sync()
        t0 = time.perf_counter()
        frames = o.getFrames
        return o, frames, time.perf_counter() - t0
    obj, frames, first = run(source.IQarray(raw, RATE))               # (the first call uploads the recording)
    got = [(f["frame_number"], f["extended"]) for f in frames if f["status"] == "ok"]
    src = source.IQarray(raw, RATE)
    src.read_device_raw(0, len(raw))
    runs = [run(src) for _ in range(a.reps)]
    assert all([f["start"] for f in r[1]] == [f["start"] for f in frames] for r in runs)
    info = obj.frameInfo
    stages = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    warm = float(np.median([r[2] for r in runs]))
    sps, w, _ = rs41.params(obj.audioRate)
    lst, m = rs41.candidates(obj.audio(), sps, w)
    kernel = kernel_us(obj.audio(), obj.audioRate, lst, m)
    bound = info["samples"] * 9.0 / HBM
    frame_bound = m * (8 * rs41.EXT * w * 8.0 + 2 * rs41.EXT) / HBM
    print(json.dumps({"stage": "decode_rs41", "samples": int(len(raw)), "seconds": tiles * BLOCK, "rate": RATE, "audio_rate": obj.audioRate,
                      "frames_sent": len(want), "frames": len(frames), "frames_match": got == want,
                      "corrected_bytes": int(sum(max(c, 0) for f in frames for c in f["corrected"])), "audio_samples": info["samples"],
                      "candidates": info["candidates"], "followed": info["followed"],
                      "first_ms": round(first * 1e3, 3), "first_stage_ms": {k: round(v * 1e3, 3) for k, v in obj.timings.items()},
                      "warm_ms": round(warm * 1e3, 3), "warm_stage_ms": stages,
                      "candidates_ns_per_audio_sample": round(stages["candidates"] * 1e6 / max(info["samples"], 1), 4),
                      "sync_kernel_us": kernel["sync"], "sync_kernel_memory_bound_us": round(bound * 1e6, 2),
                      "frame_kernel_us": kernel["frame"], "frame_kernel_memory_bound_us": round(frame_bound * 1e6, 3),
                      "frames_us_per_survivor": round(stages["frames"] * 1e3 / max(info["candidates"], 1), 4),
                      "device": _hip.device_name()}), flush=True)
    if got != want:
        raise SystemExit("decoded frames differ from those encoded")


if __name__ == "__main__":
    main()
