#!/usr/bin/env python3
"""
Side benchmark of POCSAG decoding (decode_pocsag): the time per stage -- the front end, the sync codeword
candidates at the three baud rates, the demodulation and correction of the survivors, the host's merge, chain and pages -- on a
synthesised recording at 2.4 MS/s: five seconds holding one transmission each at 512, 1200 and 2400 baud (the last inverted, two pages
each, carrier errors within +-500 Hz, amplitude 40, noise of sigma 6 per rail), tiled --duration / 5 times (60: a minute,
144 000 000 samples).  The pages decoded are checked against what was encoded.

The candidates stage and the candidate kernel alone (between two events, per baud rate) are printed beside the memory bound, one
float64 read and one mask byte written per audio sample and baud rate at 8 TB/s.  First call in the process and warm (median of --reps, a fresh decoder object each time over an IQarray whose pairs
stay resident on the device, a device synchronisation after every stage).  Nothing is gated on the numbers.  Prints one JSON line.
The library must have been built (python __graft_entry__.py).

    python tools/bench_pocsag.py [--reps 3] [--duration 60]
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
PAGES = ([(1234560, 0, "0800-555 [42]*U"), (1000007, 3, "The 512 baud page runs across the batch edge.")],
         [(77778, 1, "short"), (1000007, 3, "Alpha page of frame 7, on into batch two.")],
         [(424242, 3, "inverted"), (2097151, 0, "31337")])
BAUDS = (512, 1200, 2400)


def block(seed=43):
    """five seconds of recording with the three transmissions one behind the other"""
    from directdemod_amd import pocsag
    rng = np.random.default_rng(seed)
    pre = (64, 576, 576)                                              # (512 baud with a full preamble and two batches would not fit)
    starts, at = [], 5000.3
    for tx, baud, p in zip(PAGES, BAUDS, pre):
        starts.append(at)
        at += (p + pocsag.BATCH_BITS * len(pocsag.transmission_words(tx)) + 24) * RATE / float(baud)
    if at >= BLOCK * RATE:
        raise SystemExit("the transmissions do not fit %d seconds" % BLOCK)
    return pocsag.encode(list(PAGES), RATE, starts, BAUDS, (0, 0, 1), OFFSET, 40.0, 6.0, seed, rng.uniform(-500.0, 500.0, 3),
                         n=BLOCK * RATE, preamble=pre)


def kernel_us(audio, rate, reps=5):
    """per baud rate: k_pocsag_sync alone over the audio, with the memset of its masks (dd_debug_pocsag_masks between two events),
    the least of `reps` in microseconds"""
    import ctypes as C
    from directdemod_amd import _hip, pocsag
    L = _hip.lib()
    a, b = C.c_void_p(), C.c_void_p()
    _hip.check(L.dd_event_create(C.byref(a)), "dd_event_create")
    _hip.check(L.dd_event_create(C.byref(b)), "dd_event_create")
    mask = _hip.DevArray(audio.n, np.uint8)
    out = {}
    for baud in BAUDS:
        sps, w, slack, _ = pocsag.params(rate, baud)
        times = []
        for _ in range(reps + 1):                                     # (the first is a warm-up)
            L.dd_event_record(a, None)
            _hip.check(L.dd_debug_pocsag_masks(audio.ptr, audio.n, sps, w, slack, mask.ptr, None), "dd_debug_pocsag_masks")
            L.dd_event_record(b, None)
            ms = C.c_float(0.0)
            _hip.check(L.dd_event_elapsed_ms(a, b, C.byref(ms)), "dd_event_elapsed_ms")
            times.append(ms.value)
        out[baud] = round(min(times[1:]) * 1e3, 2)
    L.dd_event_destroy(a)
    L.dd_event_destroy(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=int, default=60)
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_pocsag, source
    _hip.require_gpu()
    tiles = max(1, a.duration // BLOCK)
    raw = np.tile(block(), (tiles, 1))
    want = [(baud, adr, fn, text) for tx, baud in zip(PAGES, BAUDS) for adr, fn, text in tx] * tiles

    def run(src):
        o = decode_pocsag.decode_pocsag(src, OFFSET)
        _hip.sync()
        t0 = time.perf_counter()
        pages = o.getPages
        return o, pages, time.perf_counter() - t0
    obj, pages, first = run(source.IQarray(raw, RATE))                # (the first call uploads the recording)
    got = [(p["baud"], p["address"], p["function"], p["text"]) for p in pages]
    src = source.IQarray(raw, RATE)
    src.read_device_raw(0, len(raw))
    runs = [run(src) for _ in range(a.reps)]
    assert all([p["bits"] for p in r[1]] == [p["bits"] for p in pages] for r in runs)
    info = obj.frameInfo
    stages = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    warm = float(np.median([r[2] for r in runs]))
    bound = len(BAUDS) * info["samples"] * 9.0 / HBM
    kernel = kernel_us(obj.audio(), obj.audioRate)
    print(json.dumps({"stage": "decode_pocsag", "samples": int(len(raw)), "seconds": tiles * BLOCK, "rate": RATE, "audio_rate": obj.audioRate,
                      "pages_sent": len(want), "pages": len(pages), "pages_match": got == want,
                      "corrected_bits": int(sum(p["corrected"] for p in pages)), "audio_samples": info["samples"],
                      "candidates": {b: v["candidates"] for b, v in info["bauds"].items()}, "batches": info["batches"],
                      "first_ms": round(first * 1e3, 3), "first_stage_ms": {k: round(v * 1e3, 3) for k, v in obj.timings.items()},
                      "warm_ms": round(warm * 1e3, 3), "warm_stage_ms": stages,
                      "candidates_ns_per_audio_sample_and_baud": round(stages["candidates"] * 1e6 / max(info["samples"] * len(BAUDS), 1), 4),
                      "candidates_memory_bound_ms": round(bound * 1e3, 4),
                      "candidates_over_bound": round(stages["candidates"] * 1e-3 / bound, 1) if bound else None,
                      "sync_kernel_us": kernel, "sync_kernel_memory_bound_us": round(bound / len(BAUDS) * 1e6, 2),
                      "batches_us_per_survivor": round(stages["batches"] * 1e3 / max(sum(v["candidates"] for v in info["bauds"].values()), 1), 4),
                      "device": _hip.device_name()}), flush=True)
    if got != want:
        raise SystemExit("decoded pages differ from those encoded")


if __name__ == "__main__":
    main()
