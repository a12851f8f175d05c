#!/usr/bin/env python3
"""
Side benchmark of ACARS decoding (decode_acars): the time per stage -- the front end of three channels, the
template candidates, the demodulation and repair of the survivors, the host's merge and parse -- on a synthesised recording at
2.4 MS/s: five seconds holding four blocks on each of three channels 25 kHz apart (a block without text, a downlink of two blocks
joined by ETB and a block of 220 characters, the middle channel inverted; AM of depth 0.8, amplitude 20 -- the three carriers at
once stay inside the u8 range --, noise of sigma 3 per rail),
tiled --duration / 5 times (60: a minute, 144 000 000 samples).  The blocks decoded are checked against what was encoded.

The candidates stage and the candidate kernel alone (between two events) are printed beside the memory bound, one float64 read
and one mask byte written per audio sample and channel at 8 TB/s.  First call in the process and warm (median of --reps, a fresh
decoder object each time over an IQarray whose pairs stay resident on the device, a device synchronisation after every stage).
Nothing is gated on the numbers.  Prints one JSON line.  The library must have been built (python __graft_entry__.py).

    python tools/bench_acars.py [--reps 3] [--duration 60]
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
OFFSETS = (-25000.0, 0.0, 25000.0)                                    # 131.525 / 131.550 / 131.575 MHz around 131.550
BLOCK = 5                                                             # seconds synthesised
HBM = 8.0e12                                                          # bytes per second
LONG = "".join(chr(33 + (11 * i) % 90) for i in range(220))


def channel_blocks(ch):
    from directdemod_amd import acars
    reg = ("G-EUPJ", "N123AB", "OH-LVA")[ch]
    return [acars.block_bytes("2", reg, None, "Q0", str(ch)),
            acars.block_bytes("2", reg, None, "10", str(3 + ch), "M1%dABA0123POS N51289W000271," % ch, more=True),
            acars.block_bytes("2", reg, None, "10", str(4 + ch), "M1%dBBA01231542,350,ETA 1630" % ch),
            acars.block_bytes("E", reg, "A", "H1", str(6 + ch), LONG)]


def block(seed=47):
    """five seconds of recording: per channel the four blocks one behind the other, the channels at once"""
    from directdemod_amd import acars
    blks, starts, offs, pols = [], [], [], []
    for ch, off in enumerate(OFFSETS):
        at = 20000.3 + 100000.7 * ch
        for b in channel_blocks(ch):
            blks.append(b)
            starts.append(at)
            offs.append(off)
            pols.append(int(ch == 1))
            at += (8 * (acars.PREKEY + 5 + len(b)) + 400) * RATE / float(acars.BAUD)
        if at >= BLOCK * RATE:
            raise SystemExit("the blocks do not fit %d seconds" % BLOCK)
    return acars.encode(blks, RATE, starts, offs, 0.8, 20.0, 3.0, seed, polarity=pols, n=BLOCK * RATE)


def kernel_us(audio, rate, reps=5):
    """k_acars_sync alone over one channel's audio, with the memset of its masks (dd_debug_acars_masks between two events), the
    least of `reps` in microseconds"""
    import ctypes as C
    from directdemod_amd import _hip, acars
    L = _hip.lib()
    a, b = C.c_void_p(), C.c_void_p()
    _hip.check(L.dd_event_create(C.byref(a)), "dd_event_create")
    _hip.check(L.dd_event_create(C.byref(b)), "dd_event_create")
    mask = _hip.DevArray(audio.n, np.uint8)
    sps, w, slack, _ = acars.params(rate)
    times = []
    for _ in range(reps + 1):                                         # (the first is a warm-up)
        L.dd_event_record(a, None)
        _hip.check(L.dd_debug_acars_masks(audio.ptr, audio.n, sps, w, slack, mask.ptr, None), "dd_debug_acars_masks")
        L.dd_event_record(b, None)
        ms = C.c_float(0.0)
        _hip.check(L.dd_event_elapsed_ms(a, b, C.byref(ms)), "dd_event_elapsed_ms")
        times.append(ms.value)
    L.dd_event_destroy(a)
    L.dd_event_destroy(b)
    return round(min(times[1:]) * 1e3, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=int, default=60)
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_acars, source
    _hip.require_gpu()
    tiles = max(1, a.duration // BLOCK)
    raw = np.tile(block(), (tiles, 1))
    want = sorted(("ABC"[ch], b[:-1]) for ch in range(len(OFFSETS)) for b in channel_blocks(ch)) * tiles

    def run(src):
        o = decode_acars.decode_acars(src, OFFSETS)
        _hip.sync()
        t0 = time.perf_counter()
        found = o.getBlocks
        return o, found, time.perf_counter() - t0
    obj, found, first = run(source.IQarray(raw, RATE))                # (the first call uploads the recording)
    got = sorted((b["channel"], b["bytes"]) for b in found)
    src = source.IQarray(raw, RATE)
    src.read_device_raw(0, len(raw))
    runs = [run(src) for _ in range(a.reps)]
    assert all([b["bytes"] for b in r[1]] == [b["bytes"] for b in found] for r in runs)
    info = obj.frameInfo
    per = info["channels"]
    stages = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    warm = float(np.median([r[2] for r in runs]))
    bound = len(OFFSETS) * info["samples"] * 9.0 / HBM
    kernel = kernel_us(obj.audio()[0], obj.audioRate)
    cands = sum(v["candidates"] for v in per.values())
    print(json.dumps({"stage": "decode_acars", "samples": int(len(raw)), "seconds": tiles * BLOCK, "rate": RATE, "audio_rate": obj.audioRate,
                      "channels": len(OFFSETS), "blocks_sent": len(want), "blocks": len(found), "blocks_match": got == sorted(want),
                      "messages": len(obj.getMessages), "corrected_bits": int(sum(b["corrected"] for b in found)),
                      "audio_samples": info["samples"], "candidates": {ch: v["candidates"] for ch, v in per.items()},
                      "first_ms": round(first * 1e3, 3), "first_stage_ms": {k: round(v * 1e3, 3) for k, v in obj.timings.items()},
                      "warm_ms": round(warm * 1e3, 3), "warm_stage_ms": stages,
                      "candidates_ns_per_audio_sample_and_channel": round(stages["candidates"] * 1e6 / max(info["samples"] * len(OFFSETS), 1), 4),
                      "candidates_memory_bound_ms": round(bound * 1e3, 4),
                      "candidates_over_bound": round(stages["candidates"] * 1e-3 / bound, 1) if bound else None,
                      "sync_kernel_us": kernel, "sync_kernel_memory_bound_us": round(bound / len(OFFSETS) * 1e6, 2),
                      "blocks_us_per_survivor": round(stages["blocks"] * 1e3 / max(cands, 1), 4),
                      "device": _hip.device_name()}), flush=True)
    if got != sorted(want):
        raise SystemExit("decoded blocks differ from those encoded")


if __name__ == "__main__":
    main()
