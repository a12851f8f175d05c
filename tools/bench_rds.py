#!/usr/bin/env python3
"""
Side benchmark of RDS decoding (decode_rds): the time per stage -- the front end, the 57 kHz baseband, the
group candidates, the decoding and repair of the survivors, the host's merge, chains, follow and parse -- on a synthesised
recording at 2.4 MS/s: 4.992 seconds holding 56 groups of one station (its name, a radiotext and the clock; 100 kHz above the
centre, amplitude 60, noise of sigma 6 per rail, a 1 kHz tone and the pilot in the multiplex), tiled --duration / 5 times (60: a
minute, 672 groups, 143 769 600 samples).  The carrier's phase and the symbol shaping break where two tiles meet, so a group there
may be lost; the groups decoded word for word as sent are counted, and fewer than nine in ten fail the run.

Each kernel alone (between two events) is printed beside its memory bound at 8 TB/s: the baseband one float64 read per multiplex
sample and one int32 pair written per D of them; the candidates one int32 pair read and one mask byte written per baseband sample;
the groups the 2 h pairs around each of a survivor's 105 bit boundaries read once and 40 bytes written.  First call in the process
and warm (median of --reps, a fresh decoder object each time over an IQarray whose pairs stay resident on the device, a device
synchronisation after every stage).  Nothing is gated on the times.  Prints one JSON line.  The library must have been built
(python __graft_entry__.py).

    python tools/bench_rds.py [--reps 3] [--duration 60]
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
OFFSET = 100000.0
GROUPS = 56
BLOCK_SAMPLES = 11980800                                              # 57 groups' time, 4.992 s: a whole number of samples
HBM = 8.0e12                                                          # bytes per second
PI, PS, TEXT = 0xD318, "RADIO 1 ", "Synthesised RDS, every group on its own.\r"


def groups():
    from directdemod_amd import rds
    out = []
    for k in range(GROUPS):
        if k % 4 == 3 and k // 4 < 11:
            out.append(rds.group_2a(PI, TEXT, k // 4))
        elif k == 55:
            out.append(rds.group_4a(PI, 60000, 13, 37, 2))
        else:
            out.append(rds.group_0a(PI, PS, k % 4, pty=10, af=(224 + 2, 10) if k == 0 else (20, 205)))
    return out


def block(seed=43):
    from directdemod_amd import rds
    return rds.encode(groups(), RATE, offset=OFFSET, amplitude=60.0, sigma=6.0, seed=seed, start=0.004, n=BLOCK_SAMPLES)


def kernel_us(mpx, rate, reps=5):
    """(k_rds_baseband over the multiplex, k_rds_sync over the baseband, k_rds_groups over the survivors), each alone between two
    events, the least of `reps` in microseconds; and the survivors' count"""
    import ctypes as C
    from directdemod_amd import _hip, rds
    L = _hip.lib()
    a, b = C.c_void_p(), C.c_void_p()
    _hip.check(L.dd_event_create(C.byref(a)), "dd_event_create")
    _hip.check(L.dd_event_create(C.byref(b)), "dd_event_create")
    d, sps, step = rds.params(rate)
    base = rds.baseband(mpx, d, step)
    m = base.n // 2
    lst, count = rds.candidates(base, m, sps, 3)
    out32 = _hip.DevArray(max(base.n, 2), np.int32)
    mask = _hip.DevArray(max(m, 1), np.uint8)
    words, meta = _hip.DevArray(4 * max(count, 1), np.uint16), _hip.DevArray(8 * max(count, 1), np.int32)
    calls = {"baseband": lambda: L.dd_rds_baseband(mpx.ptr, mpx.n, d, 0, step, rds.table_device().ptr, out32.ptr, None),
             "sync": lambda: L.dd_debug_rds_masks(base.ptr, m, sps, 3, mask.ptr, None),
             "groups": lambda: L.dd_rds_groups(base.ptr, m, sps, 2, lst.ptr, count, words.ptr, meta.ptr, None)}
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
    return out, count, d, sps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=int, default=60)
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_rds, source
    _hip.require_gpu()
    tiles = max(1, a.duration // 5)
    raw = np.tile(block(), (tiles, 1))
    want = groups() * tiles

    def run(src):
        o = decode_rds.decode_rds(src, OFFSET)
        _hip.sync()
        t0 = time.perf_counter()
        found = o.getGroups
        return o, found, time.perf_counter() - t0
    obj, found, first = run(source.IQarray(raw, RATE))                # (the first call uploads the recording)
    left, kept = {}, 0
    for w in want:
        left[w] = left.get(w, 0) + 1
    for g in found:
        w = tuple(g["words"])
        if left.get(w, 0) > 0:
            left[w] -= 1
            kept += 1
    src = source.IQarray(raw, RATE)
    src.read_device_raw(0, len(raw))
    runs = [run(src) for _ in range(a.reps)]
    assert all([g["start"] for g in r[1]] == [g["start"] for g in found] for r in runs)
    info = obj.frameInfo
    stages = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    warm = float(np.median([r[2] for r in runs]))
    kernel, count, d, sps = kernel_us(obj.audio(), obj.audioRate)
    n_mpx = obj.audio().n
    h = int(sps // 2)
    bounds = {"baseband": (8.0 * n_mpx + 8.0 * (n_mpx // d)) / HBM, "sync": 9.0 * info["samples"] / HBM,
              "groups": count * (105 * 2 * h * 8.0 + 40.0) / HBM}
    st = obj.getStations.get(PI, {})
    print(json.dumps({"stage": "decode_rds", "samples": int(len(raw)), "seconds": round(len(raw) / RATE, 3), "rate": RATE,
                      "multiplex_rate": obj.audioRate, "multiplex_samples": n_mpx, "baseband_samples": info["samples"],
                      "groups_sent": len(want), "groups": len(found), "groups_as_sent": kept, "candidates": info["candidates"],
                      "followed": info["followed"], "repaired_groups": info["repaired"], "ps": st.get("ps"), "clock": st.get("clock"),
                      "first_ms": round(first * 1e3, 3), "first_stage_ms": {k: round(v * 1e3, 3) for k, v in obj.timings.items()},
                      "warm_ms": round(warm * 1e3, 3), "warm_stage_ms": stages,
                      "baseband_kernel_us": kernel["baseband"], "baseband_kernel_memory_bound_us": round(bounds["baseband"] * 1e6, 2),
                      "sync_kernel_us": kernel["sync"], "sync_kernel_memory_bound_us": round(bounds["sync"] * 1e6, 2),
                      "groups_kernel_us": kernel["groups"], "groups_kernel_memory_bound_us": round(bounds["groups"] * 1e6, 3),
                      "device": _hip.device_name()}), flush=True)
    if kept * 10 < len(want) * 9:
        raise SystemExit("fewer than nine in ten of the groups encoded were decoded")


if __name__ == "__main__":
    main()
