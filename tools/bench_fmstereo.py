#!/usr/bin/env python3
"""
Side benchmark of FM stereo decoding (decode_fmstereo): the time per stage -- the front end, the pilot
blocks, the carrier per block, the mixer and decimating FIR, the download -- on a synthesised recording at 2.4 MS/s: 5 seconds of a
station 100 kHz above the centre (1 kHz at 0.8 in the left channel, 3 kHz at 0.5 in the right, the pilot, amplitude 60, noise of
sigma 2 per rail), tiled --duration / 5 times (60: a minute, 144 000 000 samples).  The carrier's phase breaks where two tiles meet;
nothing is measured there.

Each kernel alone (between two events) is printed beside its memory bound at 8 TB/s: the pilot one float64 read per multiplex
sample; the audio kernel one float64 read per multiplex sample and one int32 pair written per D of them.  The audio kernel is timed
by both of its exact routes (dd_debug_fms_audio_route: sums in int64 and in float64).  The NumPy restatement (fmstereo.HostOps) runs
over the device's own multiplex, its outputs are compared with the device's bit for bit, and its seconds per stage are printed
beside the device's.  First call in the process and warm (median of --reps, a fresh decoder object each time over an IQarray whose
pairs stay resident on the device, a device synchronisation after every stage).  Nothing is gated on the times.  Prints one JSON
line.  The library must have been built (python __graft_entry__.py).

    python tools/bench_fmstereo.py [--reps 3] [--duration 60]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

RATE = 2400000
OFFSET = 100000.0
BLOCK_SAMPLES = 12000000                                              # 5 s
HBM = 8.0e12                                                          # bytes per second


def block(seed=47):
    from directdemod_amd import fmstereo as F
    return F.encode(F.tone(1000.0, 0.8, BLOCK_SAMPLES, RATE), F.tone(3000.0, 0.5, BLOCK_SAMPLES, RATE), RATE, offset=OFFSET, amplitude=60.0,
                    sigma=2.0, seed=seed)


def kernel_us(mpx, rate, gain, reps=5):
    """k_fms_pilot, k_fms_carrier and k_fms_audio by either route over the multiplex, each alone between two events, the least of
    `reps` in microseconds"""
    from directdemod_amd import _hip, fmstereo as F, rds
    L = _hip.lib()
    a, b = C.c_void_p(), C.c_void_p()
    _hip.check(L.dd_event_create(C.byref(a)), "dd_event_create")
    _hip.check(L.dd_event_create(C.byref(b)), "dd_event_create")
    D, step19, step38 = F.params(rate)
    h, d0 = F.taps(float(rate), 50e-6)
    P, nb = F.pilot(mpx, step19)
    _, u, _ = F.carrier(P, nb, F.threshold(0.03, rate))
    hd = _hip.DevArray.from_host(h)
    out = _hip.DevArray(2 * ((mpx.n + D - 1) // D) + 2, np.int32)
    S, lock = _hip.DevArray(max(2 * nb, 2), np.int32), _hip.DevArray(max(nb, 1), np.uint8)
    u2, P2 = _hip.DevArray(max(2 * nb, 2), np.int32), _hip.DevArray(max(2 * nb, 2), np.int32)
    t, G = rds.table_device().ptr, F.gain_word(gain)
    calls = {"pilot": lambda: L.dd_fms_pilot(mpx.ptr, mpx.n, step19, t, P2.ptr, None),
             "carrier": lambda: L.dd_fms_carrier(P.ptr, nb, F.threshold(0.03, rate), S.ptr, u2.ptr, lock.ptr, None),
             "audio_int64": lambda: L.dd_debug_fms_audio_route(mpx.ptr, mpx.n, step38, t, u.ptr, nb, G, hd.ptr, hd.n, D, d0, 0, out.ptr, None),
             "audio_float64": lambda: L.dd_debug_fms_audio_route(mpx.ptr, mpx.n, step38, t, u.ptr, nb, G, hd.ptr, hd.n, D, d0, 1, out.ptr, None),
             "audio": lambda: L.dd_fms_audio(mpx.ptr, mpx.n, step38, t, u.ptr, nb, G, hd.ptr, hd.n, D, d0, out.ptr, None)}
    res = {}
    for name, call in calls.items():
        times = []
        for _ in range(reps + 1):                                     # (the first is a warm-up)
            L.dd_event_record(a, None)
            _hip.check(call(), name)
            L.dd_event_record(b, None)
            ms = C.c_float(0.0)
            _hip.check(L.dd_event_elapsed_ms(a, b, C.byref(ms)), "dd_event_elapsed_ms")
            times.append(ms.value)
        res[name] = round(min(times[1:]) * 1e3, 2)
    L.dd_event_destroy(a)
    L.dd_event_destroy(b)
    return res, D, len(h)


def host_stages(mpx, rate, gain):
    """(the restatement's output, its seconds per stage) over a NumPy multiplex"""
    from directdemod_amd import fmstereo as F
    D, step19, step38 = F.params(rate)
    h, d0 = F.taps(float(rate), 50e-6)
    laps, t0 = {}, time.perf_counter()
    P = F.pilot_host(mpx, step19)
    laps["pilot"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    S, u, lock = F.carrier_host(P, F.threshold(0.03, rate))
    laps["carrier"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    out = F.audio_host(mpx, step38, u, F.gain_word(gain), h, D, d0)
    laps["audio"] = time.perf_counter() - t0
    return out, laps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=int, default=60)
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_fmstereo, source
    _hip.require_gpu()
    raw = np.tile(block(), (max(1, a.duration // 5), 1))

    def run(src):
        o = decode_fmstereo.decode_fmstereo(src, OFFSET)
        _hip.sync()
        t0 = time.perf_counter()
        out = o.getSamples
        return o, out, time.perf_counter() - t0
    obj, out, first = run(source.IQarray(raw, RATE))                  # (the first call uploads the recording)
    src = source.IQarray(raw, RATE)
    src.read_device_raw(0, len(raw))
    runs = [run(src) for _ in range(a.reps)]
    assert all(np.array_equal(r[1], out) for r in runs)
    stages = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    warm = float(np.median([r[2] for r in runs]))
    mpx, rate = obj.multiplex(), obj.multiplexRate
    kernel, D, ntaps = kernel_us(mpx, rate, obj.diffGain)
    host_out, host = host_stages(mpx.to_host(), rate, obj.diffGain)
    info = obj.pilotInfo
    bounds = {"pilot": 8.0 * mpx.n / HBM, "audio": (8.0 * mpx.n + 8.0 * len(out)) / HBM}
    print(json.dumps({"stage": "decode_fmstereo", "samples": int(len(raw)), "seconds": round(len(raw) / RATE, 3), "rate": RATE,
                      "multiplex_rate": rate, "multiplex_samples": mpx.n, "audio_rate": obj.audioRate, "audio_samples": int(len(out)),
                      "decimation": D, "taps": ntaps, "diff_gain": round(obj.diffGain, 6), "stereo": obj.stereo, "blocks": info["blocks"],
                      "locked": info["locked"], "pilot_level": round(info["level"], 5), "freq_error_hz": round(info["freqError"], 4),
                      "equals_restatement": bool(np.array_equal(host_out, out)),
                      "first_ms": round(first * 1e3, 3), "first_stage_ms": {k: round(v * 1e3, 3) for k, v in obj.timings.items()},
                      "warm_ms": round(warm * 1e3, 3), "warm_stage_ms": stages,
                      "restatement_stage_ms": {k: round(v * 1e3, 1) for k, v in host.items()},
                      "pilot_kernel_us": kernel["pilot"], "pilot_kernel_memory_bound_us": round(bounds["pilot"] * 1e6, 2),
                      "carrier_kernel_us": kernel["carrier"],
                      "audio_kernel_us": kernel["audio"], "audio_kernel_int64_us": kernel["audio_int64"],
                      "audio_kernel_float64_us": kernel["audio_float64"], "audio_kernel_memory_bound_us": round(bounds["audio"] * 1e6, 2),
                      "device": _hip.device_name()}), flush=True)
    if not np.array_equal(host_out, out):
        raise SystemExit("the device's audio differs from the restatement's")


if __name__ == "__main__":
    main()
