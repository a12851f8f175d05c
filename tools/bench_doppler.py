#!/usr/bin/env python3
"""
Side benchmark of the Doppler front end (frequency_shift.find_shift) over a 2^27-sample u8 IQ recording resident in HBM, tiled
from tests/_doppler.py's case (b): milliseconds per entry point (dd_waterfall_u8 = the FFT kernel and the row pass,
dd_band_argmax_f32; device events, median of --reps), the whole find_shift call on the host clock, each kernel's own bound,
and the time of a plain NumPy statement of the same sums on the host (measured on --cpu-windows windows, scaled).

dd_waterfall_u8 is timed as one interval (its two kernels run back to back inside the call), so its bounds cover both: on the
HBM side the raw bytes read once, the per-segment partial sums written by the FFT kernel and read by the row pass, and the rows
written, at the 8 TB/s peak; on the LDS side the FFT's traffic -- per window one 16 x window write on the way in (complex float64), a read and a
write of 16 x window per pass (six radix-4 passes and one radix-2 pass at 8192) and one read for the magnitudes -- at the LDS
rates with every CU streaming (reads 150 TB/s, writes 51 TB/s).  Both are computed, not measured; the line
gives both, names the larger and the share of it that the measured time reaches.  Prints one JSON line.

    python tools/bench_doppler.py [--reps 5] [--log2 27]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM_PEAK, LDS_READ, LDS_WRITE = 8.0e12, 150e12, 51e12


def host_sums(raw, window, row_len, every, n_windows):
    """make_fft's sums in NumPy over the first n_windows windows -> seconds"""
    flat = raw.reshape(-1)
    t0 = time.perf_counter()
    acc, rows = 0, []
    for w in range(n_windows):
        s = flat[w * 2 * window:(w + 1) * 2 * window].astype(np.int16)
        acc = acc + np.abs(np.fft.fft((s[0::2] - 127) + 1j * (s[1::2] - 127)))
        if (w + 1) % row_len == 0:
            rows.append(np.log(np.fft.fftshift(acc) / window / every))
            acc = 0
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2", type=int, default=27)
    ap.add_argument("--cpu-windows", type=int, default=512)
    a = ap.parse_args()
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    import _doppler
    from directdemod_amd import _hip, frequency_shift as fsh, source
    _hip.require_gpu()
    n = 1 << a.log2
    base = _doppler.case("b")
    raw = np.tile(base, (-(-n // base.shape[0]), 1))[:n]
    src = source.IQarray(raw, _doppler.FS)
    window = fsh.WINDOW
    every = (2 * n / (_doppler.FS * 2.0)) * 8192.0 / window
    args = (_doppler.FS, _doppler.CENTER, _doppler.CHANNEL, _doppler.BANDWIDTH)
    _, band_start, band_stop = fsh._band(*args)
    t0 = time.perf_counter()
    track = fsh.find_shift(src, *args)                                 # uploads the recording, loads the code
    first = time.perf_counter() - t0
    lib = _hip.lib()
    d = src.read_device_raw(0, n)
    rows = len(track)
    out = _hip.DevArray(rows * window, np.float32)
    idx = _hip.DevArray(rows, np.int32)
    ev = [C.c_void_p() for _ in range(3)]
    for e in ev:
        _hip.check(lib.dd_event_create(C.byref(e)), "event")
    t_wf, t_am, t_all = [], [], []
    got = C.c_int64(0)
    for _ in range(a.reps):
        lib.dd_event_record(ev[0], None)
        _hip.check(lib.dd_waterfall_u8(d.ptr, 2 * n, window, every, out.ptr, rows, C.byref(got), None), "dd_waterfall_u8")
        lib.dd_event_record(ev[1], None)
        _hip.check(lib.dd_band_argmax_f32(out.ptr, rows, window, band_start, band_stop, idx.ptr, None), "dd_band_argmax_f32")
        lib.dd_event_record(ev[2], None)
        ms = C.c_float(0)
        _hip.check(lib.dd_event_elapsed_ms(ev[0], ev[1], C.byref(ms)), "elapsed")
        t_wf.append(ms.value)
        _hip.check(lib.dd_event_elapsed_ms(ev[1], ev[2], C.byref(ms)), "elapsed")
        t_am.append(ms.value)
        t0 = time.perf_counter()
        again = fsh.find_shift(src, *args)
        t_all.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(again, track)
    for e in ev:
        lib.dd_event_destroy(e)
    n_win = n // window
    row_len = int(np.ceil(every))
    passes = (window.bit_length() - 1 + 1) // 2
    lds_r = n_win * 16 * window * (passes + 1)
    lds_w = n_win * 16 * window * (passes + 1)
    nseg = min(16, -(-row_len // 8))                                   # DD_WF_SEG_WINDOWS, DD_WF_MAX_SEGS
    hbm_bytes = 2 * n + 2 * rows * nseg * window * 4 + rows * window * 4
    hbm_ms = hbm_bytes / HBM_PEAK * 1e3
    lds_ms = (lds_r / LDS_READ + lds_w / LDS_WRITE) * 1e3
    cpu_w = min(a.cpu_windows // row_len * row_len, n_win) or row_len
    cpu_s = host_sums(raw, window, row_len, every, cpu_w) * n_win / cpu_w
    wf = float(np.median(t_wf))
    print(json.dumps({"stage": "frequency_shift.find_shift", "samples": n, "windows": n_win, "rows": rows, "row_len": row_len,
                      "first_ms": round(first * 1e3, 3), "find_shift_ms": round(float(np.median(t_all)), 3),
                      "waterfall_ms": round(wf, 4), "band_argmax_ms": round(float(np.median(t_am)), 4),
                      "waterfall_bound_hbm_ms": round(hbm_ms, 4), "waterfall_bound_lds_ms": round(lds_ms, 4),
                      "waterfall_larger_bound": "lds" if lds_ms > hbm_ms else "hbm",
                      "waterfall_of_larger_bound": round(max(hbm_ms, lds_ms) / wf, 4),
                      "band_argmax_bound_ms": round(rows * (band_stop - band_start) * 4 / HBM_PEAK * 1e3, 6),
                      "cpu_numpy_ms": round(cpu_s * 1e3, 1), "cpu_windows_measured": cpu_w,
                      "speedup_vs_numpy": round(cpu_s * 1e3 / float(np.median(t_all)), 1), "device": _hip.device_name()}), flush=True)


if __name__ == "__main__":
    main()
