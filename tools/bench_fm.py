#!/usr/bin/env python3
"""
Side benchmark of decode_fm.getAudio and of the three signal classes beside it, each against the same statement in SciPy / NumPy on
the host.  Prints one JSON line per stage.

  fm.getAudio            a resident 2^27-sample u8 IQ recording in decode_fm's own shape (2.048 MS/s, /68, audio at 15 kHz, chunks of
                         constants.PROC_CHUNKSIZE), tiled from tests/_fm.py's case a: first call in the process (upload included) and
                         warm (median of --reps, a fresh decoder each time).  Host: the reference's chain restated with NumPy / SciPy
                         (exp mixer, lfilter, slice, angle, scipy.signal.resample) over the first --host-samples samples, reported per
                         sample -- the whole recording would take the host minutes.
  medianFilter(5 / 255)  2^22 float64 samples on the device (device in, device out) against scipy.signal.medfilt
  blackmanHarrisConv     151 taps over 2^22 complex samples against scipy.signal.convolve(mode='same')

    python tools/bench_fm.py [--reps 5] [--log2 27] [--host-samples 4194304] [--no-build] [--no-host]
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


def timed(fn, reps, sync):
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts))


def host_fm_chain(x, fs, offset, bw, audio):
    """decode_fm.py:61-70 for one chunk with NumPy / SciPy (history of ones: lfilter_zi(b, [1]) unscaled, filters.py:45)"""
    import scipy.signal as ss
    w = ss.windows.blackmanharris(151)
    y = x * np.exp(-2.0j * np.pi * offset * np.arange(len(x)) / fs)
    y, _ = ss.lfilter(w, [1.0], y, zi=ss.lfilter_zi(w, [1.0]))
    m = int(fs / bw)
    y = y[::m]
    a = np.angle(y[1:] * np.conj(y[:-1]))
    return ss.resample(a, int(audio * len(a) / int(fs / m)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2", type=int, default=27, help="samples of the getAudio recording, as a power of two")
    ap.add_argument("--host-samples", type=int, default=1 << 22)
    ap.add_argument("--no-build", action="store_true", help="use the library as it stands")
    ap.add_argument("--no-host", action="store_true", help="skip the SciPy runs")
    a = ap.parse_args()
    if not a.no_build:
        import __graft_entry__ as ge
        ge.build()
    import scipy.signal as ss
    import _fm
    from directdemod_amd import _hip, decode_fm, filters, source
    _hip.require_gpu()
    dev = _hip.device_name()

    # ---- getAudio
    base = _fm.case("a")
    fs, offset, _, _ = _fm.told("a")
    n = 1 << a.log2
    raw = np.tile(base, (-(-n // base.shape[0]), 1))[:n]
    src = source.IQarray(raw, fs)
    t0 = time.perf_counter()
    first_obj = decode_fm.decode_fm(src, offset)
    ref = first_obj.getAudio.signal
    first = time.perf_counter() - t0
    launches = first_obj._launch_count()

    def run():
        o = decode_fm.decode_fm(src, offset)
        o.getAudio.device_signal
    warm, best = timed(run, a.reps, _hip.sync)
    assert np.array_equal(decode_fm.decode_fm(src, offset).getAudio.signal, ref)
    line = {"stage": "fm.getAudio", "samples": n, "audio_samples": len(ref), "fused_launches": launches, "first_ms": round(first * 1e3, 3),
            "warm_ms": round(warm * 1e3, 3), "warm_min_ms": round(best * 1e3, 3), "gsamples_per_s": round(n / warm / 1e9, 3), "device": dev}
    if not a.no_host:
        hn = min(a.host_samples, n)
        x = src.read(0, hn)
        t0 = time.perf_counter()
        host_fm_chain(x, fs, offset, 30000, 15000)
        th = time.perf_counter() - t0
        line.update({"host_samples": hn, "host_ms": round(th * 1e3, 1), "host_msamples_per_s": round(hn / th / 1e6, 2),
                     "speedup_per_sample": round((n / warm) / (hn / th), 1)})
    print(json.dumps(line), flush=True)
    del raw, src, first_obj

    # ---- the classes
    rng = np.random.Generator(np.random.PCG64(1))
    m = 1 << 22
    xr = rng.standard_normal(m)
    xc = (rng.standard_normal(m) + 1j * rng.standard_normal(m)).astype(np.complex64)
    dr, dc = _hip.DevArray.from_host(xr), _hip.DevArray.from_host(xc)
    jobs = [("medianFilter(5)", filters.medianFilter(5), dr, lambda: ss.medfilt(xr, 5)),
            ("medianFilter(255)", filters.medianFilter(255), dr, lambda: ss.medfilt(xr, 255)),
            ("blackmanHarrisConv(151)", filters.blackmanHarrisConv(151), dc,
             lambda: ss.convolve(xc, ss.windows.blackmanharris(151), mode="same"))]
    for name, flt, d, host in jobs:
        flt.applyOn(d)
        warm, best = timed(lambda: flt.applyOn(d), a.reps, _hip.sync)
        line = {"stage": name, "samples": m, "dtype": str(d.dtype), "warm_ms": round(warm * 1e3, 3), "warm_min_ms": round(best * 1e3, 3),
                "msamples_per_s": round(m / warm / 1e6, 1), "device": dev}
        if not a.no_host:
            t0 = time.perf_counter()
            host()
            th = time.perf_counter() - t0
            line.update({"host_ms": round(th * 1e3, 1), "speedup": round(th / warm, 1)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
