#!/usr/bin/env python3
"""
Side benchmark of Funcube sync detection (decode_funcube.getSyncs): first call in the process and warm (median of --reps, a fresh
decoder object each time) on a 2.048 MS/s u8 IQ recording tiled from tests/_funcube.py's case (b) synthesis (the signal 30 kHz
above the centre), with the time per stage of the warm runs (mixer, low-pass, walk, lim, MINSYNC, MAXSYNC).  Prints one JSON line.

    python tools/bench_funcube.py [--reps 3] [--duration 60] [--no-build]

With --frames N: the telemetry frame decoder (decode_funcube.getFrames) on a recording of N frames built by
tests/_funcube_frames.py's definitions: the fc_* stage times beside the others, and the sync search alone on the recording's bit
metric tiled to --search-symbols entries against the NumPy restatement on the same array.

    python tools/bench_funcube.py --frames 4 [--search-symbols 7200000] [--reps 3] [--no-build]
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


def recording(dur):
    import _funcube
    base, off, _ = _funcube.case("b")
    return np.tile(base, (int(np.ceil(dur * _funcube.FS / base.shape[0])), 1))[:int(dur * _funcube.FS)], _funcube.FS, off


def frames_recording(nframes, seed=41, gap_bits=40, lead_bits=100):
    """-> (uint8[n, 2] IQ pairs, the frames' payloads): `nframes` telemetry frames (funcube_fec.encode_frame) `gap_bits` random bits
    apart, differentially encoded, as 1200 bit/s BPSK on a 300 Hz carrier (amplitude 60, sigma 4), synthesised block by block"""
    import _funcube
    import _funcube_frames as F
    from directdemod_amd import funcube_fec as fec
    g = F.rng(seed)
    data = [F.payload(seed + 1 + i) for i in range(nframes)]
    parts = [g.integers(0, 2, lead_bits).astype(np.uint8)]
    for d in data:
        parts += [fec.encode_frame(d), g.integers(0, 2, gap_bits).astype(np.uint8)]
    lev = fec.differential(np.concatenate(parts))
    n = len(lev) * 5120 // 3
    raw = np.empty((n, 2), dtype=np.uint8)
    for a in range(0, n, 1 << 21):
        t = np.arange(a, min(a + (1 << 21), n), dtype=np.int64)
        x = 60.0 * (2.0 * lev[t * 3 // 5120] - 1.0) * np.exp(2.0j * np.pi * 300.0 * t / _funcube.FS)
        x += 4.0 * (g.standard_normal(len(t)) + 1j * g.standard_normal(len(t)))
        raw[a:a + len(t)] = np.clip(np.rint(np.stack((x.real, x.imag), axis=1) + 127.5), 0, 255)
    return raw, np.stack(data)


def frames_case(a):
    """decode_funcube.getFrames on a recording of --frames frames: the fc_* stage times (warm, median of --reps), and the sync
    search alone on the recording's D tiled to --search-symbols entries beside funcube_fec.sync_candidates_np on the same array"""
    import _funcube
    from directdemod_amd import _hip, decode_funcube, source
    from directdemod_amd import funcube_fec as fec
    _hip.require_gpu()
    raw, data = frames_recording(a.frames)
    src = source.IQarray(raw, _funcube.FS)
    stages, found = [], None
    for _ in range(a.reps + 1):                                   # the first pass is the process's first call: not counted
        o = decode_funcube.decode_funcube(src, 0, None, _funcube.CENTER, _funcube.CHANNEL)
        syncs = o.getSyncs
        found, info = o.getFrames, o.frameInfo
        stages.append(dict(o.timings))
    st = {k: round(float(np.median([s[k] for s in stages[1:]])) * 1e3, 3) for k in stages[0]}
    D = fec.soft_bits(o.walker().view("sym")).to_host()
    long_d = np.tile(D, -(-a.search_symbols // max(len(D), 1)))[:a.search_symbols]
    dev = _hip.DevArray.from_host(long_d)
    took = []
    for _ in range(a.reps + 1):
        _hip.sync()
        t0 = time.perf_counter()
        got = fec.sync_candidates(dev)
        took.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = fec.sync_candidates_np(long_d)
    host = time.perf_counter() - t0
    assert np.array_equal(got, want)
    search = float(np.median(took[1:]))
    print(json.dumps({"stage": "funcube.getFrames", "frames_sent": a.frames, "samples": int(raw.shape[0]), "symbols": o.walker().nsym,
                      "frames_found": len(found), "frames_ok": int(info["ok"].sum()),
                      "frames_equal_sent": int(sum(any(np.array_equal(f, d) for d in data) for f in found)),
                      "syncs": len(syncs), "warm_stage_ms": st, "search_entries": int(len(long_d)), "search_candidates": len(got),
                      "search_ms": round(search * 1e3, 3), "search_np_ms": round(host * 1e3, 1),
                      "search_np_over_device": round(host / search, 1), "device": _hip.device_name()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=float, default=60.0)
    ap.add_argument("--no-build", action="store_true", help="use the library as it stands")
    ap.add_argument("--frames", type=int, default=0, help="the frame decoder's case: a recording of this many telemetry frames")
    ap.add_argument("--search-symbols", type=int, default=7200000, help="entries of D for the sync search alone (ten minutes)")
    a = ap.parse_args()
    if not a.no_build:
        import __graft_entry__ as ge
        ge.build()
    if a.frames:
        frames_case(a)
        return
    import _funcube
    from directdemod_amd import _hip, decode_funcube, source
    _hip.require_gpu()
    raw, fs, offset = recording(a.duration)
    src = source.IQarray(raw, fs)

    def decoder():
        return decode_funcube.decode_funcube(src, offset, None, _funcube.CENTER, _funcube.CHANNEL)
    t0 = time.perf_counter()
    obj = decoder()
    syncs = obj.getSyncs
    first = time.perf_counter() - t0
    nsym = obj.walker().nsym
    warm, stages = [], []
    for _ in range(a.reps):
        o = decoder()
        _hip.sync()
        t0 = time.perf_counter()
        assert o.getSyncs == syncs
        warm.append(time.perf_counter() - t0)
        stages.append(o.timings)
    st = {k: round(float(np.median([s[k] for s in stages])) * 1e3, 3) for k in stages[0]}
    wm = float(np.median(warm))
    print(json.dumps({"stage": "funcube.getSyncs", "duration_s": a.duration, "samples": int(raw.shape[0]), "symbols": nsym,
                      "minsyncs": len(o.minsyncs), "maxsyncs": len(o.argmax), "syncs": len(syncs), "useful": o.useful,
                      "first_ms": round(first * 1e3, 3), "warm_ms": round(wm * 1e3, 3), "warm_min_ms": round(min(warm) * 1e3, 3),
                      "us_per_symbol": round(wm * 1e6 / max(nsym, 1), 4), "warm_stage_ms": st, "device": _hip.device_name()}),
          flush=True)


if __name__ == "__main__":
    main()
