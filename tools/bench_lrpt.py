#!/usr/bin/env python3
"""
Side benchmark of Meteor-M2 LRPT decoding (decode_meteorm2.getFrames, getPackets): the time per stage of the frame decoder (lrpt_soft,
lrpt_asm, lrpt_viterbi, lrpt_finish), of Reed-Solomon correction (lrpt_rs) and of packet reassembly (lrpt_packets) beside the stages of
the decode pass they start from (front end, walk, lim, MINSYNC, MAXSYNC), on a 2.048 MS/s u8 IQ recording tiled from tests/_lrpt.py's
case (a) (random bodies: no codeword is decodable, the Reed-Solomon stage's longest way) or tests/_rs.py's case (b) (real frames and
packets, two fades per tile).  Frames break at the tile seams; the decoder simply finds the whole ones.  First call in the process and
warm (median of --reps, a fresh decoder object each time).  Prints one JSON line.  The library must have been built
(python __graft_entry__.py).

A tiled case (b) repeats its frames' counters: each tile delivers the same packets again, and whatever packet is under way at a seam
is dropped there, by the counter's jump back or by the broken frame.  "packets" counts them all, "packets_distinct" the different ones.

--case c is the image layer (decode_meteorm2.getImage).  First dd_lrpt_jpeg alone, 4096 packets per call --
flat strips, noise strips at q = 80, random bytes of 1..300 -- between device events, the median of 20 calls after 3 (the entry
uploads its 3 n + 1 descriptor words and waits for the kernel, so the figure is the upload and the kernel; --kernel-only stops
there, for a kernel trace taken in a run of its own), beside the NumPy restatement's time for the same packets on the host.  Then
the stages of getImage on tests/_jpeg.py's case (c) tiled: a tile's sequence counts repeat, so from the second tile on the packets
are decoded (mcus) and mostly not placed.

--case d is the soft-symbol entry in the Meteor-M N2-x modes (decode_lrpt): a differential stream through
the (36, 2048) interleaver with its markers, --duration seconds at 80 ksym/s, built by tests/_lrpt_modes.py from 16 seeded frame
bodies tiled to the length (the frames are tiled, not the symbols: the interleaver spreads every bit over 1.43 M symbols, so a
stream tiled from a short one would hold no whole frame).  Timed with a device synchronisation after each stage: the marker
scores and the lock (lrpt_deint_scores), the gather (lrpt_deinterleave), and the frame stages behind it with the NRZ-M template
and finish (lrpt_asm, lrpt_viterbi, lrpt_finish).

    python tools/bench_lrpt.py [--reps 3] [--duration 60] [--case a|b|c|d] [--kernel-only]
"""
import ctypes as C
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def recording(dur, case="a"):
    import _lrpt
    import _rs
    if case == "c":
        import _jpeg
        base = _jpeg.case("c")[0]
    else:
        base = (_lrpt if case == "a" else _rs).case(case)[0]
    n = int(dur * _lrpt.FS)
    return np.tile(base, (-(-n // base.shape[0]), 1))[:n], _lrpt.FS


def jpeg_kernel(npackets=4096, calls=20, warm=3):
    """dd_lrpt_jpeg over npackets packets of three kinds -> {kind: {...}}: the entry between events, the restatement on the host"""
    import _jpeg
    from directdemod_amd import _hip, lrpt
    rng = np.random.Generator(np.random.PCG64(41))
    lib = _hip.lib()

    def flat():
        w, pred = _jpeg.Writer(), 0
        for v in rng.integers(-60, 60, 14):
            w.dc(int(v) - pred).eob()
            pred = int(v)
        return w.bytes()
    kinds = {
        "flat": (lambda: flat(), 80),
        "noise_q80": (lambda: _jpeg.encode_strip(np.clip(128 + 40 * rng.standard_normal((8, 112)), 0, 255).astype(np.uint8), 80)[0], 80),
        "random": (lambda: rng.integers(0, 256, int(rng.integers(1, 301)), dtype=np.uint8).tobytes(), 80),
    }
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        _hip.check(lib.dd_event_create(C.byref(e)), "event")
    out = {}
    for kind, (make, q) in kinds.items():
        distinct = [make() for _ in range(256)]
        payloads = [distinct[i % 256] for i in range(npackets)]
        t0 = time.perf_counter()
        want = np.zeros(256, dtype=np.int32)
        for i, p in enumerate(distinct):
            coef, want[i] = lrpt.jpeg_blocks_np(p)
            lrpt.idct_np(coef[:want[i]], lrpt.quantiser(q))
        host_ms = (time.perf_counter() - t0) * 1e3 * npackets / 256                    # 256 different packets, each npackets / 256 times
        offsets = np.concatenate(([0], np.cumsum([len(p) for p in payloads]))).astype(np.int64)
        data = _hip.DevArray.from_host(np.frombuffer(b"".join(payloads), dtype=np.uint8))
        qs = np.full(npackets, q, dtype=np.uint8)
        dst = (896 * np.arange(npackets)).astype(np.int64)
        pix = _hip.DevArray(896 * npackets, np.uint8)
        mcus = _hip.DevArray(npackets, np.int32)
        ms, times = C.c_float(0), []
        for i in range(warm + calls):
            lib.dd_event_record(ev[0], None)
            _hip.check(lib.dd_lrpt_jpeg(data.ptr, offsets.ctypes.data, qs.ctypes.data, dst.ctypes.data, npackets, 112, pix.ptr, mcus.ptr, None),
                       "dd_lrpt_jpeg")
            lib.dd_event_record(ev[1], None)
            _hip.check(lib.dd_event_sync(ev[1]), "event sync")
            _hip.check(lib.dd_event_elapsed_ms(ev[0], ev[1], C.byref(ms)), "elapsed")
            if i >= warm:
                times.append(ms.value)
        assert np.array_equal(mcus.to_host(), np.tile(want, npackets // 256))
        out[kind] = {"packets": npackets, "bytes": int(offsets[-1]), "blocks": int(want.sum()) * (npackets // 256),
                     "entry_us_median": round(float(np.median(times)) * 1e3, 1), "entry_us_min": round(float(np.min(times)) * 1e3, 1),
                     "restatement_host_ms": round(host_ms, 1)}
    for e in ev:
        lib.dd_event_destroy(e)
    return out


def main_image(a):
    from directdemod_amd import _hip, decode_meteorm2, lrpt, source
    _hip.require_gpu()
    res = {"stage": "meteorm2.getImage", "case": "c", "device": _hip.device_name(), "dd_lrpt_jpeg": jpeg_kernel()}
    if a.kernel_only:
        print(json.dumps(res), flush=True)
        return
    raw, fs = recording(a.duration, "c")
    src = source.IQarray(raw, fs)

    def run():
        o = decode_meteorm2.decode_meteorm2(src, 0, None)
        pk = o.getPackets
        _hip.sync()
        t0 = time.perf_counter()
        img = o.getImage
        return o, img, time.perf_counter() - t0, pk
    obj, img, first, pkts = run()
    runs = [run() for _ in range(a.reps)]
    assert all(np.array_equal(r[1], img) for r in runs)
    info = obj.imageInfo
    t0 = time.perf_counter()
    want, _ = lrpt.image_np(pkts)
    host = time.perf_counter() - t0
    assert np.array_equal(want, img)
    res.update({"duration_s": a.duration, "samples": int(raw.shape[0]), "frames": int(len(obj.getFrames)), "packets": len(pkts),
                "image_packets": int(len(info)), "placed": int(np.sum(info["strip"] >= 0)), "whole": int(np.sum(info["mcus"] == 14)),
                "image_shape": list(img.shape), "first_image_ms": round(first * 1e3, 3),
                "warm_image_ms": round(float(np.median([r[2] for r in runs])) * 1e3, 3),
                "warm_stage_ms": {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings},
                "image_np_host_ms": round(host * 1e3, 1)})
    print(json.dumps(res), flush=True)


def main_modes(a):
    import _lrpt_modes
    from directdemod_amd import _hip, decode_lrpt, lrpt
    _hip.require_gpu()
    nsym = int(a.duration * 80000)
    depth = lrpt.INTERLEAVER_BRANCHES * lrpt.INTERLEAVER_DELAY * (lrpt.INTERLEAVER_BRANCHES - 1)       # bits
    nframes = max((nsym * 72 // 80 - depth) // lrpt.FRAME_BITS, 1)            # the run-out after them is the interleaver's depth again
    bodies = np.tile(_lrpt_modes.random_bodies(51, 16), (-(-nframes // 16), 1))[:nframes]
    s = _lrpt_modes.stream(bodies, 52, differential=True, interleaved=True, branches=lrpt.INTERLEAVER_BRANCHES,
                           delay=lrpt.INTERLEAVER_DELAY, start=3000, prefix=17, hyp=5)
    soft = _hip.DevArray.from_host(s["soft"])

    def run():
        o = decode_lrpt.decode_lrpt(soft, differential=True, interleaved=True)
        _hip.sync()
        t0 = time.perf_counter()
        frames = o.getFrames
        return o, frames, time.perf_counter() - t0
    obj, frames, first = run()
    runs = [run() for _ in range(a.reps)]
    assert all(np.array_equal(r[1], frames) for r in runs)
    info = obj.frameInfo
    assert obj.locked and info["symbol"].tolist() == s["starts"][1:] and np.array_equal(frames, bodies[1:])
    print(json.dumps({"stage": "decode_lrpt.getFrames", "case": "d", "duration_s": a.duration, "symbols": s["nsym"],
                      "symbols_deinterleaved": int(obj._deint()[2]), "frames": int(len(frames)),
                      "frames_asm_clean": int(np.sum(info["asm_errors"] == 0)), "lock": {k: int(v) for k, v in obj.lock.items()},
                      "first_frames_ms": round(first * 1e3, 3), "warm_frames_ms": round(float(np.median([r[2] for r in runs])) * 1e3, 3),
                      "warm_stage_ms": {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings},
                      "device": _hip.device_name()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=float, default=60.0)
    ap.add_argument("--case", choices=("a", "b", "c", "d"), default="a")
    ap.add_argument("--kernel-only", action="store_true", help="case c: stop after the dd_lrpt_jpeg calls")
    a = ap.parse_args()
    if a.case == "c":
        return main_image(a)
    if a.case == "d":
        return main_modes(a)
    from directdemod_amd import _hip, decode_meteorm2, source
    _hip.require_gpu()
    raw, fs = recording(a.duration, a.case)
    src = source.IQarray(raw, fs)

    def run():
        o = decode_meteorm2.decode_meteorm2(src, 0, None)
        _hip.sync()
        t0 = time.perf_counter()
        o.getSyncs
        t1 = time.perf_counter()
        frames = o.getFrames
        t2 = time.perf_counter()
        o.getPackets
        return o, frames, t1 - t0, t2 - t1, time.perf_counter() - t2
    obj, frames, first_pass, first_frames, first_packets = run()
    runs = [run() for _ in range(a.reps)]
    assert all(np.array_equal(r[1], frames) for r in runs)
    st = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    info = obj.frameInfo
    assert all(r[0].getPackets == obj.getPackets for r in runs)
    print(json.dumps({"stage": "meteorm2.getFrames", "case": a.case, "duration_s": a.duration, "samples": int(raw.shape[0]), "symbols": obj.walker().nsym,
                      "frames": int(len(frames)), "frames_asm_clean": int(np.sum(info["asm_errors"] == 0)),
                      "frames_rs_ok": int(np.sum(obj.rsInfo["ok"])), "frames_rs_corrected": int(np.sum(obj.rsInfo["ok"] & (obj.rsInfo["errors"].max(axis=1) > 0))),
                      "packets": len(obj.getPackets), "packets_distinct": len(set(obj.getPackets)),
                      "first_pass_ms": round(first_pass * 1e3, 3), "first_frames_ms": round(first_frames * 1e3, 3),
                      "first_packets_ms": round(first_packets * 1e3, 3),
                      "warm_pass_ms": round(float(np.median([r[2] for r in runs])) * 1e3, 3),
                      "warm_frames_ms": round(float(np.median([r[3] for r in runs])) * 1e3, 3),
                      "warm_packets_ms": round(float(np.median([r[4] for r in runs])) * 1e3, 3),
                      "warm_stage_ms": st, "device": _hip.device_name()}), flush=True)


if __name__ == "__main__":
    main()
