#!/usr/bin/env python3
"""
Side benchmark of AIS decoding (decode_ais): the time per stage -- the front end of both channels, the
preamble candidates, the demodulation of the survivors, the host's merge, parse and sentences -- on a synthesised recording at
2.4 MS/s: one second holding --bursts bursts (the eight published messages in turn, alternating channels, amplitudes 25 to 60,
carrier errors within +-500 Hz, noise of sigma 6 per rail), tiled --duration times (60: a minute, 144 000 000 samples).

First call in the process and warm (median of --reps, a fresh decoder object each time over an IQarray whose pairs stay resident on
the device, a device synchronisation after every stage).  Nothing is gated on the numbers.  Prints one JSON line.  The library must
have been built (python __graft_entry__.py).

    python tools/bench_ais.py [--reps 3] [--duration 60] [--bursts 16]
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
OFFSETS = (-25000.0, 25000.0)
SENTENCES = [["!AIVDM,1,1,,B,177KQJ5000G?tO`K>RA1wUbN0TKH,0*5C"], ["!AIVDM,1,1,,A,13u?etPv2;0n:dDPwUM1U1Cb069D,0*24"],
             ["!AIVDM,1,1,,B,15NG6V0P01G?cFhE`R2IU?wn28R>,0*05"], ["!AIVDM,1,1,,A,403OviQuMGCqWrRO9>E6fE700@GO,0*4D"],
             ["!AIVDM,2,1,3,B,55P5TL01VIaAL@7WKO@mBplU@<PDhh000000001S;AJ::4A80?4i@E53,0*3E", "!AIVDM,2,2,3,B,1@0000000000000,2*55"],
             ["!AIVDM,1,1,,A,B52K>;h00Fc>jpUlNV@ikwpUoP06,0*4C"], ["!AIVDM,1,1,,A,H42O55i18tMET00000000000000,2*6D"],
             ["!AIVDM,1,1,,A,H42O55lti4hhhilD3nink000?050,0*40"]]


def second(bursts, seed=41):
    """one second of recording with `bursts` bursts, none inside another"""
    from directdemod_amd import ais
    rng = np.random.default_rng(seed)
    msgs = [np.packbits(ais.from_nmea(s)[0]).tobytes() for s in SENTENCES]
    slot = RATE // bursts
    longest = max(ais.burst_len(m, RATE) for m in msgs) + 8
    if slot <= longest:
        raise SystemExit("at most %d bursts fit a second" % (RATE // (longest + 1)))
    starts = slot * np.arange(bursts) + rng.uniform(0.0, slot - longest, bursts)
    sent = [msgs[i % len(msgs)] for i in range(bursts)]
    chans = [OFFSETS[i % 2] for i in range(bursts)]
    raw = ais.encode(sent, RATE, starts, chans, rng.uniform(25.0, 60.0, bursts), 6.0, seed, rng.uniform(-500.0, 500.0, bursts), n=RATE)
    return raw, sent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=int, default=60)
    ap.add_argument("--bursts", type=int, default=16)
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_ais, source
    _hip.require_gpu()
    one, sent = second(a.bursts)
    raw = np.tile(one, (a.duration, 1))

    def run(src):
        o = decode_ais.decode_ais(src, OFFSETS)
        _hip.sync()
        t0 = time.perf_counter()
        msgs = o.getMsgs
        return o, msgs, time.perf_counter() - t0
    obj, msgs, first = run(source.IQarray(raw, RATE))                # (the first call uploads the recording)
    src = source.IQarray(raw, RATE)
    src.read_device_raw(0, len(raw))
    runs = [run(src) for _ in range(a.reps)]
    assert all([m["raw"] for m in r[1]] == [m["raw"] for m in msgs] for r in runs)
    info = obj.frameInfo
    stages = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    warm = float(np.median([r[2] for r in runs]))
    print(json.dumps({"stage": "decode_ais", "samples": int(len(raw)), "seconds": a.duration, "rate": RATE, "audio_rate": obj.audioRate,
                      "channels": len(OFFSETS), "bursts_sent": a.bursts * a.duration, "messages": len(msgs),
                      "audio_samples": info["samples"], "candidates": info["candidates"], "duplicates": info["duplicates"],
                      "first_ms": round(first * 1e3, 3), "first_stage_ms": {k: round(v * 1e3, 3) for k, v in obj.timings.items()},
                      "warm_ms": round(warm * 1e3, 3), "warm_stage_ms": stages,
                      "candidates_ns_per_audio_sample": round(stages["candidates"] * 1e6 / max(info["samples"] * len(OFFSETS), 1), 4),
                      "demod_us_per_survivor": round(stages["demod"] * 1e3 / max(info["candidates"], 1), 4),
                      "device": _hip.device_name()}), flush=True)


if __name__ == "__main__":
    main()
