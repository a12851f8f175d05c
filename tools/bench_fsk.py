#!/usr/bin/env python3
"""
Side benchmark of G3RUH 9600 baud FSK decoding (decode_fsk9600.getFrames): the time per stage -- the front
end (offsetFreq, blackmanHarris(151), bwLim, demod_fm), the timing walk, the decision / descrambler / NRZI stage and the frame
check -- on a 2.048 MS/s u8 IQ recording, 20 kHz below the centre, synthesised once by tiling tests/_fsk.py's 0.45 s recording (four
frames, one with a corrupted CRC).  The carrier and the bit clock jump at the seams; the frames inside a tile are whole, and the
walk's work per sample does not depend on what it reads.  First call in the process and warm (median of --reps, a fresh decoder
object each time); the walk's time per audio sample is the figure: it is one lane's dependent chain.  Prints one JSON line.  The
library must have been built (python __graft_entry__.py).

    python tools/bench_fsk.py [--reps 3] [--duration 60]
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

FS, OFFSET = 2048000, -20000


def recording(dur):
    import _fsk
    line, _ = _fsk.line_bits()
    raw = _fsk.fm_iq(line, FS, 41, ppm=100.0, f_carrier=float(OFFSET))
    n = int(dur * FS)
    return np.tile(raw, (-(-n // raw.shape[0]), 1))[:n], -(-n // raw.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--duration", type=float, default=60.0)
    a = ap.parse_args()
    from directdemod_amd import _hip, decode_fsk9600, source
    _hip.require_gpu()
    raw, tiles = recording(a.duration)
    src = source.IQarray(raw, FS)

    def run():
        o = decode_fsk9600.decode_fsk9600(src, OFFSET)
        _hip.sync()
        t0 = time.perf_counter()
        frames = o.getFrames
        return o, frames, time.perf_counter() - t0
    obj, frames, first = run()
    runs = [run() for _ in range(a.reps)]
    assert all([f["raw"] for f in r[1]] == [f["raw"] for f in frames] for r in runs)
    info = obj.bitInfo
    audio = obj.audio().n
    st = {k: round(float(np.median([r[0].timings[k] for r in runs])) * 1e3, 3) for k in runs[0][0].timings}
    print(json.dumps({"stage": "fsk9600.getFrames", "duration_s": a.duration, "samples": int(raw.shape[0]), "audio_samples": audio,
                      "audio_rate": obj.audioRate, "tiles": tiles, "symbols": info["symbols"], "flags": info["flags"],
                      "frames": info["frames"], "period": info["period"], "first_ms": round(first * 1e3, 3),
                      "warm_ms": round(float(np.median([r[2] for r in runs])) * 1e3, 3), "warm_stage_ms": st,
                      "walk_ns_per_sample": round(st["walk"] * 1e6 / max(audio, 1), 3),
                      "walk_us_per_symbol": round(st["walk"] * 1e3 / max(info["symbols"], 1), 4), "device": _hip.device_name()}),
          flush=True)


if __name__ == "__main__":
    main()
