"""Sensitivity of the RS41 decoder by the NumPy restatement (no GPU): the frames kept against Eb/N0, without Reed-Solomon (every
block's CRC holds in the frame as received) and with it (both codewords decode), per cut-off of the audio-rate channel filter, on a
240 kS/s recording cut to 48 kS/s audio.  Each recording holds --frames standard frames of random content 25 kHz above the centre.
Eb/N0 = A^2 fs / (2 sigma^2 4800) for amplitude A and noise sigma per rail.  Prints the table INTEGRATION.md quotes; rs41.CUT is the
cut-off that keeps the most frames around the knee.

    python tools/sens_rs41.py [--frames 20] [--cuts 3600 4800 6000 7200]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from directdemod_amd import rs41  # noqa: E402

FS, BW, OFFSET = 240000, 48000.0, 25000.0
EBN0 = range(6, 20, 2)
AMPLITUDE = 40.0
GAP = 0.62                                                            # seconds from frame to frame: 2880 bits and a little


def recording(ebn0_db, frames, seed):
    sigma = AMPLITUDE * np.sqrt(FS / (2.0 * rs41.BAUD * 10.0 ** (ebn0_db / 10.0)))
    rng = np.random.default_rng(seed)
    fields = [dict(frame_number=int(rng.integers(0, 65536)), serial="N%07d" % k, gps_week=2300, gps_tow=int(rng.integers(0, 604800000)),
                   lat=float(rng.uniform(-80, 80)), lon=float(rng.uniform(-180, 180)), alt=float(rng.uniform(0, 35000)),
                   meas_raw=[int(v) for v in rng.integers(0, 1 << 24, 12)], gpsraw=bytes(rng.integers(0, 256, 0x59).astype(np.uint8)))
              for k in range(frames)]
    raw = rs41.encode_iq(fields, FS, OFFSET, gap=GAP, start=2000.0 + rng.uniform(0.0, 50.0), amplitude=AMPLITUDE, sigma=sigma,
                         seed=int(rng.integers(1 << 31)))
    return raw, fields


def point(raw, fields, cut):
    """(frames whose blocks all hold as received, frames whose codewords both decode) among those sent"""
    audio, rate = rs41.audio_host(raw, FS, OFFSET, BW, cut)
    found, _, det = rs41.decode(audio, rate, follow=0)
    sent = {f["serial"] for f in fields}
    with_rs = {f["serial"] for f in found if f["status"] == "ok"} & sent
    without = set()
    for i in np.flatnonzero(det["status"] == rs41.OK):
        blocks = rs41.blocks_of(det["recv"][i], int(det["length"][i]), True)
        if len(blocks) == 6 and all(b["crc_ok"] for b in blocks):
            without.add(rs41.parse(blocks)["serial"])
    return len(without & sent), len(with_rs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--cuts", type=float, nargs="+", default=[3600.0, 4800.0, 6000.0, 7200.0])
    a = ap.parse_args()
    sps, w, _ = rs41.params(BW)
    print("%d S/s recording, %g S/s audio, %g samples per bit, w = %d; kept of %d frames without / with Reed-Solomon" % (FS, BW, sps, w, a.frames))
    print("| Eb/N0 dB | " + " | ".join("%g Hz" % c for c in a.cuts) + " |")
    print("|---|" + "---|" * len(a.cuts))
    for db in EBN0:
        raw, fields = recording(db, a.frames, 1000 * db)
        print("| %d | " % db + " | ".join("%d / %d" % point(raw, fields, c) for c in a.cuts) + " |", flush=True)


if __name__ == "__main__":
    main()
