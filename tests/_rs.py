"""Seeded Meteor-M2 LRPT recordings that carry real frames, for the Reed-Solomon and packet tests: CCSDS
source packets (random APIDs from a small set, random lengths, with the special lengths forced in: a packet that ends exactly at a
zone's end, headers split with 1 and with 5 bytes left in the zone, packets that span three frames) are laid into the M_PDU zones of
two virtual channels with running counters (one of them wraps 2^24) plus one fill frame, RS-encoded and interleaved into bodies, and
sent through _lrpt.frames_bits, lrpt.encode and the waveform of _lrpt.synth (its lines are restated here for given bodies).
Deterministic from the seed (NumPy PCG64); the fixture stores the sha256 of the recording it was made from.

Case (b) has two fades -- stretches of samples replaced by noise alone -- in frames well past loop acquisition.  Their lengths were
chosen on the CPU, over the reference's own symbol walk (tools/gen_golden.py --lrpt-rs) and lrpt.py's restatement:

  - the short fade, 5400 samples (190 symbols) from symbol 3000 of sent frame 6: the restatement reports 6, 6, 5, 6 byte errors in
    that frame's four codewords, all corrected (re-encode count 63);
  - the long fade, 20000 samples (703 symbols) from symbol 3000 of sent frame 9: all four codewords of that frame are not decodable
    (-1, -1, -1, -1; re-encode count 196);
  - the loops stay locked: the frames found are the sent frames 2..11 at symbols 8451 + 8192 i under hypothesis 3, and every frame
    but those two decodes with 0 errors in all four codewords, frames 7, 8 and 10, 11 after the fades included;
  - frame 10's first header pointer is 118 and the packet that starts there (318 bytes, channel 12) is the first one recovered after
    the long fade; the 1827-byte packet of channel 5 that spans frames 3, 6 and 7 arrives only because frame 6 is corrected.
"""
import numpy as np

from _meteor import FS, sha256  # noqa: F401

import _lrpt
from directdemod_amd import lrpt

APIDS = (64, 65, 68, 70)
VCIDS = (5, 12)
FIRST_COUNTER = {5: 1000, 12: (1 << 24) - 3}      # channel 12's counter wraps inside the recording
ORDER = (5, 5, 12, 5, 63, 12, 5, 5, 12, 5, 12, 5, 5, 12, 5, 12)          # whose frame it is, cyclically; 63 is fill
PLAN = ("rand", "exact", "rand", "split1", "rand", "long", "rand", "split5", "rand", "rand", "rand", "rand")
ZONE = lrpt.ZONE_BYTES

# case b: (sent frame, first faded symbol of that frame, faded samples)
FADES = ((6, 3000, 5400), (9, 3000, 20000))
CASES = {
    "b": dict(seed=32, seconds=1.3, carrier=300.0, phase=0.7, amp=40.0, sigma=4.0, fades=FADES),
}
SHORT, LONG = FADES[0][0], FADES[1][0]            # the sent frames the fades lie in


def packet(apid, count, length, rng, flags=3):
    """one source packet of `length` >= 7 bytes in all: version 0, telemetry, no secondary header"""
    head = bytes([(apid >> 8) & 7, apid & 0xFF, (flags << 6) | ((count >> 8) & 0x3F), count & 0xFF, ((length - 7) >> 8) & 0xFF,
                  (length - 7) & 0xFF])
    return head + rng.integers(0, 256, length - 6, dtype=np.uint8).tobytes()


def channel_stream(rng, nzones, step=0):
    """packets back to back over nzones zones of one channel -> [(first byte's offset in the stream, bytes)]; the last one runs past
    the end.  PLAN names each packet's length: random, or such that it ends exactly at a zone's end ("exact"), 1 or 5 bytes before
    it (the next header is split), or after two more zones ("long")."""
    out, pos, counts = [], 0, {}
    while pos < nzones * ZONE:
        kind = PLAN[step % len(PLAN)]
        step += 1
        room = ZONE - pos % ZONE
        if kind == "rand":
            n = int(rng.integers(30, 400))
        elif kind == "long":
            n = 2 * ZONE + int(rng.integers(50, 300))
        else:
            n = room - {"exact": 0, "split1": 1, "split5": 5}[kind]
            n += ZONE if n < 7 else 0
        apid = int(APIDS[int(rng.integers(0, len(APIDS)))])
        counts[apid] = (counts.get(apid, -1) + 1) & 0x3FFF
        out.append((pos, packet(apid, counts[apid], n, rng)))
        pos += n
    return out


def vcdu(vcid, counter, fhp, zone):
    """version 1, spacecraft 0, no replay, an empty insert zone"""
    head = bytes([0x40, vcid & 0x3F, (counter >> 16) & 0xFF, (counter >> 8) & 0xFF, counter & 0xFF, 0, 0, 0, (fhp >> 8) & 7, fhp & 0xFF])
    return np.frombuffer(head + bytes(zone), dtype=np.uint8)


def zones(pk, nzones):
    """[(offset, bytes)] back to back -> per zone (first-header pointer, the zone's 882 bytes)"""
    data = b"".join(p for _, p in pk)
    out = []
    for i in range(nzones):
        heads = [at - i * ZONE for at, _ in pk if i * ZONE <= at < (i + 1) * ZONE]
        out.append((heads[0] if heads else lrpt.NO_HEADER, data[i * ZONE:(i + 1) * ZONE]))
    return out


def build(rng, nframes):
    """-> dict: vcdus uint8[n, 892], bodies uint8[n, 1020] (RS-encoded, interleaved), vcid[n], counter[n], and packets: every source
    packet laid in, as dict(data, vcid, first, last) with the frames (rows) of its first byte and of its completion, per channel in
    stream order; last is None for a packet that is not completed by the last frame"""
    vcid = np.array([ORDER[i % len(ORDER)] for i in range(nframes)], dtype=np.int64)
    counter = np.zeros(nframes, dtype=np.int64)
    vcdus = np.zeros((nframes, lrpt.VCDU_BYTES), dtype=np.uint8)
    packets = []
    for k, v in enumerate(VCIDS + (lrpt.FILL_VCID,)):
        rows = np.nonzero(vcid == v)[0]
        counter[rows] = (FIRST_COUNTER.get(v, 77) + np.arange(len(rows))) & 0xFFFFFF
        if v == lrpt.FILL_VCID:
            for r in rows:
                vcdus[r] = vcdu(v, int(counter[r]), 0x7FE, rng.integers(0, 256, ZONE, dtype=np.uint8))
            continue
        pk = channel_stream(rng, len(rows), step=5 * k)
        for r, (fhp, zone) in zip(rows, zones(pk, len(rows))):
            vcdus[r] = vcdu(v, int(counter[r]), fhp, zone)
        for at, p in pk:
            end = (at + len(p) - 1) // ZONE
            # a continued packet whose last byte is its zone's last is closed by the channel's next frame (whose pointer is 0)
            close = end + 1 if (at + len(p)) % ZONE == 0 and end > at // ZONE else end
            packets.append(dict(data=p, vcid=v, first=int(rows[at // ZONE]), last=int(rows[close]) if close < len(rows) else None))
    bodies = lrpt.interleave(lrpt.rs_encode(vcdus.reshape(nframes, lrpt.VCDU_BYTES // 4, 4).swapaxes(1, 2)))
    return dict(vcdus=vcdus, bodies=bodies, vcid=vcid, counter=counter, packets=packets)


def expected(built, state):
    """The packets the definitions deliver when sent frame i is state[i] -- "ok" (all four codewords decoded), "failed" (found, not
    decodable) or "missing" (never found) -- in order of completion: a packet arrives iff every frame of its channel from its first
    byte to its completion is ok and no failed frame of any channel lies between the two (a failed frame drops every channel's partial
    packet; a missing one shows only as a gap in its own channel's counter).  Ties in the completing frame keep the stream's order."""
    got = []
    for i, p in enumerate(built["packets"]):
        if p["last"] is None:
            continue
        rows = range(p["first"], p["last"] + 1)
        if all(state[r] == "ok" for r in rows if built["vcid"][r] == p["vcid"]) and not any(state[r] == "failed" for r in rows):
            got.append((p["last"], i))
    return [built["packets"][i] for _, i in sorted(got)]


def synth(seed, seconds, carrier=0.0, phase=0.0, amp=40.0, sigma=4.0, fades=()):
    """-> (uint8[n, 2] IQ pairs centred on 127.5, built, start): _lrpt.synth for the frames of build(), the recording starting at
    bit `start` of the first; a fade (frame, symbol, samples) zeroes the signal under the noise from that symbol of that frame on"""
    n = int(round(seconds * FS))
    nsym = n * 9 // 256 + 2
    rng = np.random.Generator(np.random.PCG64(seed))
    built = build(rng, nsym // lrpt.FRAME_BITS + 2)
    start = int(rng.integers(0, lrpt.FRAME_BITS))
    code = lrpt.encode(_lrpt.frames_bits(built["bodies"])).reshape(-1, 2)[start:start + nsym]
    sym = (2.0 * code[:, 0] - 1.0) + 1j * (2.0 * code[:, 1] - 1.0)
    t = np.arange(n, dtype=np.int64)
    x = amp * sym[t * 9 // 256]
    for frame, at, length in fades:
        first = -(-(lrpt.FRAME_BITS * frame - start + at) * 256 // 9)
        x[first:first + length] = 0.0
    x = x * np.exp(1j * (2.0 * np.pi * carrier * t / FS + phase))
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.stack((x.real, x.imag), axis=1) + 127.5
    return np.clip(np.rint(iq), 0, 255).astype(np.uint8), built, start


def case(name):
    """(raw, built, start) of a named case"""
    return synth(**CASES[name])


def match(built, vcids, counters, ok):
    """decoded frames -> (sent frame per row, state per sent frame): ok rows are found by (vcid, counter), a row that is not ok is the
    sent frame after the last ok one"""
    where = {(int(v), int(c)): i for i, (v, c) in enumerate(zip(built["vcid"], built["counter"]))}
    rows, state, last = [], ["missing"] * len(built["vcid"]), -1
    for v, c, good in zip(vcids, counters, ok):
        last = where[(int(v), int(c))] if good else last + 1
        rows.append(last)
        state[last] = "ok" if good else "failed"
    return rows, state
