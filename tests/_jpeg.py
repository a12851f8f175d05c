"""An encoder for the Meteor-M2 LRPT image packets of DESIGN.md section 4.16, for the image tests: stated on its own, not by way of
the decoder's restatement in lrpt.py -- only the tables' constants (BITS / values, the zigzag order) and quantiser(q) are shared.
A float64 forward DCT, division by quantiser(q) with rounding, zigzag, and Huffman coding with the canonical codes built here from
the value to the code; a bit writer for hand-built streams; a packet builder (secondary-header flag, on-board time, mcun, q); and a
layer that lays a list of packets into the M_PDU zones of one virtual channel (_rs.vcdu / _rs.zones), RS-encodes them
(lrpt.rs_encode) and modulates them with the lines of _rs.synth.  Deterministic from the seed (NumPy PCG64)."""
import numpy as np

from _meteor import FS  # noqa: F401

import _lrpt
import _rs
from directdemod_amd import lrpt

VCID = 5
TELEMETRY_APID = 70
ZONE = lrpt.ZONE_BYTES


def _codes(bits, values):
    """value -> (code, length), the canonical assignment: within a length in value order, code = (code + count) << 1"""
    out, code, k = {}, 0, 0
    for length, count in enumerate(bits, start=1):
        for _ in range(count):
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC = _codes(lrpt.DC_BITS, lrpt.DC_VALUES)
AC = _codes(lrpt.AC_BITS, lrpt.AC_VALUES)
_C = np.array([[(np.sqrt(1 / 8) if k == 0 else 0.5) * np.cos((2 * n + 1) * k * np.pi / 16) for n in range(8)] for k in range(8)])


def category(v):
    """the number of bits of |v|"""
    return int(abs(int(v))).bit_length()


class Writer:
    """bits, MSB first: symbols of the two tables, values in T.81's sign convention, raw patterns"""

    def __init__(self):
        self.bits = []

    def raw(self, value, length):
        self.bits += [(value >> (length - 1 - i)) & 1 for i in range(length)]
        return self

    def value(self, v, n=None):
        n = category(v) if n is None else n
        return self.raw(v if v >= 0 else v + (1 << n) - 1, n) if n else self

    def dc(self, diff):
        n = category(diff)
        return self.raw(*DC[n]).value(diff, n)

    def ac(self, run, v):
        n = category(v)
        return self.raw(*AC[(run << 4) | n]).value(v, n)

    def symbol(self, rs):
        return self.raw(*AC[rs])

    def eob(self):
        return self.symbol(0x00)

    def zrl(self):
        return self.symbol(0xF0)

    def __len__(self):
        return len(self.bits)

    def bytes(self, pad=1):
        """the bits, the last byte filled with `pad` bits"""
        b = self.bits + [pad] * (-len(self.bits) % 8)
        return np.packbits(np.array(b, dtype=np.uint8)).tobytes()


def forward(blocks, table):
    """pixels [..., 8, 8] -> quantised coefficients int64[..., 64], row-major: C (p - 128) C^T / table, rounded to nearest; the DC term
    kept to 11 bits' differences and the AC terms to 10 bits"""
    F = np.einsum("uy,...yx,vx->...uv", _C, np.asarray(blocks, dtype=np.float64) - 128.0, _C)
    c = np.rint(F.reshape(F.shape[:-2] + (64,)) / np.asarray(table, dtype=np.float64)).astype(np.int64)
    return np.clip(c, -1023, 1023)


def write_block(w, c, pred):
    """one block's coefficients (row-major) onto the writer; -> the new predictor"""
    z = [int(c[lrpt.ZIGZAG[k]]) for k in range(64)]
    w.dc(z[0] - pred)
    run = 0
    for k in range(1, 64):
        if z[k] == 0:
            run += 1
            continue
        while run > 15:
            w.zrl()
            run -= 16
        w.ac(run, z[k])
        run = 0
    if run:
        w.eob()
    return z[0]


def encode(coef):
    """quantised coefficients int[m, 64] of one packet's blocks -> its entropy-coded bytes"""
    w, pred = Writer(), 0
    for c in coef:
        pred = write_block(w, c, pred)
    return w.bytes()


def encode_strip(strip, q):
    """pixels uint8[8, 112] -> (the packet's entropy-coded bytes, the coefficients int64[14, 64])"""
    blocks = np.asarray(strip).reshape(8, 14, 8).transpose(1, 0, 2)
    coef = forward(blocks, lrpt.quantiser(q))
    return encode(coef), coef


def strip_of(pixels):
    """blocks uint8[14, 8, 8] -> the strip uint8[8, 112]"""
    return np.asarray(pixels).transpose(1, 0, 2).reshape(8, 8 * len(pixels))


def packet(apid, count, payload, mcun=0, q=80, time=(0, 0, 0), secondary=1, flags=3):
    """an image packet: primary header (version 0, telemetry), the on-board time (day, ms, us), mcun, two table selectors, two
    bytes that are ignored, q, then the payload"""
    day, ms, us = time
    body = (bytes([day >> 8, day & 0xFF]) + int(ms).to_bytes(4, "big") + bytes([us >> 8, us & 0xFF, mcun, 0x00, 0x00, 0xFF, 0xF0, q])
            + bytes(payload))
    n = 6 + len(body)
    head = bytes([(secondary << 3) | ((apid >> 8) & 7), apid & 0xFF, (flags << 6) | ((count >> 8) & 0x3F), count & 0xFF,
                  ((n - 7) >> 8) & 0xFF, (n - 7) & 0xFF])
    return head + body


def picture(rng, strips, noise=6.0):
    """uint8[8 strips, 1568, 3]: smooth waves plus noise, different in every channel"""
    y, x = np.mgrid[0:8 * strips, 0:lrpt.IMAGE_WIDTH]
    planes = [128 + 90 * np.sin(x / (40.0 + 25 * j) + j) * np.cos(y / (9.0 + 4 * j)) + noise * rng.standard_normal(x.shape) for j in range(3)]
    return np.clip(np.rint(np.stack(planes, axis=2)), 0, 255).astype(np.uint8)


def cycles(rng, pic, q=60, first_count=16384 - 60, apids=lrpt.IMAGE_APIDS, day=7000):
    """the picture's packets in transmission order: per strip cycle 14 image packets of each channel, then one telemetry packet with
    the cycle's 43rd count -> [dict(data, image: None or (channel, strip, mcun))]; the shared sequence counter wraps 16384"""
    out, count = [], first_count
    for s in range(pic.shape[0] // 8):
        for j, apid in enumerate(apids):
            for m in range(0, lrpt.MCU_PER_STRIP, lrpt.MCU_PER_PACKET):
                payload, _ = encode_strip(pic[8 * s:8 * s + 8, 8 * m:8 * m + 112, j], q)
                out.append(dict(data=packet(apid, count & 0x3FFF, payload, m, q, (day, 1000 * s + 10 * j, m)), image=(j, s, m)))
                count += 1
        out.append(dict(data=packet(TELEMETRY_APID, count & 0x3FFF, rng.integers(0, 256, 42, dtype=np.uint8).tobytes(), 0, 0,
                                    (day, 1000 * s + 900, 0)), image=None))
        count += 1
    return out


def build(pkts, nframes, first_counter=500):
    """packets (cycles' dicts) back to back in the zones of nframes frames of one virtual channel -> _rs.build's dict, each packet
    with its `image` entry; there must be enough of them to fill the zones, the last one laid runs past the end"""
    at, laid = 0, []
    for p in pkts:
        if at >= nframes * ZONE:
            break
        laid.append((at, p))
        at += len(p["data"])
    assert at >= nframes * ZONE, "not enough packets for %d frames" % nframes
    zs = _rs.zones([(a, p["data"]) for a, p in laid], nframes)
    counter = (first_counter + np.arange(nframes)) & 0xFFFFFF
    vcdus = np.stack([_rs.vcdu(VCID, int(c), fhp, zone) for c, (fhp, zone) in zip(counter, zs)])
    packets = []
    for a, p in laid:
        end = (a + len(p["data"]) - 1) // ZONE
        close = end + 1 if (a + len(p["data"])) % ZONE == 0 and end > a // ZONE else end
        packets.append(dict(data=p["data"], vcid=VCID, first=a // ZONE, last=close if close < nframes else None, image=p["image"]))
    bodies = lrpt.interleave(lrpt.rs_encode(vcdus.reshape(nframes, lrpt.VCDU_BYTES // 4, 4).swapaxes(1, 2)))
    return dict(vcdus=vcdus, bodies=bodies, vcid=np.full(nframes, VCID, dtype=np.int64), counter=counter.astype(np.int64),
                packets=packets)


def modulate(rng, bodies, seconds, carrier=300.0, phase=0.7, amp=40.0, sigma=4.0, fades=()):
    """_rs.synth's waveform for given bodies -> (uint8[n, 2] IQ pairs, start)"""
    n = int(round(seconds * FS))
    nsym = n * 9 // 256 + 2
    assert len(bodies) >= nsym // lrpt.FRAME_BITS + 2
    start = int(rng.integers(0, lrpt.FRAME_BITS))
    code = lrpt.encode(_lrpt.frames_bits(bodies)).reshape(-1, 2)[start:start + nsym]
    sym = (2.0 * code[:, 0] - 1.0) + 1j * (2.0 * code[:, 1] - 1.0)
    t = np.arange(n, dtype=np.int64)
    x = amp * sym[t * 9 // 256]
    for frame, at, length in fades:
        first = -(-(lrpt.FRAME_BITS * frame - start + at) * 256 // 9)
        x[first:first + length] = 0.0
    x = x * np.exp(1j * (2.0 * np.pi * carrier * t / FS + phase))
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.stack((x.real, x.imag), axis=1) + 127.5
    return np.clip(np.rint(iq), 0, 255).astype(np.uint8), start


# case c: three channels, strip cycles back to back in one virtual channel; one frame lost to a fade as in _rs.FADES, one bit of an
# image packet in another frame flipped after RS encoding
FADE = (9, 3000, 20000)
FLIP = (6, 10 + 300, 0x10)                            # (sent frame, body byte, mask): inside that frame's packet zone
CASES = {"c": dict(seed=33, seconds=2.0, q=60)}


def case(name="c"):
    """-> (raw, built, start, pic): the recording, what was laid into it (build's dict), its first bit, the sent picture"""
    c = CASES[name]
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    nframes = (int(round(c["seconds"] * FS)) * 9 // 256 + 2) // lrpt.FRAME_BITS + 2
    pic = picture(rng, 8)
    built = build(cycles(rng, pic, c["q"]), nframes)
    bodies = built["bodies"].copy()
    bodies[FLIP[0], FLIP[1]] ^= FLIP[2]
    raw, start = modulate(rng, bodies, c["seconds"], fades=(FADE,))
    return raw, built, start, pic
