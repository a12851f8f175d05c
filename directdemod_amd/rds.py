"""
RDS on broadcast FM: 1187.5 bit/s, differentially coded biphase symbols on a 57 kHz subcarrier of the multiplex, groups of four 26-bit
blocks (16 information bits and a 10-bit checkword of the shortened cyclic code g = 0x5B9, with an offset word added per block)
(beyond the reference; DESIGN.md section 4.27 defines every stage; device side: dd_rds.h): the constants, the code, a NumPy
restatement `baseband_host` / `halfbit_host` / `scores_host` / `candidates_host` / `groups_host` of the kernels and `repair_np` of the
burst repair, the device wrappers over the C entries, `decode`, the chain behind decode_rds, which runs over either set of stages
(`DeviceOps`, `HostOps`) so that the host logic is one piece of code for both, the merge, the chains, the group parser, and
`encode` / `encode_mpx`, a synthesiser.

The multiplex is the FM discriminator's output in radians per sample at R S/s.  It is quantised (q = rint(mpx 2^15 / pi)), mixed with
a fixed 57 kHz phasor from a 1024-entry table and block-summed by D = int(R / 19000) to about 17 samples per bit: int32 pairs b.
z[p] is the sum of the h = floor(sps / 2) samples from p on less the h before p; bit k of the start t is 1 iff
Re(z[p_k] conj(z[p_(k-1)])) < 0 with p_k = floor((t + k sps) + 0.5).  No carrier and no timing is recovered: the 57 kHz phasor may be
off by the receiver's clock error, which turns z by a degree or two per bit, and every sample is tried as a group's start.

The format is IEC 62106 / EN 50067 as publicly described and has been met in synthesised recordings only; INTEGRATION.md lists the
limits.
"""
import bisect
import functools
import math

import numpy as np

from . import _burst
from ._burst import Laps, need
from ._hip import DevArray, check, lib

BITRATE = 1187.5
SUBCARRIER, PILOT = 57000.0, 19000.0
DEVIATION = 75000.0
RATE_MIN, RATE_MAX = 125000.0, 500000.0
SPS_MIN, SPS_MAX = 12.0, 32.0
TILE = 256                            # DD_RDS_TILE
D_MAX = 32                            # DD_RDS_D_MAX
SHIFT = 10                            # DD_RDS_SHIFT: |q| <= 2^15, |table| <= 2^14, 32 products -> |b| <= 2^24
H_MAX = 16
BITS = 104
SCALE = 32768.0 / np.pi
CLIP = 32768.0
TABLE_BITS = 10
TABLE_AMP = 16384.0
METRIC_SHIFT, METRIC_CAP = 20, 1 << 24
GEN = 0x5B9
A, B, CC, CP, D = range(5)            # the offset words' indices (CC: C, CP: C')
OFFSETS = (0x0FC, 0x198, 0x168, 0x350, 0x1B4)
OK, OUTSIDE = 0, 1
K_CHAIN = 24                          # groups apart at which two starts still chain: the tolerance stays below one bit
PPM = 2e-4                            # a transmitter and a receiver each 100 ppm off
FILLER = 205

_F64 = np.dtype(np.float64)
_I32 = np.dtype(np.int32)


def window_taps(fs):
    """the length of the front end's Blackman-Harris window: the odd number nearest 37 fs / 2 400 000, at least 5, whose main lobe is
    some +-250 kHz from null to null (4 fs / K), so that a +-75 kHz station with its Carson skirts passes (ais.window_taps keeps
    +-60 kHz)"""
    return max(5, 2 * int(round((37.0 * fs / 2400000.0 - 1.0) / 2.0)) + 1)


def params(rate):
    """(D, sps, step) for a multiplex rate R: D = int(R / (16 * 1187.5)) samples per baseband sample, sps = R / D / 1187.5 baseband
    samples per bit, step = rint(57000 * 2^32 / R).  ValueError unless 125 000 <= R <= 500 000 and 12 <= sps <= 32."""
    rate = float(rate) if rate and rate > 0 else float("nan")
    if not RATE_MIN <= rate <= RATE_MAX:
        raise ValueError("rds: a multiplex rate of %r S/s is not supported; %g to %g are" % (rate, RATE_MIN, RATE_MAX))
    d = int(rate / (16.0 * BITRATE))
    sps = rate / d / BITRATE
    if not SPS_MIN <= sps <= SPS_MAX or d > D_MAX:
        raise ValueError("rds: a multiplex rate of %r S/s gives %r samples per bit; %g to %g are supported" % (rate, sps, SPS_MIN, SPS_MAX))
    return d, sps, int(round(SUBCARRIER * 4294967296.0 / rate))


def check_options(clean, fix, follow):
    if int(clean) != clean or not 2 <= clean <= 4:
        raise ValueError("rds: clean must be 2, 3 or 4, got %r" % (clean,))
    if int(fix) != fix or not 0 <= fix <= 5:
        raise ValueError("rds: fix must be from 0 to 5, got %r" % (fix,))
    if int(follow) != follow or follow < 0:
        raise ValueError("rds: follow must be a count from 0 up, got %r" % (follow,))


# ------------------------------------------------------------------------------------------------------------------ the code
def remainder(words):
    """words mod g for 26-bit words (any integer array or a number): the 10-bit remainder"""
    w = np.asarray(words, dtype=np.int64)
    r = np.zeros(w.shape, dtype=np.int64)
    for i in range(25, -1, -1):
        r = (r << 1) | ((w >> i) & 1)
        r = np.where(r & 0x400, r ^ GEN, r)
    return r


def checkword(info, offset):
    """the 10 bits behind the 16 information bits: (info x^10 mod g) XOR the offset word"""
    return int(remainder(int(info) << 10)) ^ OFFSETS[offset]


def block(info, offset):
    """the 26-bit block of an information word"""
    return int(info) << 10 | checkword(info, offset)


def x_power(e):
    """x^e mod g"""
    v = 1
    for _ in range(e):
        v <<= 1
        if v & 0x400:
            v ^= GEN
    return v


@functools.lru_cache(maxsize=None)
def bursts():
    """the 367 bursts of 1 to 5 bits inside 26: a tuple of (error word, remainder, length, ones); a burst begins and ends in a wrong
    bit, so its pattern is an odd number below 32 shifted up"""
    out = []
    for pat in range(1, 32, 2):
        ln = pat.bit_length()
        for up in range(0, 26 - ln + 1):
            e = pat << up
            out.append((e, int(remainder(e)), ln, bin(e).count("1")))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _burst_of():
    return {r: (e, ln, ones) for e, r, ln, ones in bursts()}


def repair_np(word, offset, fix):
    """(block, status) of a 26-bit word held against an offset word: status 0 and the word when it is clean; n and the word without
    the one burst of at most `fix` bits that makes it clean, n its ones; -1 and the word when there is none"""
    word = int(word) & 0x3FFFFFF
    syn = int(remainder(word)) ^ OFFSETS[offset]
    if syn == 0:
        return word, 0
    hit = _burst_of().get(syn)
    if hit is None or hit[1] > fix:
        return word, -1
    return word ^ hit[0], hit[2]


# ------------------------------------------------------------------------------------------------------------------ the restatement
def quantise(mpx):
    """q = rint(mpx * 2^15 / pi) as int64; 0 for a NaN and beyond +-2^15"""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(mpx, dtype=np.float64) * SCALE)
        return np.where((r >= -CLIP) & (r <= CLIP), r, 0.0).astype(np.int64)


@functools.lru_cache(maxsize=None)
def table():
    """int32[1024, 2]: rint(2^14 exp(-2 pi i (j + 1/2) / 1024))"""
    w = np.exp(-2j * np.pi * (np.arange(1 << TABLE_BITS) + 0.5) / (1 << TABLE_BITS))
    t = np.stack((np.rint(TABLE_AMP * w.real), np.rint(TABLE_AMP * w.imag)), axis=1).astype(np.int32)
    t.setflags(write=False)
    return t


def phases(n0, n, step):
    """the table index of the global samples n0 .. n0 + n - 1: bits 31 .. 22 of (j step) mod 2^32"""
    with np.errstate(over="ignore"):
        j = np.uint64(int(n0) & 0xFFFFFFFFFFFFFFFF) + np.arange(n, dtype=np.uint64)
        return (((j * np.uint64(step)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - TABLE_BITS)).astype(np.int64)


def baseband_sums_host(mpx, d, step, n0=0):
    """int64[n // d, 2]: the block sums of q times the table phasor, shifted down (|.| <= 2^24 for d <= 32: the bit budget)"""
    q = quantise(mpx)
    nout = len(q) // d
    q = q[:nout * d]
    w = table()[phases(n0, nout * d, step)].astype(np.int64)
    return (q[:, None] * w).reshape(nout, d, 2).sum(axis=1) >> SHIFT


def baseband_host(mpx, d, step, n0=0):
    """int32[n // d, 2]: the baseband as the device stores it"""
    return baseband_sums_host(mpx, d, step, n0).astype(np.int32)


def halfbit_host(b, h):
    """int64[m, 2]: z[p] = the sum of b[p .. p + h - 1] less the sum of b[p - h .. p - 1] for h <= p <= m - h, else 0"""
    b = np.asarray(b, dtype=np.int64).reshape(-1, 2)
    m = len(b)
    z = np.zeros((m, 2), dtype=np.int64)
    if m >= 2 * h:
        cum = np.concatenate((np.zeros((1, 2), dtype=np.int64), np.cumsum(b, axis=0)))
        p = np.arange(h, m - h + 1)
        z[h:m - h + 1] = cum[p + h] - 2 * cum[p] + cum[p - h]
    return z


def positions(ts, ks, sps):
    """int64[len(ts), len(ks)]: p_k = floor((t + k sps) + 0.5), the product and the sums each rounded to float64"""
    t = np.asarray(ts, dtype=np.int64).astype(np.float64).reshape(-1, 1)
    k = np.asarray(ks, dtype=np.int64).astype(np.float64).reshape(1, -1)
    return np.floor((t + k * sps) + 0.5).astype(np.int64)


def fits(ts, sps, m):
    """the starts whose group lies inside the data: 0 <= t < m, p_-1 >= 0 and p_103 <= m - h"""
    ts = np.asarray(ts, dtype=np.int64).reshape(-1)
    p = positions(ts, [-1, BITS - 1], sps)
    return (ts >= 0) & (ts < m) & (p[:, 0] >= 0) & (p[:, 1] <= m - int(sps // 2))


def products_host(z, ts, sps):
    """int64[len(ts), 104]: Re(z[p_k] conj(z[p_(k-1)])) of starts that fit"""
    p = positions(ts, np.arange(-1, BITS), sps)
    zr, zi = z[p, 0], z[p, 1]
    return zr[:, 1:] * zr[:, :-1] + zi[:, 1:] * zi[:, :-1]


_WEIGHTS = (1 << np.arange(25, -1, -1)).astype(np.int64)


def blocks_host(prod):
    """int64[n, 4]: the four 26-bit blocks, the first-sent bit highest"""
    return ((prod < 0).reshape(len(prod), 4, 26) * _WEIGHTS).sum(axis=2)


def scores_host(b, sps, chunk=1 << 15):
    """uint8[m]: per start the blocks whose remainder is their offset word's (A, B, C or C', D); 0 where the group does not fit"""
    b = np.asarray(b, dtype=np.int64).reshape(-1, 2)
    m = len(b)
    z = halfbit_host(b, int(sps // 2))
    out = np.zeros(m, dtype=np.uint8)
    for a in range(0, m, chunk):
        ts = np.arange(a, min(m, a + chunk), dtype=np.int64)
        ts = ts[fits(ts, sps, m)]
        if not len(ts):
            continue
        r = remainder(blocks_host(products_host(z, ts, sps)))
        out[ts] = ((r[:, 0] == OFFSETS[A]).astype(np.uint8) + (r[:, 1] == OFFSETS[B]) + ((r[:, 2] == OFFSETS[CC]) | (r[:, 2] == OFFSETS[CP])) +
                   (r[:, 3] == OFFSETS[D]))
    return out


def masks_host(b, sps, clean=3):
    """the mask byte of every start: score << 1 | (score >= clean)"""
    s = scores_host(b, sps)
    return (s << 1 | (s >= clean)).astype(np.uint8)


def candidates_host(b, sps, clean=3):
    """the ordered starts with at least `clean` clean blocks, int64"""
    return np.flatnonzero(scores_host(b, sps) >= clean).astype(np.int64)


def _empty_det(m=0):
    return {"t": np.zeros(m, np.int64), "words": np.zeros((m, 4), np.uint16), "status": np.full((m, 4), -1, np.int32),
            "third": np.zeros(m, np.int32), "metric": np.zeros(m, np.int32), "state": np.full(m, OUTSIDE, np.int32),
            "good": np.zeros(m, np.int32)}


def groups_host(b, sps, fix, ts):
    """the listed starts' groups: a dict of t, words uint16[n, 4], status int32[n, 4] (0 clean, n bits repaired, -1 not decodable),
    third (0: C, 1: C'), metric, state (OK, OUTSIDE), good (blocks decoded)"""
    b = np.asarray(b, dtype=np.int64).reshape(-1, 2)
    ts = np.asarray(ts, dtype=np.int64).reshape(-1)
    det = _empty_det(len(ts))
    det["t"] = ts
    idx = np.flatnonzero(fits(ts, sps, len(b)))
    if not len(idx):
        return det
    prod = products_host(halfbit_host(b, int(sps // 2)), ts[idx], sps)
    blocks = blocks_host(prod)
    det["metric"][idx] = np.minimum(np.abs(prod) >> METRIC_SHIFT, METRIC_CAP).sum(axis=1)
    det["state"][idx] = OK
    rem = remainder(blocks)
    for r, i in enumerate(idx):
        w, st = [0] * 4, [0] * 4
        w[0], st[0] = repair_np(blocks[r, 0], A, fix)
        w[1], st[1] = repair_np(blocks[r, 1], B, fix)
        third = (w[1] >> 21) & 1 if st[1] >= 0 else int(rem[r, 2] == OFFSETS[CP])
        w[2], st[2] = repair_np(blocks[r, 2], CP if third else CC, fix)
        w[3], st[3] = repair_np(blocks[r, 3], D, fix)
        det["words"][i] = [v >> 10 for v in w]
        det["status"][i] = st
        det["third"][i] = third
        det["good"][i] = sum(1 for s in st if s >= 0)
    return det


# ------------------------------------------------------------------------------------------------------------------ the device stages
@functools.lru_cache(maxsize=None)
def table_device():
    """the phasor table on the device, int32[2048], uploaded once"""
    return DevArray.from_host(np.ascontiguousarray(table()).ravel())


def baseband(mpx, d, step, n0=0):
    """float64 device multiplex -> the baseband as a device int32 array of n // d pairs (dd_rds_baseband)"""
    need(mpx, _F64, "rds.baseband")
    nout = mpx.n // int(d)
    b = DevArray(max(2 * nout, 2), np.int32)
    check(lib().dd_rds_baseband(mpx.ptr, mpx.n, int(d), int(n0) & 0xFFFFFFFFFFFFFFFF, int(step), table_device().ptr, b.ptr, None),
          "dd_rds_baseband")
    return b.view(0, 2 * nout)


def capacity(m):
    """the default list capacity: a clean group passes at about half of its bit's starts; 1024 and a share of the data"""
    return 1024 + int(m) // 256


def candidates(b, m, sps, clean=3, cap=None):
    """device baseband of m pairs -> (the survivors as a device int64 array, how many) (dd_rds_candidates); a list that proves too
    small is asked for again at the true count"""
    need(b, _I32, "rds.candidates")
    cap = capacity(m) if cap is None else int(cap)
    def call(lst, cap, count):
        return lib().dd_rds_candidates(b.ptr, int(m), float(sps), int(clean), lst, cap, count, None)
    return _burst.candidates("dd_rds_candidates", cap, call)


def groups(b, m, sps, fix, lst, count):
    """the first `count` starts of the device list -> the dict of groups_host, on the host (dd_rds_groups)"""
    need(b, _I32, "rds.groups")
    if not isinstance(lst, DevArray):
        lst = DevArray.from_host(np.ascontiguousarray(lst, dtype=np.int64)) if count else None
    det = _empty_det(count)
    if count == 0:
        return det
    words, meta = DevArray(4 * count, np.uint16), DevArray(8 * count, np.int32)
    check(lib().dd_rds_groups(b.ptr, int(m), float(sps), int(fix), lst.ptr, count, words.ptr, meta.ptr, None), "dd_rds_groups")
    meta = meta.to_host().reshape(count, 8)
    det.update(t=lst.view(0, count).to_host(), words=words.to_host().reshape(count, 4), status=meta[:, 0:4].copy(), third=meta[:, 4].copy(),
               metric=meta[:, 5].copy(), state=meta[:, 6].copy(), good=meta[:, 7].copy())
    return det


def masks_device(b, m, sps, clean=3):
    """the mask byte of every start, uint8[m] on the host (dd_debug_rds_masks, a diagnostic)"""
    need(b, _I32, "rds.masks_device")
    return _burst.masks("dd_debug_rds_masks", m,
                        lambda mask: lib().dd_debug_rds_masks(b.ptr, int(m), float(sps), int(clean), mask, None))


def halfbit_device(b, m, sps):
    """z as int32[m, 2] on the host (dd_debug_rds_halfbit, a diagnostic)"""
    need(b, _I32, "rds.halfbit_device")
    z = DevArray(max(2 * m, 2), np.int32)
    check(lib().dd_debug_rds_halfbit(b.ptr, int(m), float(sps), z.ptr, None), "dd_debug_rds_halfbit")
    return z.to_host()[:2 * m].reshape(m, 2)


def repair_device(words, offs, fix):
    """26-bit words and offset indices -> (blocks uint32, status int32) by the device's wave (dd_debug_rds_repair, a diagnostic)"""
    words = np.ascontiguousarray(words, dtype=np.uint32).ravel()
    offs = np.ascontiguousarray(offs, dtype=np.int32).ravel()
    n = len(words)
    if n == 0:
        return words.copy(), np.zeros(0, np.int32)
    w, o, fixed, status = DevArray.from_host(words), DevArray.from_host(offs), DevArray(n, np.uint32), DevArray(n, np.int32)
    check(lib().dd_debug_rds_repair(w.ptr, o.ptr, n, int(fix), fixed.ptr, status.ptr, None), "dd_debug_rds_repair")
    return fixed.to_host(), status.to_host()


class HostOps(Laps):
    """the stages of `decode` in NumPy"""

    def baseband(self, mpx, d, step):
        b = baseband_host(mpx, d, step)
        return b, len(b)

    def detect(self, b, m, sps, clean, fix):
        return groups_host(b, sps, fix, candidates_host(b, sps, clean))

    def groups(self, b, m, sps, fix, ts):
        return groups_host(b, sps, fix, ts)


class DeviceOps(Laps):
    """the stages of `decode` on the device; `laps` collects seconds per stage, with a synchronisation after each"""

    def baseband(self, mpx, d, step):
        b = baseband(mpx, d, step)
        self.lap("baseband")
        return b, b.n // 2

    def detect(self, b, m, sps, clean, fix):
        lst, count = candidates(b, m, sps, clean)
        self.lap("candidates")
        det = groups(b, m, sps, fix, lst, count)
        self.lap("groups")
        return det

    def groups(self, b, m, sps, fix, ts):
        det = groups(b, m, sps, fix, ts, len(ts))
        self.lap("groups")
        return det


# ------------------------------------------------------------------------------------------------------------------ the parser
def char(c):
    """0x20 .. 0x7E as ASCII, the rest as U+FFFD"""
    return chr(c) if 0x20 <= c <= 0x7E else "�"


def mjd_date(mjd):
    """(year, month, day) of a modified Julian day by the standard's formula (valid from 1900-03-01 to 2100-02-28)"""
    y = int((mjd - 15078.2) / 365.25)
    mo = int((mjd - 14956.1 - int(y * 365.25)) / 30.6001)
    d = mjd - 14956 - int(y * 365.25) - int(mo * 30.6001)
    k = 1 if mo in (14, 15) else 0
    return 1900 + y + k, mo - 1 - 12 * k, d


def clock_of(w1, w2, w3):
    """the three words of a 4A group -> {"utc": ISO, "offset": half hours, "mjd": ...} or None when hour or minute is out of range"""
    mjd = (w1 & 3) << 15 | w2 >> 1
    hour, minute = (w2 & 1) << 4 | w3 >> 12, w3 >> 6 & 63
    if hour > 23 or minute > 59:
        return None
    off = w3 & 31
    y, mo, d = mjd_date(mjd)
    return {"utc": "%04d-%02d-%02dT%02d:%02d:00Z" % (y, mo, d, hour, minute), "offset": -off if w3 >> 5 & 1 else off, "mjd": mjd}


def af_of(code):
    """an alternative frequency code of method A: ("freq", MHz) for 1 .. 204, ("count", n) for 225 .. 249, else None (205 is filler)"""
    if 1 <= code <= 204:
        return "freq", round(87.5 + 0.1 * code, 1)
    if 225 <= code <= 249:
        return "count", code - 224
    return None


def fields(words, third):
    """(pi, group, tp, pty) of a group's words (None where not decoded); the PI is block 1's, or block 3's of a version B group"""
    w0, w1, w2, _ = words
    pi = w0 if w0 is not None else (w2 if third == 1 and w2 is not None else None)
    if w1 is None:
        return pi, None, None, None
    return pi, "%d%s" % (w1 >> 12, "AB"[w1 >> 11 & 1]), w1 >> 10 & 1, w1 >> 5 & 31


def _station():
    return {"ps": [None] * 8, "rt": [None] * 64, "rt_flag": None, "pty": None, "tp": None, "ta": None, "ms": None, "di": [None] * 4,
            "af": [], "af_count": None, "clock": None, "groups": {}}


def assemble(found):
    """groups (with words, pi, group, tp, pty) in time order -> per PI the station's state (stations() makes it public).  A group
    whose PI was not decoded goes to the station of the last group before it that had one: a channel carries one station."""
    out, last = {}, None
    for g in found:
        last = g["pi"] if g["pi"] is not None else last
        if last is None:
            continue
        s = out.setdefault(last, _station())
        w0, w1, w2, w3 = g["words"]
        if w1 is None:
            continue
        s["groups"][g["group"]] = s["groups"].get(g["group"], 0) + 1
        s["tp"], s["pty"] = g["tp"], g["pty"]
        kind = g["group"]
        if kind in ("0A", "0B"):
            seg = w1 & 3
            s["ta"], s["ms"] = w1 >> 4 & 1, w1 >> 3 & 1
            s["di"][3 - seg] = w1 >> 2 & 1
            if w3 is not None:
                s["ps"][2 * seg], s["ps"][2 * seg + 1] = char(w3 >> 8), char(w3 & 255)
            if kind == "0A" and w2 is not None:
                for code in (w2 >> 8, w2 & 255):
                    af = af_of(code)
                    if af and af[0] == "count":
                        s["af_count"] = af[1]
                    elif af and af[1] not in s["af"]:
                        s["af"].append(af[1])
        elif kind in ("2A", "2B"):
            flag, seg = w1 >> 4 & 1, w1 & 15
            if s["rt_flag"] is not None and flag != s["rt_flag"]:
                s["rt"] = [None] * 64
            s["rt_flag"] = flag
            if kind == "2A":
                for j, w in ((0, w2), (2, w3)):
                    if w is not None:
                        s["rt"][4 * seg + j], s["rt"][4 * seg + j + 1] = w >> 8, w & 255
            elif w3 is not None:
                s["rt"][2 * seg], s["rt"][2 * seg + 1] = w3 >> 8, w3 & 255
        elif kind == "4A" and w2 is not None and w3 is not None:
            s["clock"] = clock_of(w1, w2, w3) or s["clock"]
    return out


def radiotext(rt):
    """the 64 places -> the text: up to the first 0x0D if one was received, undecoded places as spaces, trailing spaces dropped"""
    end = rt.index(0x0D) if 0x0D in rt else len(rt)
    return "".join(" " if c is None else char(c) for c in rt[:end]).rstrip(" ")


def stations(found):
    """getStations of a list of groups"""
    out = {}
    for pi, s in assemble(found).items():
        di = None if any(v is None for v in s["di"]) else sum(v << k for k, v in enumerate(s["di"]))
        out[pi] = {"ps": "".join(c or " " for c in s["ps"]), "ps_complete": all(c is not None for c in s["ps"]),
                   "radiotext": radiotext(s["rt"]), "pty": s["pty"], "tp": s["tp"], "ta": s["ta"], "ms": s["ms"], "di": di,
                   "af": list(s["af"]), "af_count": s["af_count"],
                   "clock": None if s["clock"] is None else (s["clock"]["utc"], s["clock"]["offset"]), "groups": dict(s["groups"])}
    return out


def text_lines(found):
    """getText: one line per station"""
    out = []
    for pi, s in sorted(stations(found).items()):
        line = "RDS %04X PS: '%s' RT: '%s'" % (pi, s["ps"], s["radiotext"])
        if s["clock"] is not None:
            line += " CT: %s %+.1f h" % (s["clock"][0], s["clock"][1] / 2.0)
        out.append(line)
    return out


# ------------------------------------------------------------------------------------------------------------------ the host logic
def _clean(det, i):
    return int((det["status"][i] == 0).sum())


def merge(det, sps):
    """The candidates -> (the kept indices in time order, how many duplicates were dropped): a run of candidates inside the data, each
    within one bit of the one before, is one group (a clean group passes around its best start and, weakly, some two thirds of a bit
    to either side of it; groups are 104 bits apart); the one with the most clean blocks stays, then the largest metric, then the
    earliest."""
    acc = sorted((int(i) for i in np.flatnonzero(det["state"] == OK)), key=lambda i: (int(det["t"][i]), i))
    t, clean, metric = det["t"].tolist(), (det["status"] == 0).sum(axis=1).tolist(), det["metric"].tolist()
    keep, dup, a = [], 0, 0
    while a < len(acc):
        e = a + 1
        while e < len(acc) and t[acc[e]] - t[acc[e - 1]] <= sps:
            e += 1
        keep.append(min(acc[a:e], key=lambda j: (-clean[j], -metric[j], t[j])))
        dup += e - a - 1
        a = e
    return keep, dup


def chain_tolerance(k, sps):
    """samples by which two starts k groups apart may miss k * 104 bits: half a bit and 200 ppm of the distance"""
    return 0.5 * sps + PPM * k * BITS * sps


def chained(ts, sps):
    """bool per start (ascending): another start lies k * 104 bits away, 1 <= k <= K_CHAIN, within chain_tolerance(k)"""
    ts = np.asarray(ts, dtype=np.float64)
    out = np.zeros(len(ts), dtype=bool)
    period = BITS * sps
    for i in range(len(ts)):
        d = ts[i + 1:] - ts[i]
        k = np.rint(d / period)
        hit = (k >= 1) & (k <= K_CHAIN) & (np.abs(d - k * period) <= chain_tolerance(k, sps))
        if hit.any():
            out[i] = True
            out[i + 1:] |= hit
    return out


def group_of(det, i, d, rate, followed=False):
    """candidate i as a group dict"""
    st = det["status"][i]
    words = [int(w) if s >= 0 else None for w, s in zip(det["words"][i], st)]
    third = int(det["third"][i])
    pi, kind, tp, pty = fields(words, third)
    t = int(det["t"][i])
    return {"t": t * d / float(rate), "start": t, "pi": pi, "group": kind, "tp": tp, "pty": pty, "words": words,
            "repaired": int(st[st > 0].sum()), "followed": followed, "third": third, "status": [int(s) for s in st],
            "metric": int(det["metric"][i])}


def decode(mpx, rate, clean=3, fix=2, follow=2, ops=None):
    """The chain behind decode_rds over the multiplex (a float64 device array for DeviceOps, NumPy for HostOps) at `rate` S/s ->
    (groups in time order, frameInfo, the candidates' dict).

    A candidate is accepted when another kept candidate lies a whole number of groups away (chained), or when all four of its
    blocks are clean.  Behind an accepted group up to `follow` groups in a row are taken at their predicted start, 104 bits on, where
    no kept candidate lies; such a group is accepted when at least two of its blocks decode."""
    ops = HostOps() if ops is None else ops
    check_options(clean, fix, follow)
    d, _, step = params(rate)
    b, m = ops.baseband(mpx, d, step)
    return decode_baseband(b, m, rate, clean, fix, follow, ops)


def decode_baseband(b, m, rate, clean=3, fix=2, follow=2, ops=None):
    """`decode` from the baseband on: b holds m pairs (a device int32 array for DeviceOps, int32[m, 2] for HostOps)"""
    ops = HostOps() if ops is None else ops
    check_options(clean, fix, follow)
    d, sps, _ = params(rate)
    det = ops.detect(b, m, sps, clean, fix)
    keep, dup = merge(det, sps)
    link = chained([int(det["t"][i]) for i in keep], sps)
    good = [i for i, c in zip(keep, link) if c or _clean(det, i) == 4]
    found = [group_of(det, i, d, rate) for i in good]
    info = {"samples": m, "candidates": len(det["t"]), "duplicates": dup, "dropped": len(keep) - len(good), "followed": 0}
    ops.lap("host")
    period = BITS * sps
    tails = [(g, 0) for g in found]
    starts = sorted(g["start"] for g in found)

    def kept_near(at):
        i = bisect.bisect_left(starts, at - sps)
        return i < len(starts) and starts[i] <= at + sps
    while follow and tails:
        ask = []
        for g, run in tails:
            at = int(math.floor(g["start"] + period + 0.5))
            if run < follow and not kept_near(at) and bool(fits([at], sps, m)[0]):
                ask.append((at, run))
        ask = sorted(set(ask))
        if not ask:
            break
        ops.lap("host")
        dd = ops.groups(b, m, sps, fix, np.array([a for a, _ in ask], dtype=np.int64))
        tails = []
        for j, (at, run) in enumerate(ask):
            if dd["state"][j] == OK and dd["good"][j] >= 2 and not kept_near(at):
                g = group_of(dd, j, d, rate, True)
                found.append(g)
                bisect.insort(starts, g["start"])
                tails.append((g, run + 1))
                info["followed"] += 1
        ops.lap("host")
    found.sort(key=lambda g: g["start"])
    info["groups"] = len(found)
    info["repaired"] = sum(1 for g in found if g["repaired"])
    return found, info, det


# ------------------------------------------------------------------------------------------------------------------ the synthesiser
def group_0a(pi, ps, seg, tp=0, pty=0, ta=0, ms=1, di=0, af=(FILLER, FILLER), version="A"):
    """the four words of a 0A (or 0B) group: segment `seg` (0 .. 3) of the eight-character name `ps`, bit 3 - seg of `di`, two AF codes
    (0B: the PI again)"""
    ps = ps.ljust(8)[:8].encode("ascii")
    w1 = (0x0800 if version == "B" else 0) | tp << 10 | pty << 5 | ta << 4 | ms << 3 | (di >> (3 - seg) & 1) << 2 | seg
    w2 = pi if version == "B" else af[0] << 8 | af[1]
    return pi, w1, w2, ps[2 * seg] << 8 | ps[2 * seg + 1]


def group_2a(pi, text, seg, flag=0, tp=0, pty=0, version="A"):
    """the four words of a 2A group: characters 4 seg .. 4 seg + 3 of `text` (2B: 2 seg, 2 seg + 1 in block 4, the PI in block 3);
    the text is padded with spaces, put a "\\r" where it ends"""
    w1 = 2 << 12 | (0x0800 if version == "B" else 0) | tp << 10 | pty << 5 | flag << 4 | seg
    if version == "B":
        c = text.ljust(32)[:32].encode("ascii")
        return pi, w1, pi, c[2 * seg] << 8 | c[2 * seg + 1]
    c = text.ljust(64)[:64].encode("ascii")
    return pi, w1, c[4 * seg] << 8 | c[4 * seg + 1], c[4 * seg + 2] << 8 | c[4 * seg + 3]


def group_4a(pi, mjd, hour, minute, offset=0, tp=0, pty=0):
    """the four words of a 4A group: the modified Julian day, UTC hour and minute, the local offset in half hours (signed)"""
    w1 = 4 << 12 | tp << 10 | pty << 5 | mjd >> 15 & 3
    w2 = (mjd & 0x7FFF) << 1 | hour >> 4 & 1
    w3 = (hour & 15) << 12 | minute << 6 | (1 << 5 if offset < 0 else 0) | abs(offset) & 31
    return pi, w1, w2, w3


def group_blocks(words):
    """four information words -> the four 26-bit blocks: offset words A, B, C (C' when bit 11 of the second word says version B), D"""
    third = CP if words[1] >> 11 & 1 else CC
    return [block(w, o) for w, o in zip(words, (A, B, third, D))]


def air_bits(groups):
    """groups (four words each) -> the bits in the order sent, uint8[104 n]"""
    out = []
    for g in groups:
        for blk in group_blocks(g):
            out.extend(blk >> i & 1 for i in range(25, -1, -1))
    return np.array(out, dtype=np.uint8)


def _pulse(rate, reach=4.0):
    """the shaping pulse at `rate` S/s, whose spectrum is cos(pi f T / 4) up to 2 / T: two sincs T / 4 apart, cut `reach` bits
    either way and faded out by a Hann window"""
    T = 1.0 / BITRATE
    half = int(math.ceil(reach * T * rate))
    t = np.arange(-half, half + 1) / rate
    h = np.sinc(4.0 * (t + T / 8.0) / T) + np.sinc(4.0 * (t - T / 8.0) / T)
    return h * np.hanning(len(h) + 2)[1:-1]


def symbols(bits, rate, n, start=0.0, clock_ppm=0.0):
    """float64[n]: the shaped biphase signal of the bits, differentially coded, bit k's impulse pair at the transmitter's times
    start + k T and start + (k + 1/2) T seconds; a receiver clock `clock_ppm` fast sees the times stretched.  Peak about 1."""
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    level = 2.0 * (np.cumsum(bits) & 1) - 1.0                         # d_k = d_(k-1) XOR bit_k from d_-1 = 0
    T = 1.0 / BITRATE
    x = np.zeros(n + 2)
    scale = rate * (1.0 + clock_ppm * 1e-6)
    for sign, shift in ((1.0, 0.0), (-1.0, 0.5)):
        at = (start + (np.arange(len(bits)) + shift) * T) * scale
        i = np.floor(at).astype(np.int64)
        f = at - i
        ok = (i >= 0) & (i < n)
        np.add.at(x, i[ok], sign * level[ok] * (1.0 - f[ok]))
        np.add.at(x, i[ok] + 1, sign * level[ok] * f[ok])
    h = _pulse(rate)
    half = len(h) // 2
    pair = h[int(round(0.5 * T * rate)):] - h[:len(h) - int(round(0.5 * T * rate))]
    h = h / np.abs(pair).max()
    size = 1 << int(math.ceil(math.log2(n + 2 + len(h))))
    y = np.fft.irfft(np.fft.rfft(x, size) * np.fft.rfft(h, size), size)
    return y[half:half + n]


def stream_length(count, rate, start=0.0, tail=0.002):
    """samples that hold `count` groups from `start` seconds on and `tail` seconds more"""
    return int(math.ceil((start + count * BITS / BITRATE + tail) * rate)) + 1


def multiplex(groups, rate, n=None, phase=0.0, level=0.04, pilot=0.09, tone=0.3, tone_hz=1000.0, start=0.0, clock_ppm=0.0):
    """float64[n]: the multiplex as a fraction of the peak deviation: a tone, the 19 kHz pilot and the RDS signal on 57 kHz, `phase`
    radians against three times the pilot.  groups: four words each, or the bits themselves as a uint8 array (which lets a test damage
    them).  clock_ppm: the receiver's sample clock error, which moves every frequency and the bit rate alike."""
    bits = groups if isinstance(groups, np.ndarray) else air_bits(groups)
    n = stream_length(len(bits) // BITS + (1 if len(bits) % BITS else 0), rate, start) if n is None else int(n)
    tau = np.arange(n) / (rate * (1.0 + clock_ppm * 1e-6))
    s = symbols(bits, rate, n, start, clock_ppm) if level else 0.0
    return (tone * np.sin(2.0 * np.pi * tone_hz * tau) + pilot * np.sin(2.0 * np.pi * PILOT * tau) +
            level * s * np.sin(3.0 * 2.0 * np.pi * PILOT * tau + phase))


def encode_mpx(groups, rate, sigma=0.0, seed=0, deviation=DEVIATION, **kw):
    """The discriminator's view of a station: float64[n] in radians per sample, 2 pi deviation * multiplex / rate, plus Gaussian
    noise of `sigma` radians; the keywords of `multiplex`"""
    x = 2.0 * np.pi * deviation / rate * multiplex(groups, rate, **kw)
    if sigma:
        x = x + np.random.default_rng(seed).normal(0.0, sigma, len(x))
    return x


def encode(groups, rate, offset=0.0, amplitude=60.0, sigma=0.0, seed=0, carrier_ppm=0.0, carrier=100e6, deviation=DEVIATION, **kw):
    """A recording uint8[n, 2] at `rate` S/s with the station `offset` Hz from the centre, frequency modulated at 75 kHz deviation by
    `multiplex` (its keywords; clock_ppm is the sample clock's error), its carrier `carrier_ppm` of `carrier` Hz off; Gaussian noise
    of `sigma` per rail; the u8 value is clip(rint(z + 127.5), 0, 255)"""
    mpx = multiplex(groups, rate, **kw)
    rng = np.random.default_rng(seed)
    f = deviation * mpx + offset + carrier_ppm * 1e-6 * carrier
    phase = rng.uniform(0.0, 2.0 * np.pi) + 2.0 * np.pi * np.cumsum(f) / rate
    z = amplitude * np.exp(1j * phase)
    v = np.stack((z.real, z.imag), axis=1) + 127.5
    if sigma:
        v = v + rng.normal(0.0, 1.0, v.shape) * sigma
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ the front end, restated
def audio_host(raw, fs, offset, bw=240000.0, taps=None):
    """(float64 multiplex, its rate) of the station at `offset` Hz of a uint8[N, 2] recording in float64 NumPy: decode_rds's front
    end restated (the mixer, the Blackman-Harris window of window_taps(fs) taps started over ones, every int(fs / bw)-th sample, the
    discriminator).  The device's float32 stages round differently: this is the same chain, not the same bits."""
    from . import filters
    a = np.asarray(raw, dtype=np.uint8).reshape(-1, 2).astype(np.float64) - 127.5
    x = (a[:, 0] + 1j * a[:, 1]) * np.exp(-2j * np.pi * offset * np.arange(len(a)) / float(fs))
    K = window_taps(fs) if taps is None else int(taps)                 # (taps: tools/sens_rds.py compares window lengths)
    bh = filters._cosine_sum(K, [0.35875, 0.48829, 0.14128, 0.01168])
    y = np.convolve(np.concatenate((np.ones(K - 1), x)), bh)[K - 1:K - 1 + len(x)]
    step = int(fs / bw)
    y = y[::step]
    return np.angle(y[1:] * np.conj(y[:-1])), fs / step
