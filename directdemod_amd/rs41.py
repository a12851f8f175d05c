"""
Vaisala RS41 radiosonde telemetry: 2-GFSK at 4800 baud, one frame of 320 or 518 bytes per second behind a 64-bit header, whitened
with a 64-byte mask, protected by two interleaved RS(255,231) codewords and a CRC-16 per block (beyond the reference; DESIGN.md
section 4.26 defines every stage; device side: dd_rs41.h): the constants, the Reed-Solomon code, a NumPy restatement `masks_host` /
`candidates_host` / `frames_host` of the two kernels and `rs_decode_np` of the Reed-Solomon wave, the device wrappers over the C
entries, `decode`, the chain behind decode_rs41, which runs over either set of stages (`DeviceOps`, `HostOps`) so that the host logic
is one piece of code for both, the merge, the block parser, the positions, and `encode` / `encode_iq`, a synthesiser.

The audio is the FM discriminator's output in radians per sample, quantised, positioned and summed as for AIS (ais.quantise,
ais.positions, ais.values): bit k of the start t is read around sample floor(t + (k + 0.5) sps), v(t, k) is the sum of the w samples
q around it.  The header has 25 ones and 39 zeros, so its mean is no threshold: with S1 the sum of v over the one-places and S0 over
the zero-places, a value is high when 1950 v > 39 S1 + 25 S0 and low when 1950 v < 39 S1 + 25 S0, the midpoint of the two classes'
means.  Polarity 0 reads high as 1, polarity 1 reads low as 1.  A byte holds its first-sent bit in bit 0.

The format is taken from public descriptions of the RS41 and has been met in synthesised recordings only; INTEGRATION.md lists the
limits.
"""
import datetime
import functools
import math

import numpy as np

from . import _burst
from ._burst import Laps, need
from ._hip import DevArray, check, lib
from .ais import positions, quantise, values  # noqa: F401  (the same quantiser, positions and window sums)

BAUD = 4800
SPS_MIN, SPS_MAX = 4.0, 64.0
W_MAX = 39                            # DD_RS41_W_MAX
HEADER_DISTANCE = 24                  # the header slid into its preamble differs from itself and its inverse in this many places or more
SLACK_MAX = (HEADER_DISTANCE - 1) // 2    # 11, DD_RS41_SLACK_MAX: a slid header with `slack` errors of its own still fails
TILE = 256                            # DD_RS41_TILE
HEADER = bytes.fromhex("10B6CA11229612F8")            # on the air
HEADER_CLEAR = bytes.fromhex("8635F44093DF1A60")      # de-whitened
MASK = np.frombuffer(bytes.fromhex(
    "96833E51B14908983205590EF944C6262160C2EA795D6DA15469470CDCE85CF1F776827F0799A22C937C3063F5102E61D0BCB4B606AAF423786E3BAEBF7B4CC1"),
    dtype=np.uint8)
HEADER_BITS = np.unpackbits(np.frombuffer(HEADER, dtype=np.uint8), bitorder="little").astype(bool)   # first sent first
ONES, ZEROS = 25, 39
STD, EXT = 320, 518                   # bytes of a standard and of an extended frame
TYPE_AT = 56
TYPE_STD, TYPE_EXT = 0x0F, 0xF0
PARITY_AT = 8
DATA_AT = 56
RS_N, RS_T = 255, 12
RS_POLY = 0x11D
OK, OUTSIDE = 0, 1
PREAMBLE_BITS = 320
DEVIATION = 2400.0
CUT = 3600.0                          # the audio-rate channel filter's cut-off, Hz (tools/sens_rs41.py)
BLOCK_STATUS, BLOCK_MEAS, BLOCK_GPSINFO, BLOCK_GPSRAW, BLOCK_GPSPOS, BLOCK_EMPTY, BLOCK_XDATA = 0x79, 0x7A, 0x7C, 0x7D, 0x7B, 0x76, 0x7E
LAYOUT = ((0x039, 0x79, 0x28), (0x065, 0x7A, 0x2A), (0x093, 0x7C, 0x1E), (0x0B5, 0x7D, 0x59), (0x112, 0x7B, 0x15), (0x12B, 0x76, 0x11))
SUBFRAMES = 51
WGS84_A, WGS84_F = 6378137.0, 1.0 / 298.257223563
WGS84_E2 = WGS84_F * (2.0 - WGS84_F)
GPS_EPOCH = datetime.datetime(1980, 1, 6)

_F64 = np.dtype(np.float64)


def params(rate, w=None, slack=4):
    """(sps, w, slack) for an audio rate: sps = rate / 4800 must lie in 4 .. 64; w None: the odd number nearest 0.6 sps"""
    sps = float(rate) / BAUD if rate and rate > 0 else float("nan")
    if not SPS_MIN <= sps <= SPS_MAX:              # (also false for a NaN)
        raise ValueError("rs41: an audio rate of %r S/s is %r samples per bit; %g to %g are supported" % (rate, sps, SPS_MIN, SPS_MAX))
    if w is None:
        w = min(W_MAX, 2 * int(math.floor((0.6 * sps - 1.0) / 2.0 + 0.5)) + 1)
    if int(w) != w or not 1 <= w <= W_MAX or not int(w) & 1:
        raise ValueError("rs41: w must be an odd number from 1 to %d, got %r" % (W_MAX, w))
    if int(slack) != slack or not 0 <= slack <= SLACK_MAX:
        raise ValueError("rs41: slack must be from 0 to %d, got %r" % (SLACK_MAX, slack))
    return sps, int(w), int(slack)


def reach(sps, w):
    """samples from a start to past the last one its header reads"""
    return int(math.floor(63.5 * sps)) + w // 2 + 1


def n_starts(n, sps, w):
    return max(0, int(n) - reach(sps, w) + 1)


def slide_distance(preamble=PREAMBLE_BITS):
    """the least number of places in which the header differs from a window of 64 bits that lies 1 .. `preamble` bits before it in
    alternating bits (of either phase) + header, or from that window's inverse: what SLACK_MAX follows from"""
    best = 64
    for phase in (0, 1):
        seq = np.concatenate((((np.arange(preamble) + phase) & 1).astype(bool), HEADER_BITS))
        for s in range(1, preamble + 1):
            d = int((seq[preamble - s:preamble - s + 64] != HEADER_BITS).sum())
            best = min(best, d, 64 - d)
    return best


def crc16(data):
    """CRC-16, polynomial 0x1021, preset 0xFFFF, not reflected"""
    c = 0xFFFF
    for v in bytes(data):
        c ^= v << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x1021) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


# ------------------------------------------------------------------------------------------------------------------ Reed-Solomon
@functools.lru_cache(maxsize=None)
def gf_tables():
    """(exp uint8[512], log int16[256]) of GF(2)[x] / 0x11D, alpha = 2: exp[log[a] + log[b]] is a * b for non-zero a, b"""
    ex, lg = np.zeros(512, dtype=np.uint8), np.zeros(256, dtype=np.int16)
    v = 1
    for i in range(255):
        ex[i], lg[v] = v, i
        v <<= 1
        if v & 0x100:
            v ^= RS_POLY
    ex[255:510], ex[510:] = ex[:255], ex[:2]
    ex.setflags(write=False)
    lg.setflags(write=False)
    return ex, lg


def gf_mul(a, b):
    ex, lg = gf_tables()
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    return np.where((a == 0) | (b == 0), 0, ex[lg[a] + lg[b]]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def rs_generator():
    """g(x) = prod over j = 0 .. 23 of (x - alpha^j), uint8[25], low to high coefficient"""
    ex, _ = gf_tables()
    g = np.array([1], dtype=np.uint8)
    for j in range(2 * RS_T):
        g = np.concatenate(([0], g)).astype(np.uint8) ^ np.concatenate((gf_mul(g, ex[j]), [0])).astype(np.uint8)
    g.setflags(write=False)
    return g


def rs_encode(data):
    """data uint8[..., 231], the coefficients of x^254 .. x^24 -> codewords uint8[..., 255] in the decoder's order (byte i is the
    coefficient of x^(254 - i)): the data, then the remainder of data(x) x^24 modulo g(x)"""
    data = np.asarray(data, dtype=np.uint8)
    if data.shape[-1] != RS_N - 2 * RS_T:
        raise ValueError("rs41.rs_encode: 231 data bytes per word")
    taps = rs_generator()[2 * RS_T - 1::-1]
    reg = np.zeros(data.shape[:-1] + (2 * RS_T,), dtype=np.uint8)
    for i in range(data.shape[-1]):
        fb = data[..., i] ^ reg[..., 0]
        reg = np.concatenate((reg[..., 1:], np.zeros_like(reg[..., :1])), axis=-1) ^ gf_mul(fb[..., None], taps)
    return np.concatenate((data, reg), axis=-1)


def rs_syndromes(words):
    """words uint8[..., 255] -> uint8[..., 24]: S_j = c(alpha^j) with byte i the coefficient of x^(254 - i)"""
    ex, lg = gf_tables()
    words = np.asarray(words, dtype=np.uint8)
    if words.shape[-1] != RS_N:
        raise ValueError("rs41.rs_syndromes: 255 bytes per word")
    lr = np.arange(2 * RS_T, dtype=np.int16)
    acc = np.zeros(words.shape[:-1] + (2 * RS_T,), dtype=np.uint8)
    for i in range(RS_N):
        acc = np.where(acc == 0, 0, ex[lg[acc] + lr]).astype(np.uint8) ^ words[..., i, None]
    return acc


def _poly_at(coef, lx):
    """sum of coef[k] * alpha^(k lx[p]) over k, for every p: uint8[len(lx)]"""
    ex, lg = gf_tables()
    coef = np.asarray(coef, dtype=np.uint8)
    k = np.arange(len(coef), dtype=np.int64)[:, None]
    terms = np.where(coef[:, None] == 0, 0, ex[(lg[coef].astype(np.int64)[:, None] + k * lx[None, :]) % 255])
    return np.bitwise_xor.reduce(terms.astype(np.uint8), axis=0)


def _rs_correction(S, first_valid):
    """syndromes uint8[24], not all zero -> (positions, values) of the error pattern Berlekamp-Massey, a search of the 255 positions
    and Forney's formula propose, or None when they propose none: a locator of degree > 12, fewer roots than its degree, a zero
    value, a position below first_valid.  The caller checks the corrected word's syndromes."""
    ex, lg = (t.tolist() for t in gf_tables())
    S = [int(v) for v in S]
    top = 2 * RS_T + 1

    def mul(a, b):
        return ex[lg[a] + lg[b]] if a and b else 0
    Cc, B, L, m, b = [1] + [0] * (top - 1), [1] + [0] * (top - 1), 0, 1, 1
    for n in range(2 * RS_T):
        d = S[n]
        for i in range(1, L + 1):
            d ^= mul(Cc[i], S[n - i])
        if d == 0:
            m += 1
            continue
        coef = ex[lg[d] + 255 - lg[b]]
        was = Cc[:]
        for i in range(m, top):
            Cc[i] ^= mul(coef, B[i - m])
        if 2 * L <= n:
            L, B, b, m = n + 1 - L, was, d, 1
        else:
            m += 1
    if L > RS_T or max(i for i in range(top) if Cc[i]) != L:
        return None
    lam = Cc[:RS_T + 1]
    lX = (254 - np.arange(RS_N, dtype=np.int64)) % 255                          # position i has locator X = alpha^(254 - i)
    lx = (255 - lX) % 255                                                      # X^-1
    pos = np.nonzero(_poly_at(lam, lx) == 0)[0]
    if len(pos) != L or np.any(pos < first_valid):
        return None
    omega = [0] * RS_T                                                         # S Lambda mod x^24 has degree < L <= 12
    for k in range(RS_T):
        for i in range(k + 1):
            omega[k] ^= mul(lam[i], S[k - i])
    deriv = [lam[i + 1] if i % 2 == 0 else 0 for i in range(RS_T)]              # Lambda'(x): the odd terms, one degree down
    num, den = _poly_at(omega, lx[pos]), _poly_at(deriv, lx[pos])
    if np.any(num == 0) or np.any(den == 0):
        return None
    glog = gf_tables()[1]
    val = gf_tables()[0][(glog[num].astype(np.int64) - glog[den] + lX[pos]) % 255]      # the first root is alpha^0: X^(1 - 0)
    return pos, val


def rs_decode_np(words, first_valid=0):
    """words uint8[..., 255] -> (fixed uint8[..., 255], errors int32[...]): the codeword within Hamming distance 12 of each word
    that changes no byte below position first_valid, and how many bytes it changes, or the word itself and -1 where there is none"""
    words = np.asarray(words, dtype=np.uint8)
    if words.shape[-1] != RS_N:
        raise ValueError("rs41.rs_decode_np: 255 bytes per word")
    flat = words.reshape(-1, RS_N)
    fixed = flat.copy()
    errors = np.zeros(len(flat), dtype=np.int32)
    syn = rs_syndromes(flat)
    tried = []
    for i in np.nonzero(syn.any(axis=1))[0]:
        fix = _rs_correction(syn[i], first_valid)
        if fix is None:
            errors[i] = -1
        else:
            fixed[i, fix[0]] ^= fix[1]
            errors[i] = len(fix[0])
            tried.append(i)
    if tried:
        tried = np.array(tried)
        bad = tried[rs_syndromes(fixed[tried]).any(axis=1)]
        fixed[bad] = flat[bad]
        errors[bad] = -1
    return fixed.reshape(words.shape), errors.reshape(words.shape[:-1])


def message_count(length):
    """message bytes per codeword of a frame of `length` bytes: 132 or 231"""
    return (length - DATA_AT) // 2


def _where(length):
    """int64[2, 255]: the frame's byte behind position i of codeword j, -1 where the frame has ended (the shortened part)"""
    p = 254 - np.arange(RS_N)
    out = np.full((2, RS_N), -1, dtype=np.int64)
    for j in range(2):
        out[j] = np.where(p < 2 * RS_T, PARITY_AT + 2 * RS_T * j + p,
                          np.where(p - 2 * RS_T < message_count(length), DATA_AT + 2 * (p - 2 * RS_T) + j, -1))
    return out


def codewords(frame, length):
    """frame uint8[>= length] -> uint8[2, 255]: the two codewords in the decoder's order, zero in the shortened part"""
    at = _where(length)
    f = np.asarray(frame, dtype=np.uint8)
    return np.where(at >= 0, f[np.maximum(at, 0)], 0).astype(np.uint8)


def first_valid(length):
    return RS_N - 2 * RS_T - message_count(length)


def add_parity(frame, length):
    """the frame with bytes 8 .. 55 set to its two codewords' parity"""
    f = np.array(frame, dtype=np.uint8)
    at = _where(length)
    cw = rs_encode(codewords(f, length)[:, :RS_N - 2 * RS_T])
    f[at[:, RS_N - 2 * RS_T:]] = cw[:, RS_N - 2 * RS_T:]
    return f


# ------------------------------------------------------------------------------------------------------------------ the restatement
def header_of(q, ts, sps, w):
    """(c int64[m, 64] = 1950 v, mid int64[m] = 39 S1 + 25 S0) of the starts ts"""
    v = values(q, ts, np.arange(64), sps, w)
    mid = ZEROS * v[:, HEADER_BITS].sum(axis=1) + ONES * v[:, ~HEADER_BITS].sum(axis=1)
    return 2 * ONES * ZEROS * v, mid


def masks_host(audio, sps, w, slack=4, block=1 << 13):
    """the mask byte of every start: bit 0 pass, bit 1 the other polarity; uint8[n_starts]"""
    q = quantise(audio)
    total = n_starts(len(q), sps, w)
    out = np.zeros(total, dtype=np.uint8)
    for a in range(0, total, block):
        ts = np.arange(a, min(total, a + block), dtype=np.int64)
        c, mid = header_of(q, ts, sps, w)
        mis0 = ((c > mid[:, None]) != HEADER_BITS).sum(axis=1)
        mis1 = ((c < mid[:, None]) != HEADER_BITS).sum(axis=1)
        out[a:a + len(ts)] = np.where(mis0 <= slack, 1, np.where(mis1 <= slack, 3, 0))
    return out


def candidates_host(audio, sps, w, slack=4):
    """the ordered starts that pass the header test, int64"""
    return np.flatnonzero(masks_host(audio, sps, w, slack) & 1).astype(np.int64)


def _empty_det(m=0):
    return {"t": np.zeros(m, np.int64), "fixed": np.zeros((m, EXT), np.uint8), "recv": np.zeros((m, EXT), np.uint8),
            "status": np.full(m, OUTSIDE, np.int32), "polarity": np.zeros(m, np.int32), "length": np.zeros(m, np.int32),
            "mis": np.zeros(m, np.int32), "errs": np.zeros((m, 2), np.int32)}


def fits(ts, length, sps, w, n):
    return positions(ts, [8 * length - 1], sps)[:, 0] + w // 2 < n


def frames_host(audio, sps, w, ts):
    """the listed starts' frames: a dict of t, fixed uint8[m, 518], recv uint8[m, 518], status, polarity, length, mis, errs int32[m, 2]"""
    q = quantise(audio)
    n = len(q)
    ts = np.asarray(ts, dtype=np.int64).reshape(-1)
    det = _empty_det(len(ts))
    det["t"] = ts
    weights = (1 << np.arange(8)).astype(np.int64)
    white = np.tile(MASK, 9)[:EXT]
    inside = (ts >= 0) & (ts < n)
    inside[inside] = fits(ts[inside], STD, sps, w, n)
    for a in range(0, len(ts), 32):
        idx = a + np.flatnonzero(inside[a:a + 32])
        if not len(idx):
            continue
        v = values(q, ts[idx], np.arange(8 * EXT), sps, w)
        c = 2 * ONES * ZEROS * v
        mid = (ZEROS * v[:, :64][:, HEADER_BITS].sum(axis=1) + ONES * v[:, :64][:, ~HEADER_BITS].sum(axis=1)).reshape(-1, 1)
        mis0 = ((c[:, :64] > mid) != HEADER_BITS).sum(axis=1)
        mis1 = ((c[:, :64] < mid) != HEADER_BITS).sum(axis=1)
        inv = mis1 < mis0
        bits = np.where(inv.reshape(-1, 1), c < mid, c > mid)
        recv = ((bits.reshape(len(idx), EXT, 8) * weights).sum(axis=2) ^ white).astype(np.uint8)
        ty = recv[:, TYPE_AT].astype(np.int64)
        pop = lambda v: ((v[:, None] >> np.arange(8)) & 1).sum(axis=1)          # noqa: E731
        ext = (pop(ty ^ TYPE_EXT) < pop(ty ^ TYPE_STD)) & fits(ts[idx], EXT, sps, w, n)
        length = np.where(ext, EXT, STD)
        recv[np.arange(EXT)[None, :] >= length[:, None]] = 0
        fixed = recv.copy()
        for r, i in enumerate(idx):
            at = _where(int(length[r]))
            cw, errs = rs_decode_np(codewords(recv[r], int(length[r])), first_valid(int(length[r])))
            fixed[r, at[at >= 0]] = cw[at >= 0]
            det["errs"][i] = errs
        det["fixed"][idx], det["recv"][idx] = fixed, recv
        det["status"][idx], det["polarity"][idx], det["length"][idx] = OK, inv, length
        det["mis"][idx] = np.where(inv, mis1, mis0)
    return det


# ------------------------------------------------------------------------------------------------------------------ the device stages
def capacity(n, sps):
    """the default list capacity: a clean frame passes at about sps adjacent starts of its second; 1024 and a share of the audio"""
    return 1024 + int(n) // 512


def candidates(audio, sps, w, slack=4, cap=None):
    """float64 device audio -> (the survivors as a device int64 array, how many) (dd_rs41_candidates); a list that proves too small
    is asked for again at the true count"""
    need(audio, _F64, "rs41.candidates")
    cap = capacity(audio.n, sps) if cap is None else int(cap)
    def call(lst, cap, count):
        return lib().dd_rs41_candidates(audio.ptr, audio.n, float(sps), int(w), int(slack), lst, cap, count, None)
    return _burst.candidates("dd_rs41_candidates", cap, call)


def frames(audio, sps, w, lst, m):
    """the first m starts of the device list -> the dict of frames_host, on the host (dd_rs41_frames)"""
    need(audio, _F64, "rs41.frames")
    if not isinstance(lst, DevArray):
        lst = DevArray.from_host(np.ascontiguousarray(lst, dtype=np.int64))
    det = _empty_det(m)
    if m == 0 or audio.n == 0:
        return det
    fixed, recv, meta = DevArray(EXT * m, np.uint8), DevArray(EXT * m, np.uint8), DevArray(6 * m, np.int32)
    check(lib().dd_rs41_frames(audio.ptr, audio.n, float(sps), int(w), lst.ptr, m, fixed.ptr, recv.ptr, meta.ptr, None), "dd_rs41_frames")
    meta = meta.to_host().reshape(m, 6)
    det.update(t=lst.view(0, m).to_host(), fixed=fixed.to_host().reshape(m, EXT), recv=recv.to_host().reshape(m, EXT),
               status=meta[:, 0].copy(), polarity=meta[:, 1].copy(), length=meta[:, 2].copy(), mis=meta[:, 3].copy(), errs=meta[:, 4:6].copy())
    return det


def masks_device(audio, sps, w, slack=4):
    """the mask byte of every sample, uint8[n] on the host, 0 past the last start (dd_debug_rs41_masks, a diagnostic)"""
    need(audio, _F64, "rs41.masks_device")
    return _burst.masks("dd_debug_rs41_masks", audio.n,
                        lambda mask: lib().dd_debug_rs41_masks(audio.ptr, audio.n, float(sps), int(w), int(slack), mask, None))


def rs_device(words, first_valid=0):
    """words uint8[m, 255] -> (fixed uint8[m, 255], errors int32[m]) by the device's wave (dd_debug_rs41_rs, a diagnostic)"""
    words = np.ascontiguousarray(words, dtype=np.uint8).reshape(-1, RS_N)
    m = len(words)
    if m == 0:
        return words.copy(), np.zeros(0, np.int32)
    src, fixed, errors = DevArray.from_host(words.ravel()), DevArray(RS_N * m, np.uint8), DevArray(m, np.int32)
    check(lib().dd_debug_rs41_rs(src.ptr, m, int(first_valid), fixed.ptr, errors.ptr, None), "dd_debug_rs41_rs")
    return fixed.to_host().reshape(m, RS_N), errors.to_host()


class HostOps(Laps):
    """the stages of `decode` in NumPy"""

    def detect(self, audio, sps, w, slack):
        return frames_host(audio, sps, w, candidates_host(audio, sps, w, slack))

    def frames(self, audio, sps, w, ts):
        return frames_host(audio, sps, w, ts)


class DeviceOps(Laps):
    """the stages of `decode` on the device; `laps` collects seconds per stage, with a synchronisation after each"""

    def detect(self, audio, sps, w, slack):
        lst, m = candidates(audio, sps, w, slack)
        self.lap("candidates")
        det = frames(audio, sps, w, lst, m)
        self.lap("frames")
        return det

    def frames(self, audio, sps, w, ts):
        det = frames(audio, sps, w, ts, len(ts))
        self.lap("frames")
        return det


# ------------------------------------------------------------------------------------------------------------------ the parser
def blocks_of(frame, length, trusted):
    """The block chain from byte 57 on: a list of dicts id, at (the offset of the id byte), crc_ok, bytes (the data).  A chain is
    walked by its length bytes; where a block of an untrusted frame (Reed-Solomon failed) fails its CRC, the walk goes on at the
    standard layout's next offset, since the length byte itself may be the damage."""
    f = bytes(bytearray(np.asarray(frame, dtype=np.uint8)[:length]))
    out, at = [], TYPE_AT + 1
    while at + 4 <= length:
        ln = f[at + 1]
        good = at + ln + 4 <= length
        if good:
            data = f[at + 2:at + 2 + ln]
            good = crc16(data) == f[at + 2 + ln] | f[at + 3 + ln] << 8
            if good or trusted:
                out.append({"id": f[at], "at": at, "crc_ok": good, "bytes": data})
        if good or (trusted and at + ln + 4 <= length):
            at += ln + 4
            continue
        later = [o for o, _, _ in LAYOUT if o > at]
        if not later:
            break
        at = later[0]
    return out


def geodetic(x, y, z):
    """ECEF metres -> (latitude, longitude in degrees, height in metres) on WGS-84, float64: the latitude by fixed-point iteration
    on atan2(z, p (1 - e^2 N / (N + h))), the height as p cos(lat) + z sin(lat) - a sqrt(1 - e^2 sin^2(lat)), which keeps its
    precision at the poles"""
    x, y, z = float(x), float(y), float(z)
    p = math.hypot(x, y)
    lon = math.degrees(math.atan2(y, x)) if p > 0.0 else 0.0
    lat = math.atan2(z, p * (1.0 - WGS84_E2))
    for _ in range(8):
        s = math.sin(lat)
        N = WGS84_A / math.sqrt(1.0 - WGS84_E2 * s * s)
        h = p * math.cos(lat) + z * s - WGS84_A * math.sqrt(1.0 - WGS84_E2 * s * s)
        lat = math.atan2(z, p * (1.0 - WGS84_E2 * N / (N + h)))
    s = math.sin(lat)
    h = p * math.cos(lat) + z * s - WGS84_A * math.sqrt(1.0 - WGS84_E2 * s * s)
    return math.degrees(lat), lon, h


def ecef(lat, lon, alt):
    """WGS-84 degrees and metres -> ECEF metres"""
    la, lo = math.radians(lat), math.radians(lon)
    N = WGS84_A / math.sqrt(1.0 - WGS84_E2 * math.sin(la) ** 2)
    return ((N + alt) * math.cos(la) * math.cos(lo), (N + alt) * math.cos(la) * math.sin(lo), (N * (1.0 - WGS84_E2) + alt) * math.sin(la))


def _enu(lat, lon):
    la, lo = math.radians(lat), math.radians(lon)
    return np.array([[-math.sin(lo), math.cos(lo), 0.0],
                     [-math.sin(la) * math.cos(lo), -math.sin(la) * math.sin(lo), math.cos(la)],
                     [math.cos(la) * math.cos(lo), math.cos(la) * math.sin(lo), math.sin(la)]])


def gps_time(week, tow_ms):
    """GPS week and milliseconds of week -> the GPS time as an ISO string (no leap seconds are taken off: this is not UTC)"""
    return (GPS_EPOCH + datetime.timedelta(weeks=int(week), milliseconds=int(tow_ms))).isoformat(timespec="milliseconds")


def parse(blocks):
    """the fields of the blocks whose CRC holds: a dict with None where a block is missing"""
    out = {"frame_number": None, "serial": None, "battery": None, "subframe": None, "calibration": None, "gps_week": None,
           "gps_tow": None, "time": None, "lat": None, "lon": None, "alt": None, "speed": None, "heading": None, "climb": None,
           "sats": None, "ecef": None, "velocity": None, "meas_raw": None, "xdata": None}
    for b in blocks:
        d = b["bytes"]
        if not b["crc_ok"]:
            continue
        if b["id"] == BLOCK_STATUS and len(d) >= 0x28:
            out["frame_number"] = int.from_bytes(d[0:2], "little")
            out["serial"] = d[2:10].decode("ascii", "replace")
            out["battery"] = d[10] / 10.0
            out["subframe"], out["calibration"] = d[0x17], bytes(d[0x18:0x28])
        elif b["id"] == BLOCK_GPSINFO and len(d) >= 6:
            out["gps_week"], out["gps_tow"] = int.from_bytes(d[0:2], "little"), int.from_bytes(d[2:6], "little")
            out["time"] = gps_time(out["gps_week"], out["gps_tow"])
        elif b["id"] == BLOCK_GPSPOS and len(d) >= 19:
            xyz = [int.from_bytes(d[4 * i:4 * i + 4], "little", signed=True) for i in range(3)]
            vel = [int.from_bytes(d[12 + 2 * i:14 + 2 * i], "little", signed=True) for i in range(3)]
            out["ecef"], out["velocity"], out["sats"] = tuple(xyz), tuple(vel), d[18]
            if any(xyz):
                out["lat"], out["lon"], out["alt"] = geodetic(*(v / 100.0 for v in xyz))
                e, nn, u = (_enu(out["lat"], out["lon"]) @ (np.array(vel, dtype=np.float64) / 100.0)).tolist()
                out["speed"], out["heading"], out["climb"] = math.hypot(e, nn), math.degrees(math.atan2(e, nn)) % 360.0, u
        elif b["id"] == BLOCK_MEAS and len(d) >= 36:
            out["meas_raw"] = [int.from_bytes(d[3 * i:3 * i + 3], "little") for i in range(12)]
        elif b["id"] == BLOCK_XDATA:
            out["xdata"] = bytes(d)
    return out


# ------------------------------------------------------------------------------------------------------------------ the host logic
def _rank(det, i):
    errs = det["errs"][i]
    return (bool((errs < 0).any()), int(det["mis"][i]), int(errs[errs >= 0].sum()), int(det["t"][i]))


def frame_of(det, i, rate, followed=False, centre=None):
    """candidate i as a frame dict, or None when it is neither ok (both codewords decode) nor partial (a block's CRC holds);
    centre: the middle of the starts at which the frame decodes (merge), the start itself when None"""
    if det["status"][i] != OK:
        return None
    errs, length = det["errs"][i], int(det["length"][i])
    ok = bool((errs >= 0).all())
    blocks = blocks_of(det["fixed"][i], length, ok)
    if not ok and not any(b["crc_ok"] for b in blocks):
        return None
    f = parse(blocks)
    t = int(det["t"][i])
    f.update(t=t / float(rate), start=t, status="ok" if ok else "partial", extended=length == EXT, polarity=int(det["polarity"][i]),
             blocks=[{"id": b["id"], "crc_ok": b["crc_ok"], "bytes": b["bytes"]} for b in blocks],
             corrected=(int(errs[0]), int(errs[1])), header_errors=int(det["mis"][i]), followed=followed,
             raw=det["fixed"][i].copy(), length=length, centre=t if centre is None else int(centre))
    return f


def merge(det, sps):
    """The candidates -> (the kept indices in time order, how many duplicates were dropped, per kept index the group's centre):
    candidates inside the audio whose starts lie within one bit time of the group's first are one frame; one whose codewords both
    decode goes before one that is not, then the one with the fewest wrong header places stays, then the fewest corrected bytes,
    then the earliest.  The earliest of a run of equals is the run's early edge, with little timing margin left; the centre, the
    middle of the group's starts whose codewords both decode (of all its starts when none does), is where `decode` predicts the
    next frame from."""
    acc = sorted((int(i) for i in np.flatnonzero(det["status"] == OK)), key=lambda i: (int(det["t"][i]), i))
    t = det["t"].tolist()
    keep, dup, a, centre = [], 0, 0, {}
    while a < len(acc):
        b = a
        while b < len(acc) and t[acc[b]] - t[acc[a]] <= sps:
            b += 1
        keep.append(min(acc[a:b], key=lambda j: _rank(det, j)))
        good = [t[j] for j in acc[a:b] if not _rank(det, j)[0]] or [t[j] for j in acc[a:b]]
        centre[keep[-1]] = (good[0] + good[-1]) // 2
        dup += b - a - 1
        a = b
    return keep, dup, centre


def assemble(found):
    """frames -> per serial a dict: first, last (frame numbers), frames, position (the last valid lat, lon, alt or None),
    calibration uint8[51, 16], seen bool[51]"""
    out = {}
    for f in found:
        if f["serial"] is None:
            continue
        s = out.setdefault(f["serial"], {"first": f["frame_number"], "last": f["frame_number"], "frames": 0, "position": None,
                                         "calibration": np.zeros((SUBFRAMES, 16), np.uint8), "seen": np.zeros(SUBFRAMES, bool)})
        s["frames"] += 1
        s["last"] = f["frame_number"]
        if f["lat"] is not None:
            s["position"] = (f["lat"], f["lon"], f["alt"])
        if f["subframe"] is not None and f["subframe"] < SUBFRAMES:
            s["calibration"][f["subframe"]] = np.frombuffer(f["calibration"], dtype=np.uint8)
            s["seen"][f["subframe"]] = True
    return out


def decode(audio, rate, slack=4, follow=2, w=None, ops=None):
    """The chain behind decode_rs41 over the audio (a float64 device array for DeviceOps, NumPy for HostOps) at `rate` S/s ->
    (frames in time order, frameInfo, the candidates' dict)."""
    ops = HostOps() if ops is None else ops
    if int(follow) != follow or follow < 0:
        raise ValueError("rs41: follow must be a count from 0 up, got %r" % (follow,))
    sps, w, slack = params(rate, w, slack)
    n = len(audio)
    det = ops.detect(audio, sps, w, slack)
    keep, dup, centre = merge(det, sps)
    found = [f for f in (frame_of(det, i, rate, centre=centre[i]) for i in keep) if f is not None]
    info = {"samples": n, "candidates": len(det["t"]), "duplicates": dup, "dropped": len(keep) - len(found), "followed": 0}
    ops.lap("host")
    period = int(round(rate))
    shifts = np.array([-1, 0, 1], dtype=np.int64) * max(1, int(round(sps / 3.0)))
    tails = [(f, 0) for f in found]                    # (a frame, how many followed frames lead up to it)

    def kept_near(at):
        """a kept frame within one bit time of `at`: what `merge` calls one frame.  A sonde's second is round(rate) samples only to
        the two clocks' difference, so its next header lies some samples off the prediction"""
        return any(abs(g["centre"] - at) <= sps for g in found)
    while follow and tails:
        ask = []
        for f, run in tails:
            at = f["centre"] + period
            if run < follow and at < n and not kept_near(at):
                ask.append((at, run))
        ask = sorted(set(ask))
        if not ask:
            break
        # each prediction a third of a bit early, as it is and a third late: the clocks' difference moves the header by some samples
        # a second, and a start decodes over most of a bit time around its centre
        d = ops.frames(audio, sps, w, (np.array([a for a, _ in ask], dtype=np.int64).reshape(-1, 1) + shifts).reshape(-1))
        tails = []
        for j, (at, run) in enumerate(ask):
            tries = [frame_of(d, 3 * j + k, rate, True) for k in range(3)]
            tries = [f for f in tries if f is not None and f["status"] == "ok"]
            if tries and not kept_near(at):
                f = min(tries, key=lambda f: (sum(f["corrected"]), abs(f["start"] - at)))
                found.append(f)
                tails.append((f, run + 1))
                info["followed"] += 1
        ops.lap("host")
    found.sort(key=lambda f: f["start"])
    info["frames"] = len(found)
    info["ok"] = sum(1 for f in found if f["status"] == "ok")
    info["partial"] = info["frames"] - info["ok"]
    return found, info, det


# ------------------------------------------------------------------------------------------------------------------ the synthesiser
def _block(ident, data):
    c = crc16(data)
    return bytes([ident, len(data)]) + bytes(data) + bytes([c & 0xFF, c >> 8])


def build_frame(fields):
    """A field dict -> the de-whitened frame, uint8[320] or uint8[518] when `xdata` (bytes, at most 211) is given.  Keys, all
    optional: frame_number, serial (8 characters), battery (V), subframe, calibration (16 bytes), gps_week, gps_tow (ms), ecef (three
    whole cm) or lat, lon, alt (degrees, m; rounded to the cm in ECEF), velocity (three whole cm/s in ECEF) or speed, heading, climb
    (m/s, degrees), sats, meas_raw (twelve counts below 2^24), gpsraw (0x59 bytes), xdata."""
    g = fields.get
    st = bytearray(0x28)
    st[0:2] = int(g("frame_number", 0)).to_bytes(2, "little")
    st[2:10] = g("serial", "S0000000").encode("ascii").ljust(8)[:8]
    st[10] = int(round(g("battery", 0.0) * 10.0)) & 0xFF
    st[0x17] = int(g("subframe", 0))
    st[0x18:0x28] = bytes(g("calibration", bytes(16))).ljust(16, b"\0")[:16]
    meas = bytearray(0x2A)
    for i, v in enumerate(g("meas_raw", [0] * 12)):
        meas[3 * i:3 * i + 3] = int(v).to_bytes(3, "little")
    info = bytearray(0x1E)
    info[0:2], info[2:6] = int(g("gps_week", 0)).to_bytes(2, "little"), int(g("gps_tow", 0)).to_bytes(4, "little")
    raw = bytes(g("gpsraw", bytes(0x59))).ljust(0x59, b"\0")[:0x59]
    xyz = g("ecef")
    if xyz is None and g("lat") is not None:
        xyz = [int(round(v * 100.0)) for v in ecef(g("lat"), g("lon"), g("alt", 0.0))]
    xyz = [0, 0, 0] if xyz is None else xyz
    vel = g("velocity")
    if vel is None and g("speed") is not None:
        lat, lon, _ = geodetic(*(v / 100.0 for v in xyz))
        hd = math.radians(g("heading", 0.0))
        enu = np.array([g("speed") * math.sin(hd), g("speed") * math.cos(hd), g("climb", 0.0)])
        vel = [int(round(v * 100.0)) for v in (_enu(lat, lon).T @ enu).tolist()]
    vel = [0, 0, 0] if vel is None else vel
    pos = bytearray(0x15)
    for i in range(3):
        pos[4 * i:4 * i + 4] = int(xyz[i]).to_bytes(4, "little", signed=True)
        pos[12 + 2 * i:14 + 2 * i] = int(vel[i]).to_bytes(2, "little", signed=True)
    pos[18] = int(g("sats", 0))
    body = (_block(BLOCK_STATUS, st) + _block(BLOCK_MEAS, meas) + _block(BLOCK_GPSINFO, info) + _block(BLOCK_GPSRAW, raw) +
            _block(BLOCK_GPSPOS, pos))
    xdata = g("xdata")
    if xdata is None:
        body += _block(BLOCK_EMPTY, bytes(0x11))
        length, kind = STD, TYPE_STD
    else:
        if len(xdata) > 211:
            raise ValueError("rs41.build_frame: at most 211 bytes of xdata")
        body += _block(BLOCK_XDATA, bytes(xdata)) + _block(BLOCK_EMPTY, bytes(211 - len(xdata)))
        length, kind = EXT, TYPE_EXT
    f = np.zeros(length, dtype=np.uint8)
    f[:8] = np.frombuffer(HEADER_CLEAR, dtype=np.uint8)
    f[TYPE_AT] = kind
    f[TYPE_AT + 1:] = np.frombuffer(body, dtype=np.uint8)
    return add_parity(f, length)


def air_bits(frame, preamble=PREAMBLE_BITS):
    """a de-whitened frame -> the bits on the air: `preamble` alternating bits that end in a 1, then the whitened bytes, lowest bit
    first"""
    f = np.asarray(frame, dtype=np.uint8)
    white = f ^ np.tile(MASK, 9)[:len(f)]
    return np.concatenate(((np.arange(preamble) & 1).astype(np.uint8), np.unpackbits(white, bitorder="little")))


def _frames_bits(frames, preamble):
    return [air_bits(f if isinstance(f, np.ndarray) else build_frame(f), preamble) for f in frames]


def frame_start(rate, k=0, start=0.0, gap=1.0, preamble=PREAMBLE_BITS):
    """the fractional sample at which the header of frame k of a recording encoded at `start` begins"""
    return start + k * gap * rate + preamble * rate / float(BAUD)


def _levels(bits, bt, over=16):
    """the Gaussian-filtered NRZ levels (+1 for a 1) at `over` points per bit; point j is the time (j + 0.5) / over bits"""
    sq = np.repeat(2.0 * np.asarray(bits, dtype=np.float64) - 1.0, over)
    sigma = over * math.sqrt(math.log(2.0)) / (2.0 * math.pi * bt)
    half = int(math.ceil(4.0 * sigma))
    g = np.exp(-0.5 * (np.arange(-half, half + 1) / sigma) ** 2)
    return np.convolve(np.concatenate((np.full(half, sq[0]), sq, np.full(half, sq[-1]))), g / g.sum(), mode="valid")


def frequency(frames, rate, n, polarity=0, bt=0.5, deviation=DEVIATION, gap=1.0, start=0.0, preamble=PREAMBLE_BITS):
    """(float64[n] frequency in Hz, bool[n] carrier on) of one transmission per frame, frame k from the fractional sample
    start + k gap rate on: a 1 is +deviation (-deviation for polarity 1), Gaussian filtered with the bandwidth-time product bt"""
    f, on = np.zeros(n), np.zeros(n, dtype=bool)
    spb, over = rate / float(BAUD), 16
    for k, bits in enumerate(_frames_bits(frames, preamble)):
        s = start + k * gap * rate
        lo, hi = max(int(math.ceil(s)), 0), min(n, int(math.floor(s + len(bits) * spb)) + 1)
        if hi <= lo:
            continue
        lv = _levels(bits, bt, over)
        pos = (np.arange(lo, hi) - s) / spb * over - 0.5
        f[lo:hi] = np.interp(pos, np.arange(len(lv)), lv) * deviation * (-1.0 if polarity else 1.0)
        on[lo:hi] = True
    return f, on


def _length(frames, rate, gap, start, preamble):
    return int(math.ceil(start + (len(frames) - 1) * gap * rate + (preamble + 8 * EXT + 16) * rate / float(BAUD))) + 1 if len(frames) else 0


def encode(frames, rate, polarity=0, bt=0.5, deviation=DEVIATION, gap=1.0, start=0.0, sigma=0.0, seed=0, n=None,
           preamble=PREAMBLE_BITS):
    """The discriminator's view of a sonde: float64[n] audio at `rate` S/s in radians per sample, 2 pi f / rate inside a frame's
    transmission and 0 outside, plus Gaussian noise of `sigma` radians.  frames: field dicts (build_frame) or de-whitened frames as
    uint8 arrays, which lets a test damage bytes; frame k starts `gap` seconds after frame k - 1.  n None: long enough for the last."""
    n = _length(frames, rate, gap, start, preamble) if n is None else int(n)
    f, _ = frequency(frames, rate, n, polarity, bt, deviation, gap, start, preamble)
    x = 2.0 * np.pi * f / rate
    if sigma:
        x = x + np.random.default_rng(seed).normal(0.0, sigma, n)
    return x


def encode_iq(frames, rate, offset=0.0, polarity=0, bt=0.5, deviation=DEVIATION, gap=1.0, start=0.0, amplitude=40.0, sigma=0.0, seed=0,
              n=None, preamble=PREAMBLE_BITS):
    """A recording uint8[n, 2] at `rate` S/s with the sonde at `offset` Hz: the carrier is on during each frame's transmission, from
    a seeded random phase; Gaussian noise of `sigma` per rail; the u8 value is clip(rint(z + 127.5), 0, 255)"""
    n = _length(frames, rate, gap, start, preamble) if n is None else int(n)
    f, on = frequency(frames, rate, n, polarity, bt, deviation, gap, start, preamble)
    rng = np.random.default_rng(seed)
    phase = rng.uniform(0.0, 2.0 * np.pi) + 2.0 * np.pi * np.cumsum(f + offset) / rate
    z = amplitude * on * np.exp(1j * phase)
    v = np.stack((z.real, z.imag), axis=1) + rng.normal(0.0, 1.0, (n, 2)) * sigma + 127.5
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ the front end, restated
def audio_host(raw, fs, offset, bw=48000.0, cut=CUT):
    """(float64 audio, its rate) of the channel at `offset` Hz of a uint8[N, 2] recording in float64 NumPy: decode_rs41's front end
    restated, which is decode_ais's for one channel (ais.audio_host).  The device's float32 stages round differently: this is the
    same chain, not the same bits."""
    from . import ais
    return ais.audio_host(raw, fs, offset, bw, cut)
