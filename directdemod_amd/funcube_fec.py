"""
Funcube telemetry frame decoding -- beyond the reference, which stops at the sync list: from the PLL-corrected soft symbols of the
symbol walk (decode_funcube.getSymbols, 12 ksym/s, ten per channel bit) to the 256-byte telemetry frames of the AO-40 FEC block
(where every stage is defined bit for bit).  Device stages (dd_funcube_frames.h): the differential bit
metric (`soft_bits`, `diff`), the search for the 65-bit sync vector the 80 x 65 interleaver spreads over a frame
(`sync_candidates`), the de-interleaving gather with the terminated Viterbi decode and the descrambling (`viterbi`), and the two
shortened Reed-Solomon (160,128) codewords (`reed_solomon`).  Host stages, O(frames): `frame_starts`, `frame_header`.  NumPy
restatements of the same definitions, for the tests: `soft_bits_np`, `diff_np`, `sync_candidates_np`, `viterbi_np`,
`reed_solomon_np`, and the encoder `encode_frame`, `differential`.  All arithmetic is integer.

The format constants below come from public descriptions of the AO-40 FEC scheme and of the Funcube frame header; they have not
been checked against a recording of a satellite.  They are all here (and, for the device, at the top of dd_funcube_frames.h).
"""
import functools

import numpy as np

from . import lrpt
from ._hip import DevArray, check, lib

FRAME_BYTES = 256                         # telemetry bytes per frame: two codewords' 128 data bytes, interleaved
CHANNEL_BITS = 5200                       # 80 x 65 interleaver slots
SYMBOLS_PER_BIT = 10                      # 12000 symbols/s of the walk over 1200 bit/s
MIN_SCORE = 54                            # of 65
GUARD = 10                                # positions around a candidate in which a better one suppresses it
SYNC_BITS, ROWS = 65, 80                  # sync bit k is channel bit 80 k; slot s is channel bit 80 (s % 65) + s // 65
SYNC_START, SYNC_TAPS = 0x7F, 0x48        # the sync vector's 7-bit register: output bit 6, feedback parity(sr & 0x48)
CODE_BITS, STEPS, TAIL = 5132, 2566, 6    # code bits at slots 65 .. 5196; trellis steps = 2560 data bits + 6 tail zeros
BLOCK_BYTES = 320                         # the scrambled block: two interleaved codewords of 160 bytes
RS_DATA, RS_PARITY, RS_PAD, RS_DEPTH = 128, 32, 95, 2     # RS(255,223) shortened by 95 leading zero bytes
RS_WORD = RS_DATA + RS_PARITY
SPAN = SYMBOLS_PER_BIT * (CHANNEL_BITS - 1) + 1           # entries of D a frame spans: p .. p + 51990
START_METRIC = -(1 << 24)                 # of the states other than 0 at the first trellis step
INFO = np.dtype([("symbol", np.int64), ("sample", np.int64), ("inverted", np.int64), ("sync_score", np.int64),
                 ("sync_corr", np.int64), ("corrected", np.int64), ("rs_errors", np.int64, (RS_DEPTH,)), ("ok", np.bool_),
                 ("sat_id", np.int64), ("frame_type", np.int64)])


# ------------------------------------------------------------------ the definitions in NumPy
@functools.lru_cache(maxsize=None)
def sync_vector():
    """uint8[65]: sr = 0x7F, output bit 6, sr = ((sr << 1) | parity(sr & 0x48)) & 0x7F"""
    sr, out = SYNC_START, []
    for _ in range(SYNC_BITS):
        out.append((sr >> 6) & 1)
        sr = ((sr << 1) | (bin(sr & SYNC_TAPS).count("1") & 1)) & 0x7F
    v = np.array(out, dtype=np.uint8)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def code_positions():
    """int64[5132]: the channel bit of code bit j, 80 ((65 + j) % 65) + (65 + j) // 65"""
    s = SYNC_BITS + np.arange(CODE_BITS, dtype=np.int64)
    q = ROWS * (s % SYNC_BITS) + s // SYNC_BITS
    q.setflags(write=False)
    return q


def diff_np(r):
    """int8 soft symbols r[n] -> D int8[n - 19]: S[i] = r[i] + .. + r[i + 9]; with a = S[i + 10], b = S[i]: 0 when either is 0,
    else +-min(min(|a|, |b|) // 10, 127), + where the signs differ (a phase flip: channel bit 1).  Empty for n < 20."""
    r = np.asarray(r, dtype=np.int8).astype(np.int32)
    if len(r) < 2 * SYMBOLS_PER_BIT:
        return np.zeros(0, dtype=np.int8)
    c = np.concatenate(([0], np.cumsum(r, dtype=np.int64)))
    S = (c[SYMBOLS_PER_BIT:] - c[:-SYMBOLS_PER_BIT]).astype(np.int32)
    a, b = S[SYMBOLS_PER_BIT:], S[:-SYMBOLS_PER_BIT]
    mag = np.minimum(np.minimum(np.abs(a), np.abs(b)) // SYMBOLS_PER_BIT, 127)
    s = np.where((a < 0) != (b < 0), 1, -1)
    return np.where((a == 0) | (b == 0), 0, s * mag).astype(np.int8)


def soft_bits_np(sym):
    """complex symbols -> D: diff_np of lim(re / 2), the even entries of lrpt.soft_np"""
    return diff_np(lrpt.soft_np(sym)[0::2])


def sync_candidates_np(D, min_score=MIN_SCORE):
    """int64[c, 3] = every (p, C, score) with score >= min_score, sorted by p: C(p) = sum of (2 V[k] - 1) D[p + 800 k]; the hard bit
    is D > 0, or D < 0 when C(p) < 0; score = how many of the 65 equal V[k]"""
    D = np.asarray(D, dtype=np.int8)
    npos = max(len(D) - (SPAN - 1), 0)
    if npos == 0:
        return np.zeros((0, 3), dtype=np.int64)
    V = sync_vector()
    C = np.zeros(npos, dtype=np.int32)
    pos = np.zeros(npos, dtype=np.int32)
    neg = np.zeros(npos, dtype=np.int32)
    for k in range(SYNC_BITS):
        d = D[ROWS * SYMBOLS_PER_BIT * k:ROWS * SYMBOLS_PER_BIT * k + npos]
        C += (2 * int(V[k]) - 1) * d.astype(np.int32)
        pos += (d > 0) == bool(V[k])
        neg += (d < 0) == bool(V[k])
    score = np.where(C < 0, neg, pos)
    p = np.nonzero(score >= min_score)[0]
    return np.stack((p, C[p], score[p]), axis=1).astype(np.int64).reshape(-1, 3)


def frame_starts(cands):
    """candidates int64[c, 3] = (p, C, score) -> the frame starts among them, sorted by p: no candidate within +-10 positions has a
    larger |C|; among equal |C| the lower p wins"""
    c = np.asarray(cands, dtype=np.int64).reshape(-1, 3)
    c = c[np.argsort(c[:, 0], kind="stable")]
    mag = np.abs(c[:, 1])
    keep = []
    lo = 0
    for i in range(len(c)):
        p = c[i, 0]
        while c[lo, 0] < p - GUARD:
            lo += 1
        best = True
        j = lo
        while j < len(c) and c[j, 0] <= p + GUARD:
            if j != i and (mag[j] > mag[i] or (mag[j] == mag[i] and c[j, 0] < p)):
                best = False
                break
            j += 1
        if best:
            keep.append(i)
    return c[keep]


def _soft_code(D, p, inv):
    D = np.asarray(D, dtype=np.int8)
    if p < 0 or p + SPAN > len(D) or inv not in (0, 1):
        raise ValueError("funcube_fec: frame outside D")
    x = D[p + SYMBOLS_PER_BIT * code_positions()].astype(np.int32)
    return -x if inv else x


def viterbi_np(D, p, inv):
    """One frame at position p of D, polarity inv -> (block uint8[320], corrected): the gather x[j] = +-D[p + 10 pos(j)], the
    terminated K = 7 trellis of lrpt (state 0 starts at 0, the others at -(1 << 24); x = 1 survives only when strictly larger;
    traceback from state 0), bits 0..2559 packed MSB first XOR the pseudo-noise sequence, and how many of the 5132 hard bits x > 0
    differ from the re-encoding of the 2566 decoded bits"""
    x = _soft_code(D, int(p), int(inv))
    a, b = x[0::2], x[1::2]
    m = np.full(64, START_METRIC, dtype=np.int32)
    m[0] = 0
    dec = np.zeros((STEPS, 64), dtype=bool)
    for t in range(STEPS):
        c = m[lrpt._PRED] + (lrpt._S1 * a[t] + lrpt._S2 * b[t]).astype(np.int32)
        d = c[:, 1] > c[:, 0]
        dec[t] = d
        m = np.where(d, c[:, 1], c[:, 0])
    bits = np.zeros(STEPS, dtype=np.uint8)
    st = 0
    for t in range(STEPS - 1, -1, -1):
        bits[t] = st >> 5
        st = ((st & 31) << 1) | int(dec[t, st])
    block = np.packbits(bits[:8 * BLOCK_BYTES]) ^ lrpt.pn_sequence(BLOCK_BYTES)
    corrected = int(np.sum(lrpt.encode(bits) != (x > 0)))
    return block, corrected


def reed_solomon_np(blocks):
    """blocks uint8[n, 320] -> (frames uint8[n, 256], errors int32[n, 2]): codeword c = block[c::2] behind 95 zero bytes, decoded as
    lrpt's (255,223) code; a corrected word with a non-zero byte among the 95 counts as not decodable (-1).  Frame bytes c::2 are
    the codeword's 128 data bytes, corrected where it decoded, as received where it did not."""
    blocks = np.asarray(blocks, dtype=np.uint8).reshape(-1, BLOCK_BYTES)
    n = len(blocks)
    words = np.zeros((n, RS_DEPTH, lrpt.RS_N), dtype=np.uint8)
    for c in range(RS_DEPTH):
        words[:, c, RS_PAD:] = blocks[:, c::RS_DEPTH]
    fixed, errors = lrpt.rs_decode_np(words)
    bad = (errors >= 0) & fixed[:, :, :RS_PAD].any(axis=2)
    fixed = np.where(bad[:, :, None], words, fixed)
    errors = np.where(bad, -1, errors).astype(np.int32)
    frames = np.zeros((n, FRAME_BYTES), dtype=np.uint8)
    for c in range(RS_DEPTH):
        frames[:, c::RS_DEPTH] = fixed[:, c, RS_PAD:RS_PAD + RS_DATA]
    return frames, errors


def frames_np(D, min_score=MIN_SCORE):
    """D -> (frames uint8[n, 256], starts int64[n, 3] = (p, C, score), corrected int64[n], errors int32[n, 2]): every stage above,
    one after the other"""
    starts = frame_starts(sync_candidates_np(D, min_score))
    done = [viterbi_np(D, p, C < 0) for p, C, _ in starts]
    blocks = np.array([b for b, _ in done], dtype=np.uint8).reshape(-1, BLOCK_BYTES)
    frames, errors = reed_solomon_np(blocks)
    return frames, starts, np.array([c for _, c in done], dtype=np.int64), errors


def rs_block(data):
    """data uint8[256] -> the 320-byte block before scrambling: bytes c::2 = codeword c = 128 data bytes data[c::2], then the 32
    parity bytes of the (255,223) code over 95 zero bytes and the data"""
    data = np.asarray(data, dtype=np.uint8)
    if data.shape != (FRAME_BYTES,):
        raise ValueError("funcube_fec: 256 bytes per frame")
    blk = np.zeros(BLOCK_BYTES, dtype=np.uint8)
    for c in range(RS_DEPTH):
        word = np.zeros(lrpt.RS_K, dtype=np.uint8)
        word[RS_PAD:] = data[c::RS_DEPTH]
        blk[c::RS_DEPTH] = lrpt.rs_encode(word)[RS_PAD:]
    return blk


def encode_frame(data):
    """data uint8[256] -> uint8[5200] channel bits: Reed-Solomon, interleave two deep, scramble, the K = 7 code with six tail zeros,
    the sync vector at channel bits 80 k, the code bits through the interleaver; the last three slots stay 0"""
    bits = np.concatenate((np.unpackbits(rs_block(data) ^ lrpt.pn_sequence(BLOCK_BYTES)), np.zeros(TAIL, dtype=np.uint8)))
    out = np.zeros(CHANNEL_BITS, dtype=np.uint8)
    out[ROWS * np.arange(SYNC_BITS)] = sync_vector()
    out[code_positions()] = lrpt.encode(bits)
    return out


def differential(bits, start=0):
    """channel bits -> the levels sent, uint8[len(bits)]: a 1 flips the phase; `start` is the level before the first bit"""
    return (np.bitwise_xor.accumulate(np.asarray(bits, dtype=np.uint8)) ^ np.uint8(start & 1)).astype(np.uint8)


def frame_header(frame):
    """satellite id (byte 0's top two bits) and frame type (its low six bits); the layout is from public descriptions"""
    b = int(np.asarray(frame, dtype=np.uint8).reshape(-1)[0])
    return dict(sat_id=b >> 6, frame_type=b & 0x3F)


# ------------------------------------------------------------------ device stages
def diff(soft, n):
    """device int8 pairs (lrpt.soft_symbols' output, the real part in the even entries) of n symbols -> device D int8[max(n - 19, 0)]"""
    if soft.dtype != np.dtype(np.int8) or n < 0 or soft.n < 2 * n:
        raise ValueError("funcube_fec.diff: a device int8 array of n pairs expected")
    m = max(n - (2 * SYMBOLS_PER_BIT - 1), 0)
    out = DevArray(max(m, 1), np.int8)
    check(lib().dd_fc_diff(soft.ptr, n, out.ptr, None), "dd_fc_diff")
    return out.view(0, m)


def soft_bits(sym):
    """complex128 device symbols -> device D int8[max(n - 19, 0)]"""
    return diff(lrpt.soft_symbols(sym), sym.n)


def sync_candidates(D, min_score=MIN_SCORE, cap=1 << 16):
    """device D -> int64[c, 3] = every (p, C, score) with score >= min_score, sorted by p; more than `cap` of them raise"""
    if D.dtype != np.dtype(np.int8):
        raise ValueError("funcube_fec.sync_candidates: a device int8 array expected")
    cand = DevArray(3 * max(cap, 1), np.int64)
    cnt = DevArray(1, np.uint64)
    check(lib().dd_fc_sync_search(D.ptr, D.n, min_score, cap, cand.ptr, cnt.ptr, None), "dd_fc_sync_search")
    c = int(cnt.to_host()[0])
    if c > cap:
        raise RuntimeError("Funcube sync search: %d candidates, more than %d" % (c, cap))
    out = cand.view(0, 3 * c).to_host().reshape(c, 3)
    return out[np.argsort(out[:, 0], kind="stable")]


def viterbi(D, frames):
    """frames [(p, inv)] -> (blocks uint8[n, 320], corrected int32[n]) on the host: viterbi_np of every frame"""
    if D.dtype != np.dtype(np.int8):
        raise ValueError("funcube_fec.viterbi: a device int8 array expected")
    s = np.ascontiguousarray(np.asarray(frames, dtype=np.int64).reshape(-1, 2))
    n = len(s)
    blocks = DevArray(max(n * BLOCK_BYTES, 1), np.uint8)
    corrected = DevArray(max(n, 1), np.int32)
    check(lib().dd_fc_viterbi(D.ptr, D.n, s.ctypes.data, n, blocks.ptr, corrected.ptr, None), "dd_fc_viterbi")
    return blocks.view(0, n * BLOCK_BYTES).to_host().reshape(n, BLOCK_BYTES), corrected.view(0, n).to_host()


def reed_solomon(blocks):
    """blocks (host uint8[n, 320] or a device uint8 array of n * 320 bytes) -> (frames uint8[n, 256], errors int32[n, 2]), both on
    the host: reed_solomon_np's result"""
    if isinstance(blocks, DevArray):
        if blocks.dtype != np.dtype(np.uint8) or blocks.n % BLOCK_BYTES:
            raise ValueError("funcube_fec.reed_solomon: a device uint8 array of n * 320 bytes expected")
        dev = blocks
    else:
        host = np.ascontiguousarray(blocks, dtype=np.uint8)
        if host.ndim != 2 or host.shape[1] != BLOCK_BYTES:
            raise ValueError("funcube_fec.reed_solomon: uint8[n, 320] expected")
        dev = DevArray.from_host(host)
    n = dev.n // BLOCK_BYTES
    frames = DevArray(max(n * FRAME_BYTES, 1), np.uint8)
    errors = DevArray(max(RS_DEPTH * n, 1), np.int32)
    check(lib().dd_fc_rs(dev.ptr, n, frames.ptr, errors.ptr, None), "dd_fc_rs")
    return (frames.view(0, n * FRAME_BYTES).to_host().reshape(n, FRAME_BYTES),
            errors.view(0, RS_DEPTH * n).to_host().reshape(n, RS_DEPTH))
