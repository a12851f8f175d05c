"""
Meteor-M2 LRPT channel decoding -- beyond the reference, which stops at the sync list: from the PLL-corrected soft symbols of the
symbol walk (decode_meteorm2.getSymbols, 72 ksym/s) to de-randomised 1020-byte frame bodies (where every
stage is defined bit for bit).  Device stages (dd_lrpt.h): the int8 soft pairs (`soft_symbols`), the attached-sync-marker scores
under the eight phase / IQ-swap hypotheses (`asm_candidates`), the block-wise soft-decision Viterbi decode of the rate-1/2, K = 7
code (`viterbi`) and the per-frame finish (`finish`: marker check, de-randomisation, re-encode count).  Host stages, O(frames):
`frame_starts`, `vcdu_header`.  NumPy restatements of the same definitions, for the tests: `encode`, `pn_sequence`, `hypothesis`,
`soft_np`, `asm_scores`, `asm_candidates_np`, `viterbi_blocks`, `finish_np`.  All arithmetic is integer.

Section 4.15 finishes the channel decoder: Reed-Solomon (255,223) correction of a frame's four interleaved codewords on the device
(`reed_solomon`, dd_lrpt_rs.h) and, on the host, the VCDU / M_PDU layer and the reassembly of CCSDS source packets (`mpdu_header`,
`packet_header`, `packets`).  Restatements: `gf_tables`, `rs_generator`, `rs_encode`, `rs_syndromes`, `rs_decode_np`, `interleave`,
`deinterleave`, `rs_frames_np`.

Section 4.16 reads the image packets: the JPEG-like payload's Huffman decoding, dequantisation and 8x8 inverse transform on the
device (`jpeg_decode`, `image`; dd_lrpt_jpeg.h), the packets' image headers and their placement in the picture on the host
(`image_header`, `place`).  Restatements: `huffman_tables`, `quantiser`, `jpeg_blocks_np`, `idct_np`, `image_np`.

Section 4.18 is the modes of the Meteor-M N2-x satellites, from soft symbols: differential (NRZ-M) coding -- the marker search with
another template (`asm_candidates(template=ASM_ENCODED_NRZM)`) and `finish(nrzm=True)` -- and the 80 ksym/s mode's convolutional
interleaver behind its 8-bit marker: `deint_scores`, `deint_lock` (host), `deint` (dd_lrpt_modes.h); the soft-symbol file
(`read_soft`, `write_soft`).  Restatements: `nrzm_encode`, `nrzm_decode`, `finish_nrzm_np`, `interleave_np`, `deinterleave_np`,
`add_markers_np`, `deint_scores_np`, `deint_np`.  decode_lrpt.py runs the whole chain on such a stream.

Section 4.19 adds the one-symbol stagger between the rails that an OQPSK demodulator leaves at two of its four carrier-phase
ambiguities: `restagger` (dd_lrpt_modes.h), restated as `restagger_np`; decode_lrpt's `stagger` keyword tries the three of them.
"""
import ctypes
import functools

import numpy as np

from ._hip import DevArray, check, lib

FRAME_BITS = 8192
BODY_BYTES = 1020
ASM = np.array([0x1A, 0xCF, 0xFC, 0x1D], dtype=np.uint8)
ASM_ENCODED = 0x035D49C24FF2686B          # encode(ASM bits) from state 0, first code bit in bit 63
ASM_SKIP = 12                             # code bits that depend on the previous frame's tail: never scored
MIN_SCORE = 46                            # of 52
GUARD = 31                                # symbols around a candidate in which a better one suppresses it
BLOCK, WARM = 512, 128                    # trellis steps decoded per block; steps of warm-up before and of tail after it
G1, G2 = 0x79, 0x5B
INFO = np.dtype([("symbol", np.int64), ("sample", np.int64), ("hypothesis", np.int64), ("asm_score", np.int64),
                 ("asm_errors", np.int64), ("corrected", np.int64), ("vcid", np.int64), ("counter", np.int64)])
GF_POLY, RS_BETA_LOG, RS_FIRST_ROOT = 0x187, 11, 112     # GF(256) = GF(2)[x] / 0x187, alpha = 2; beta = alpha^11; c(beta^j) = 0, j = 112..143
RS_N, RS_K, RS_T, RS_DEPTH = 255, 223, 16, 4
VCDU_BYTES, ZONE_BYTES = 892, 882                         # a frame's data bytes; the M_PDU packet zone, VCDU bytes 10..891
FILL_VCID, NO_HEADER = 63, 0x7FF
RS_INFO = np.dtype([("errors", np.int64, (RS_DEPTH,)), ("ok", np.bool_), ("vcid", np.int64), ("counter", np.int64)])
PACKET_INFO = np.dtype([("apid", np.int64), ("flags", np.int64), ("count", np.int64), ("vcid", np.int64), ("frame", np.int64),
                        ("length", np.int64)])


# ------------------------------------------------------------------ the definitions in NumPy
def _taps(g):
    return [j for j in range(7) if (g >> j) & 1]


def encode(bits, state=0):
    """The code bits (c1, c2 per input bit, interleaved) of `bits` from encoder state `state` (the previous six input bits, newest at
    bit 5): r = (b << 6) | s, c1 = parity(r & 0x79), c2 = parity(r & 0x5B), s' = r >> 1."""
    bits = np.asarray(bits, dtype=np.uint8)
    ext = np.concatenate((np.array([(state >> j) & 1 for j in range(6)], dtype=np.uint8), bits))     # r bit j of step k = ext[k + j]
    n = len(bits)
    out = np.zeros((n, 2), dtype=np.uint8)
    for col, g in enumerate((G1, G2)):
        for j in _taps(g):
            out[:, col] ^= ext[j:j + n]
    return out.ravel()


def pn_sequence(nbytes=BODY_BYTES):
    """The CCSDS pseudo-noise bytes: h(x) = x^8 + x^7 + x^5 + x^3 + 1, register all ones, output r[0], feedback
    r[0] ^ r[3] ^ r[5] ^ r[7] shifted in at the far end; period 255 bits."""
    r = [1] * 8
    one = []
    for _ in range(255):
        one.append(r[0])
        r = r[1:] + [r[0] ^ r[3] ^ r[5] ^ r[7]]
    reps = -(-8 * nbytes // 255)
    return np.packbits(np.tile(np.array(one, dtype=np.uint8), reps)[:8 * nbytes])


def hypothesis(a, b, h):
    """The soft pair (a, b) under hypothesis h in 0..7, in int32 (-(-128) = 128 survives): h & 3 selects (a, b), (-b, a), (-a, -b),
    (b, -a); h & 4 then exchanges the two."""
    a = np.asarray(a).astype(np.int32)
    b = np.asarray(b).astype(np.int32)
    a, b = ((a, b), (-b, a), (-a, -b), (b, -a))[h & 3]
    return (b, a) if h & 4 else (a, b)


def soft_np(sym):
    """complex symbols -> int8[2 n]: lim(re / 2), lim(im / 2) (symbolsync.lim), interleaved"""
    sym = np.asarray(sym, dtype=np.complex128)
    v = np.stack((sym.real, sym.imag), axis=1).ravel() / 2.0
    out = np.trunc(np.clip(v, -128.0, 127.0))
    out = np.where((v > 0) & (v < 1), 1.0, out)
    out = np.where((v > -1) & (v < 0), -1.0, out)
    return out.astype(np.int8)


def _asm_code_bits(template=ASM_ENCODED):
    return np.array([(template >> (63 - j)) & 1 for j in range(64)], dtype=np.uint8)


def asm_scores(soft, nsym, template=ASM_ENCODED):
    """int64[nsym - 31, 8]: score(p, h) = how many of the code bits j in 12..63 of the encoded marker (`template`) equal the hard
    bit 2p + j under h (0..52); empty for nsym < 32"""
    soft = np.asarray(soft, dtype=np.int8)[:2 * nsym]
    npos = max(nsym - 31, 0)
    out = np.zeros((npos, 8), dtype=np.int64)
    if npos == 0:
        return out
    e = _asm_code_bits(template)[ASM_SKIP:]
    for h in range(8):
        a, b = hypothesis(soft[0::2], soft[1::2], h)
        hard = np.stack((a > 0, b > 0), axis=1).ravel().astype(np.uint8)
        win = np.lib.stride_tricks.sliding_window_view(hard, 64)[::2][:npos, ASM_SKIP:]
        out[:, h] = np.sum(win == e, axis=1)
    return out


def asm_candidates_np(soft, nsym, min_score=MIN_SCORE, template=ASM_ENCODED):
    """int64[m, 3] = every (p, h, score) with score >= min_score, sorted by (p, h)"""
    sc = asm_scores(soft, nsym, template)
    p, h = np.nonzero(sc >= min_score)
    return np.stack((p, h, sc[p, h]), axis=1).astype(np.int64).reshape(-1, 3)


def _trellis():
    """per state ns and predecessor choice x: the predecessor ((ns & 31) << 1) | x and the signs (2 c1 - 1, 2 c2 - 1) of its branch"""
    ns = np.arange(64)[:, None]
    x = np.arange(2)[None, :]
    pred = ((ns & 31) << 1) | x
    r = ((ns >> 5) << 6) | pred
    par = lambda v: np.array([[bin(int(q)).count("1") & 1 for q in row] for row in v])      # noqa: E731
    return pred, 2 * par(r & G1) - 1, 2 * par(r & G2) - 1


_PRED, _S1, _S2 = _trellis()


def _decode_group(a, b, warm, nout):
    """add-compare-select over the steps of a[g, t], b[g, t] (int32 soft pairs under the hypothesis, all 64 metrics 0 at t = 0), then
    traceback from the best final state (lowest index among equals): the input bits of steps warm .. warm + nout - 1, uint8[g, nout]"""
    G, T = a.shape
    m = np.zeros((G, 64), dtype=np.int32)
    dec = np.zeros((T, G, 64), dtype=bool)
    for t in range(T):
        c = m[:, _PRED] + (_S1[None] * a[:, t, None, None] + _S2[None] * b[:, t, None, None]).astype(np.int32)
        d = c[:, :, 1] > c[:, :, 0]                       # x = 1 wins only when strictly larger
        dec[t] = d
        m = np.where(d, c[:, :, 1], c[:, :, 0])
    st = np.argmax(m, axis=1)
    out = np.zeros((G, nout), dtype=np.uint8)
    g = np.arange(G)
    for t in range(T - 1, warm - 1, -1):
        if t < warm + nout:
            out[:, t - warm] = st >> 5
        st = ((st & 31) << 1) | dec[t, g, st]
    return out


def viterbi_blocks(soft, nsym, p, h, nbits, block=BLOCK, warm=WARM):
    """The decoded bits (uint8[nbits]) of the nbits trellis steps from symbol p under hypothesis h: blocks [k, e) of `block` steps,
    each with add-compare-select over max(0, k - warm) .. min(nsym, e + warm) and traceback to k.  block = nbits decodes the span as
    one block."""
    if nbits % block or nbits <= 0 or p < 0 or p + nbits > nsym or not 0 <= h < 8:
        raise ValueError("viterbi_blocks: span")
    soft = np.asarray(soft, dtype=np.int8)
    a, b = hypothesis(soft[0:2 * nsym:2], soft[1:2 * nsym:2], h)
    groups = {}
    for i, k in enumerate(range(p, p + nbits, block)):
        lo, hi = max(0, k - warm), min(nsym, k + block + warm)
        groups.setdefault((k - lo, hi - lo), []).append((i, lo))
    out = np.zeros(nbits, dtype=np.uint8)
    for (w, T), members in groups.items():
        idx = np.array([lo for _, lo in members])[:, None] + np.arange(T)[None, :]
        bits = _decode_group(a[idx], b[idx], w, block)
        for (i, _), row in zip(members, bits):
            out[i * block:(i + 1) * block] = row
    return out


def finish_np(bits, soft, nsym, p, h):
    """One frame's decoded bits (uint8[8192], from symbol p under h) -> (body uint8[1020], asm_errors, corrected): the marker bits that
    differ, bytes 4..1023 XOR PN, and over steps 6..8191 how many of the 2 * 8186 hard input bits differ from the re-encoding of
    the decoded bits (the encoder state taken from the decoded bits themselves)."""
    bits = np.asarray(bits, dtype=np.uint8)
    if len(bits) != FRAME_BITS or p < 0 or p + FRAME_BITS > nsym:
        raise ValueError("finish_np: frame")
    asm_errors = int(np.sum(bits[:32] != np.unpackbits(ASM)))
    body = np.packbits(bits)[4:] ^ pn_sequence()
    soft = np.asarray(soft, dtype=np.int8)
    a, b = hypothesis(soft[2 * p:2 * (p + FRAME_BITS):2], soft[2 * p + 1:2 * (p + FRAME_BITS):2], h)
    hard = np.stack((a > 0, b > 0), axis=1)[6:].ravel().astype(np.uint8)
    code = np.zeros((FRAME_BITS - 6, 2), dtype=np.uint8)
    for col, g in enumerate((G1, G2)):
        for j in _taps(g):
            code[:, col] ^= bits[j:j + FRAME_BITS - 6]
    return body, asm_errors, int(np.sum(code.ravel() != hard))


# ------------------------------------------------------------------ section 4.18 in NumPy: NRZ-M, the 80k interleaver and its marker
ASM_ENCODED_NRZM = 0x03B10B02F33D2076     # encode(nrzm_encode(ASM bits, 0)) from state 0, first code bit in bit 63
INTERLEAVER_BRANCHES, INTERLEAVER_DELAY = 36, 2048
MARKER, MARKER_BITS, GROUP_BITS = 0x27, 8, 72            # the marker byte in front of every 72 interleaved bits
PERIOD_SYMBOLS, MARKER_SYMBOLS = 40, 4                   # (8 + 72) / 2 symbols per period, the first four the marker
DEINT_SEGMENT = 256                                       # periods per segment of the marker score
LOCK_MIN_NUM, LOCK_MIN_DEN = 3, 4                         # locked: at least 3/4 of the counted markers' bits match
DEINT_INFO = np.dtype([("score", np.int64), ("markers", np.int64), ("offset", np.int64), ("hypothesis", np.int64),
                       ("best_score", np.int64)])


def nrzm_encode(d, prev=0):
    """m[i] = m[i-1] ^ d[i] with m[-1] = prev: a 1 changes the level"""
    d = np.asarray(d, dtype=np.uint8)
    return (np.bitwise_xor.accumulate(d) ^ np.uint8(prev & 1)).astype(np.uint8) if len(d) else d.copy()


def nrzm_decode(v):
    """d[i] = v[i] ^ v[i-1] for i >= 1; d[0] = 0 (the bit before lies in another decode span)"""
    v = np.asarray(v, dtype=np.uint8)
    d = np.zeros(len(v), dtype=np.uint8)
    d[1:] = v[1:] ^ v[:-1]
    return d


def finish_nrzm_np(bits, soft, nsym, p, h):
    """finish_np for a differential stream: d = nrzm_decode(bits); asm_errors over bits 1..31 of d, body = packbits(d)[4:] XOR PN;
    corrected is finish_np's, from the Viterbi bits themselves"""
    d = nrzm_decode(bits)
    _, _, corrected = finish_np(bits, soft, nsym, p, h)
    asm_errors = int(np.sum(d[1:32] != np.unpackbits(ASM)[1:]))
    return np.packbits(d)[4:] ^ pn_sequence(), asm_errors, corrected


def _check_interleaver(branches, delay):
    if branches < 1 or GROUP_BITS % branches or delay < 0:
        raise ValueError("interleaver: branches must divide 72 and delay must be >= 0")
    return branches * delay * (branches - 1)


def interleave_np(x, branches=INTERLEAVER_BRANCHES, delay=INTERLEAVER_DELAY):
    """code bits (or any values) x[n] -> y with y[n + B M (n mod B)] = x[n], len(x) + B M (B - 1) long, 0 where nothing lands"""
    x = np.asarray(x)
    span = _check_interleaver(branches, delay)
    y = np.zeros(len(x) + span, dtype=x.dtype)
    n = np.arange(len(x), dtype=np.int64)
    y[n + branches * delay * (n % branches)] = x
    return y


def deinterleave_np(y, branches=INTERLEAVER_BRANCHES, delay=INTERLEAVER_DELAY):
    """x[n] = y[n + B M (n mod B)] for 0 <= n < N = len(y) - B M (B - 1), rounded down to even; empty where N <= 0"""
    y = np.asarray(y)
    N = max(len(y) - _check_interleaver(branches, delay), 0) & ~1
    n = np.arange(N, dtype=np.int64)
    return y[n + branches * delay * (n % branches)]


def marker_bits():
    return np.unpackbits(np.array([MARKER], dtype=np.uint8))


def add_markers_np(bits):
    """The interleaved bits in groups of 72 (the last one filled with 0), each preceded by the 8 bits of 0x27: uint8[80 groups]"""
    bits = np.asarray(bits, dtype=np.uint8)
    groups = -(-len(bits) // GROUP_BITS)
    body = np.zeros((groups, GROUP_BITS), dtype=np.uint8)
    body.ravel()[:len(bits)] = bits
    return np.concatenate((np.tile(marker_bits(), (groups, 1)), body), axis=1).ravel()


def deint_scores_np(soft, nsym, seg=DEINT_SEGMENT):
    """int64[nseg, 40, 8]: for the symbols q with q + 4 <= nsym, how many of the 8 hard bits from bit 2q under h equal the marker's,
    summed into [q // (40 seg), q % 40, h]; nseg = ceil(nsym / (40 seg))"""
    if seg < 1:
        raise ValueError("deint_scores_np: seg")
    soft = np.asarray(soft, dtype=np.int8)[:2 * nsym]
    nseg = -(-nsym // (PERIOD_SYMBOLS * seg))
    out = np.zeros((nseg, PERIOD_SYMBOLS, 8), dtype=np.int64)
    npos = nsym - MARKER_SYMBOLS + 1
    if npos <= 0:
        return out
    q = np.arange(npos, dtype=np.int64)
    for h in range(8):
        a, b = hypothesis(soft[0::2], soft[1::2], h)
        hard = np.stack((a > 0, b > 0), axis=1).ravel().astype(np.uint8)
        sc = np.sum(np.lib.stride_tricks.sliding_window_view(hard, MARKER_BITS)[::2][:npos] == marker_bits(), axis=1)
        np.add.at(out[:, :, h], (q // (PERIOD_SYMBOLS * seg), q % PERIOD_SYMBOLS), sc)
    return out


def _markers(nsym, o, lo=0, hi=None):
    """how many markers of offset o lie wholly inside the symbols and start in [lo, hi)"""
    hi = nsym - MARKER_SYMBOLS + 1 if hi is None else min(hi, nsym - MARKER_SYMBOLS + 1)
    first = max(-(-(lo - o) // PERIOD_SYMBOLS), 0)
    return max(-(-(hi - o) // PERIOD_SYMBOLS) - first, 0)


def deint_lock(scores, nsym, seg=DEINT_SEGMENT):
    """The marker scores int[nseg, 40, 8] of nsym symbols -> dict(offset, hypothesis, score, markers, groups, locked, info): the
    (o, h) with the largest total over the segments (among equals the lower o, then the lower h), how many markers it counts, the
    whole periods from o on, locked = score >= 3/4 of 8 bits per counted marker (and there is one), and per segment a DEINT_INFO
    record: score and markers at the lock, and the segment's own best offset, hypothesis and best_score"""
    sc = np.asarray(scores, dtype=np.int64).reshape(-1, PERIOD_SYMBOLS, 8)
    total = sc.sum(axis=0)
    o, h = (int(v) for v in np.unravel_index(np.argmax(total), total.shape))
    markers = _markers(nsym, o)
    info = np.zeros(len(sc), dtype=DEINT_INFO)
    info["score"] = sc[:, o, h]
    info["markers"] = [_markers(nsym, o, s * PERIOD_SYMBOLS * seg, (s + 1) * PERIOD_SYMBOLS * seg) for s in range(len(sc))]
    best = sc.reshape(len(sc), -1).argmax(axis=1) if len(sc) else np.zeros(0, dtype=np.int64)
    info["offset"], info["hypothesis"] = best // 8, best % 8
    info["best_score"] = sc.reshape(len(sc), -1).max(axis=1) if len(sc) else 0
    score = int(total[o, h])
    return dict(offset=o, hypothesis=h, score=score, markers=markers, groups=max(nsym - o, 0) // PERIOD_SYMBOLS,
                locked=bool(markers > 0 and LOCK_MIN_DEN * score >= LOCK_MIN_NUM * MARKER_BITS * markers), info=info)


def deint_np(soft, nsym, o, h, branches=INTERLEAVER_BRANCHES, delay=INTERLEAVER_DELAY):
    """The deinterleaved soft pairs int8[2 nsym_out] of the stream locked at (o, h): y[72 t + i] = rail i % 2 of symbol
    o + 40 t + 4 + i // 2 under h (128 stored as 127) for t < (nsym - o) // 40, then deinterleave_np"""
    if not (0 <= o < PERIOD_SYMBOLS and 0 <= h < 8):
        raise ValueError("deint_np: offset in 0..39 and hypothesis in 0..7 expected")
    soft = np.asarray(soft, dtype=np.int8)[:2 * nsym]
    groups = (nsym - o) // PERIOD_SYMBOLS
    sym = (o + PERIOD_SYMBOLS * np.arange(groups, dtype=np.int64)[:, None] + MARKER_SYMBOLS
           + np.arange(GROUP_BITS // 2, dtype=np.int64)[None, :]).ravel()
    a, b = hypothesis(soft[2 * sym], soft[2 * sym + 1], h)
    y = np.minimum(np.stack((a, b), axis=1).ravel(), 127).astype(np.int8)
    return deinterleave_np(y, branches, delay)


def restagger_np(soft, nsym, s):
    """The rails of an OQPSK demodulator's output brought together: int8[2 (nsym - |s|)], output pairs
    (I[k], Q[k + s]) for every k with both indices in range, s in -1, 0, +1"""
    if s not in (-1, 0, 1) or nsym < 0:
        raise ValueError("restagger_np: a stagger of -1, 0 or 1 expected")
    soft = np.asarray(soft, dtype=np.int8)[:2 * nsym]
    nout = max(nsym - abs(s), 0)
    lead = 1 if s < 0 else 0
    out = np.zeros(2 * nout, dtype=np.int8)
    out[0::2] = soft[0::2][lead:lead + nout]
    out[1::2] = soft[1::2][lead + s:lead + s + nout]
    return out


STAGGERS = (0, -1, 1)                                     # the order in which stagger="auto" tries them


def stagger_pick(scores):
    """the stagger of STAGGERS with the largest score, the earlier one among equals"""
    return STAGGERS[int(np.argmax(np.asarray(scores, dtype=np.int64)))]


def stagger_scores_np(soft, nsym, interleaved=False, template=ASM_ENCODED):
    """Per stagger of STAGGERS the score of the re-staggered stream: the sum of asm_score over its frame starts, or with
    `interleaved` the marker score of its deint_lock.  (Under a wrong stagger half of a frame marker's bits are random and it stays
    below MIN_SCORE; the 8-bit marker still finds 15/16 of its bits at a neighbouring offset with one rail inverted.)"""
    out = []
    for s in STAGGERS:
        c = restagger_np(soft, nsym, s)
        n = len(c) // 2
        if interleaved:
            out.append(int(deint_lock(deint_scores_np(c, n), n)["score"]))
        else:
            out.append(int(frame_starts(asm_candidates_np(c, n, template=template), n)[:, 2].sum()))
    return out


def read_soft(path):
    """A soft-symbol file (raw int8 I, Q pairs, one pair per symbol) -> int8[2 n]; a trailing odd byte is dropped"""
    soft = np.fromfile(path, dtype=np.int8)
    return soft[:len(soft) & ~1]


def write_soft(path, soft):
    """int8 soft pairs -> a soft-symbol file"""
    soft = np.asarray(soft)
    if soft.dtype != np.dtype(np.int8) or soft.size % 2:
        raise ValueError("write_soft: int8 I, Q pairs expected")
    np.ascontiguousarray(soft).ravel().tofile(path)


# ------------------------------------------------------------------ section 4.15 in NumPy: GF(256), RS(255,223), interleave
@functools.lru_cache(maxsize=None)
def gf_tables():
    """(exp uint8[512], log int16[256]): exp[i] = alpha^(i mod 255), so that exp[log[a] + log[b]] is a * b for non-zero a, b with no
    reduction of the sum; log[0] is 0 and never meant"""
    ex = np.zeros(512, dtype=np.uint8)
    lg = np.zeros(256, dtype=np.int16)
    v = 1
    for i in range(255):
        ex[i] = v
        lg[v] = i
        v <<= 1
        if v & 0x100:
            v ^= GF_POLY
    ex[255:510] = ex[:255]
    ex[510:] = ex[:2]
    ex.setflags(write=False)
    lg.setflags(write=False)
    return ex, lg


def gf_mul(a, b):
    """a * b in GF(256), element-wise over uint8 arrays"""
    ex, lg = gf_tables()
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    return np.where((a == 0) | (b == 0), 0, ex[lg[a] + lg[b]]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def rs_generator():
    """g(x) = prod over j = 112..143 of (x - beta^j), uint8[33], low to high coefficient"""
    ex, _ = gf_tables()
    g = np.array([1], dtype=np.uint8)
    for j in range(RS_FIRST_ROOT, RS_FIRST_ROOT + 2 * RS_T):
        root = ex[RS_BETA_LOG * j % 255]
        g = np.concatenate(([0], g)).astype(np.uint8) ^ np.concatenate((gf_mul(g, root), [0])).astype(np.uint8)
    g.setflags(write=False)
    return g


def rs_encode(data):
    """data uint8[..., 223] -> codewords uint8[..., 255]: the data, then the remainder of data(x) x^32 modulo g(x), high coefficient
    first"""
    data = np.asarray(data, dtype=np.uint8)
    if data.shape[-1] != RS_K:
        raise ValueError("rs_encode: 223 data bytes per word")
    taps = rs_generator()[2 * RS_T - 1::-1]                         # g31 .. g0: register cell k holds the coefficient of x^(31 - k)
    reg = np.zeros(data.shape[:-1] + (2 * RS_T,), dtype=np.uint8)
    for i in range(RS_K):
        fb = data[..., i] ^ reg[..., 0]
        reg = np.concatenate((reg[..., 1:], np.zeros_like(reg[..., :1])), axis=-1) ^ gf_mul(fb[..., None], taps)
    return np.concatenate((data, reg), axis=-1)


def rs_syndromes(words):
    """words uint8[..., 255] -> uint8[..., 32]: S_j = c(beta^(112 + j)) with byte i the coefficient of x^(254 - i)"""
    ex, lg = gf_tables()
    words = np.asarray(words, dtype=np.uint8)
    if words.shape[-1] != RS_N:
        raise ValueError("rs_syndromes: 255 bytes per word")
    lr = (RS_BETA_LOG * (RS_FIRST_ROOT + np.arange(2 * RS_T)) % 255).astype(np.int16)
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


def _rs_correction(S):
    """syndromes uint8[32], not all zero -> (positions, values) of the error pattern Berlekamp-Massey, a search of the 255 positions
    and Forney's formula propose, or None when they propose none: a locator of degree > 16, fewer roots than its degree, a zero
    value.  The caller checks the corrected word's syndromes."""
    ex, lg = (t.tolist() for t in gf_tables())
    S = [int(v) for v in S]

    def mul(a, b):
        return ex[lg[a] + lg[b]] if a and b else 0
    C, B, L, m, b = [1] + [0] * 32, [1] + [0] * 32, 0, 1, 1
    for n in range(2 * RS_T):
        d = S[n]
        for i in range(1, L + 1):
            d ^= mul(C[i], S[n - i])
        if d == 0:
            m += 1
            continue
        coef = ex[lg[d] + 255 - lg[b]]
        T = C[:]
        for i in range(m, 33):
            C[i] ^= mul(coef, B[i - m])
        if 2 * L <= n:
            L, B, b, m = n + 1 - L, T, d, 1
        else:
            m += 1
    if L > RS_T or max(i for i in range(33) if C[i]) != L:
        return None
    lam = C[:RS_T + 1]
    lX = RS_BETA_LOG * (254 - np.arange(RS_N, dtype=np.int64)) % 255       # position i has locator X = beta^(254 - i)
    lx = (255 - lX) % 255                                                      # X^-1
    pos = np.nonzero(_poly_at(lam, lx) == 0)[0]
    if len(pos) != L:
        return None
    omega = [0] * RS_T                                                         # S Lambda mod x^32 has degree < L <= 16
    for k in range(RS_T):
        for i in range(min(k, RS_T) + 1):
            omega[k] ^= mul(lam[i], S[k - i])
    deriv = [lam[i + 1] if i % 2 == 0 else 0 for i in range(RS_T)]              # Lambda'(x): the odd terms, one degree down
    num, den = _poly_at(omega, lx[pos]), _poly_at(deriv, lx[pos])
    if np.any(num == 0) or np.any(den == 0):
        return None
    glog = gf_tables()[1]
    val = gf_tables()[0][(glog[num].astype(np.int64) - glog[den] + (1 - RS_FIRST_ROOT) * lX[pos]) % 255]
    return pos, val


def rs_decode_np(words):
    """words uint8[..., 255] -> (fixed uint8[..., 255], errors int32[...]): the codeword within Hamming distance 16 of each word and
    how many bytes it changes, or the word itself and -1 where there is none.  Table-driven; the syndromes before and after are
    computed for all words together, the locator word by word for the damaged ones."""
    words = np.asarray(words, dtype=np.uint8)
    if words.shape[-1] != RS_N:
        raise ValueError("rs_decode_np: 255 bytes per word")
    flat = words.reshape(-1, RS_N)
    fixed = flat.copy()
    errors = np.zeros(len(flat), dtype=np.int32)
    syn = rs_syndromes(flat)
    tried = []
    for w in np.nonzero(syn.any(axis=1))[0]:
        fix = _rs_correction(syn[w])
        if fix is None:
            errors[w] = -1
        else:
            fixed[w, fix[0]] ^= fix[1]
            errors[w] = len(fix[0])
            tried.append(w)
    if tried:
        tried = np.array(tried)
        bad = tried[rs_syndromes(fixed[tried]).any(axis=1)]
        fixed[bad] = flat[bad]
        errors[bad] = -1
    return fixed.reshape(words.shape), errors.reshape(words.shape[:-1])


def interleave(words):
    """codewords uint8[..., 4, 255] -> bodies uint8[..., 1020]: body byte k is byte k // 4 of codeword k % 4"""
    words = np.asarray(words, dtype=np.uint8)
    if words.shape[-2:] != (RS_DEPTH, RS_N):
        raise ValueError("interleave: four words of 255 bytes")
    return np.ascontiguousarray(np.swapaxes(words, -1, -2)).reshape(words.shape[:-2] + (BODY_BYTES,))


def deinterleave(bodies):
    """bodies uint8[..., 1020] -> codewords uint8[..., 4, 255]"""
    bodies = np.asarray(bodies, dtype=np.uint8)
    if bodies.shape[-1] != BODY_BYTES:
        raise ValueError("deinterleave: 1020 bytes per body")
    return np.ascontiguousarray(np.swapaxes(bodies.reshape(bodies.shape[:-1] + (RS_N, RS_DEPTH)), -1, -2))


def rs_frames_np(bodies):
    """bodies uint8[n, 1020] -> (fixed uint8[n, 1020], errors int32[n, 4]): every decodable codeword corrected, parity included"""
    bodies = np.asarray(bodies, dtype=np.uint8).reshape(-1, BODY_BYTES)
    fixed, errors = rs_decode_np(deinterleave(bodies))
    return interleave(fixed), errors


# ------------------------------------------------------------------ host stages
def frame_starts(cands, nsym):
    """candidates int64[m, 3] = (p, h, score) -> the frame starts among them, sorted by p: no candidate within +-31 symbols is better
    (higher score; among equal scores the lower p, then the lower h), and the frame fits (p + 8192 <= nsym)"""
    c = np.asarray(cands, dtype=np.int64).reshape(-1, 3)
    c = c[np.lexsort((c[:, 1], c[:, 0]))]
    keep = []
    lo = 0
    for i in range(len(c)):
        p, h, sc = c[i]
        while c[lo, 0] < p - GUARD:
            lo += 1
        best = True
        j = lo
        while j < len(c) and c[j, 0] <= p + GUARD:
            if j != i and (c[j, 2] > sc or (c[j, 2] == sc and (c[j, 0], c[j, 1]) < (p, h))):
                best = False
                break
            j += 1
        if best and p + FRAME_BITS <= nsym:
            keep.append(i)
    return c[keep]


def vcdu_header(body):
    """version, spacecraft id, virtual channel and the 24-bit frame counter from a frame body's first six bytes"""
    body = np.frombuffer(body, dtype=np.uint8) if isinstance(body, (bytes, bytearray)) else np.asarray(body, dtype=np.uint8)
    b = [int(v) for v in body[:6]]
    return dict(version=b[0] >> 6, scid=((b[0] & 0x3F) << 2) | (b[1] >> 6), vcid=b[1] & 0x3F, counter=(b[2] << 16) | (b[3] << 8) | b[4])


def mpdu_header(vcdu):
    """spare bits and the first-header pointer from a VCDU's bytes 8..9: fhp = ((b8 & 7) << 8) | b9"""
    v = np.frombuffer(vcdu, dtype=np.uint8) if isinstance(vcdu, (bytes, bytearray)) else np.asarray(vcdu, dtype=np.uint8)
    return dict(spare=int(v[8]) >> 3, fhp=((int(v[8]) & 7) << 8) | int(v[9]))


def packet_header(pkt):
    """version, type, secondary-header flag, APID, sequence flags, sequence count and the total length 7 + (b4 << 8 | b5) from a
    source packet's first six bytes"""
    b = [int(v) for v in bytes(pkt[:6])]
    return dict(version=b[0] >> 5, type=(b[0] >> 4) & 1, secondary=(b[0] >> 3) & 1, apid=((b[0] & 7) << 8) | b[1], flags=b[2] >> 6,
                count=((b[2] & 0x3F) << 8) | b[3], length=7 + ((b[4] << 8) | b[5]))


def packets(vcdus, ok, vcids, counters):
    """The source packets of the frames in stream order (section 4.15, reassembly) -> (list of bytes, info PACKET_INFO[m]).
    vcdus uint8[n, 892]; ok, vcids, counters per frame (rsInfo's fields)."""
    vcdus = np.asarray(vcdus, dtype=np.uint8).reshape(-1, VCDU_BYTES)
    part, last, out, rows = {}, {}, [], []                  # per channel: (bytes so far, frame of the first byte); the last counter

    def emit(pkt, vcid, frame):
        h = packet_header(pkt)
        out.append(bytes(pkt))
        rows.append((h["apid"], h["flags"], h["count"], vcid, frame, len(pkt)))

    def complete(pkt):
        return len(pkt) >= 6 and len(pkt) == packet_header(pkt)["length"]
    for f, (v, good, vcid, ctr) in enumerate(zip(vcdus, ok, vcids, counters)):
        if not good:
            part.clear()                                    # whose frame it was is not known
            continue
        vcid, ctr = int(vcid), int(ctr)
        if vcid == FILL_VCID:
            continue
        if vcid in last and ctr != (last[vcid] + 1) & 0xFFFFFF:
            part.pop(vcid, None)
        last[vcid] = ctr
        fhp = mpdu_header(v)["fhp"]
        zone = v[10:].tobytes()
        held = part.pop(vcid, None)
        if fhp == NO_HEADER:
            if held is not None:
                part[vcid] = (held[0] + zone, held[1])
            continue
        if fhp >= ZONE_BYTES:
            continue
        if held is not None and complete(held[0] + zone[:fhp]):
            emit(held[0] + zone[:fhp], vcid, held[1])
        pos = fhp
        while pos < ZONE_BYTES:
            rest = zone[pos:]
            if len(rest) < 6 or len(rest) < packet_header(rest)["length"]:
                part[vcid] = (rest, f)
                break
            n = packet_header(rest)["length"]
            emit(rest[:n], vcid, f)
            pos += n
    return out, np.array(rows, dtype=PACKET_INFO).reshape(-1)


# ------------------------------------------------------------------ device stages
def _spans(spans):
    s = np.ascontiguousarray(np.asarray(spans, dtype=np.int64).reshape(-1, 2))
    return s, len(s)


def soft_symbols(sym):
    """complex128 device symbols -> device int8[2 n], (lim(re / 2), lim(im / 2)) per symbol"""
    if sym.dtype != np.dtype(np.complex128):
        raise TypeError("complex128 device array expected, got %s" % sym.dtype)
    out = DevArray(max(2 * sym.n, 1), np.int8)
    check(lib().dd_lrpt_soft(sym.ptr, sym.n, out.ptr, None), "dd_lrpt_soft")
    return out.view(0, 2 * sym.n)


def asm_candidates(soft, nsym, min_score=MIN_SCORE, cap=1 << 16, template=ASM_ENCODED):
    """int64[m, 3] = every (p, h, score) with score >= min_score, sorted by (p, h); more than `cap` of them raise.  `template`: the
    encoded marker, ASM_ENCODED (dd_lrpt_asm_search) or another 64-bit code word such as ASM_ENCODED_NRZM (dd_lrpt_asm_search_t)"""
    cand = DevArray(3 * max(cap, 1), np.int64)
    cnt = DevArray(1, np.uint64)
    if template == ASM_ENCODED:
        check(lib().dd_lrpt_asm_search(soft.ptr, nsym, min_score, cap, cand.ptr, cnt.ptr, None), "dd_lrpt_asm_search")
    else:
        check(lib().dd_lrpt_asm_search_t(soft.ptr, nsym, template, min_score, cap, cand.ptr, cnt.ptr, None), "dd_lrpt_asm_search_t")
    m = int(cnt.to_host()[0])
    if m > cap:
        raise RuntimeError("LRPT marker search: %d candidates, more than %d" % (m, cap))
    c = cand.view(0, 3 * m).to_host().reshape(m, 3)
    return c[np.lexsort((c[:, 1], c[:, 0]))]


def viterbi(soft, nsym, spans, nbits=FRAME_BITS):
    """spans [(p, h)] -> device uint8[len(spans) * nbits / 8]: each span's nbits decoded bits from symbol p under h, MSB first"""
    s, n = _spans(spans)
    out = DevArray(max(n * nbits // 8, 1), np.uint8)
    check(lib().dd_lrpt_viterbi(soft.ptr, nsym, s.ctypes.data, n, nbits, out.ptr, None), "dd_lrpt_viterbi")
    return out.view(0, n * nbits // 8)


def finish(bits, soft, nsym, spans, nrzm=False):
    """The frames decoded by viterbi(soft, nsym, spans) -> (bodies uint8[n, 1020], info int32[n, 3] = asm_errors, corrected, vcid);
    nrzm: the stream is differential, the frames' bits are nrzm_decode of the Viterbi bits (dd_lrpt_finish_nrzm)"""
    s, n = _spans(spans)
    bodies = DevArray(max(n * BODY_BYTES, 1), np.uint8)
    info = DevArray(max(3 * n, 1), np.int32)
    entry = "dd_lrpt_finish_nrzm" if nrzm else "dd_lrpt_finish"
    check(getattr(lib(), entry)(bits.ptr, soft.ptr, nsym, s.ctypes.data, n, bodies.ptr, info.ptr, None), entry)
    return bodies.view(0, n * BODY_BYTES).to_host().reshape(n, BODY_BYTES), info.view(0, 3 * n).to_host().reshape(n, 3)


def deint_scores(soft, nsym, seg=DEINT_SEGMENT):
    """deint_scores_np on the device -> int64[nseg, 40, 8] on the host"""
    nseg = -(-nsym // (PERIOD_SYMBOLS * seg)) if seg >= 1 and nsym >= 0 else 0
    sc = DevArray(max(nseg * PERIOD_SYMBOLS * 8, 1), np.int32)
    check(lib().dd_lrpt_deint_scores(soft.ptr, nsym, seg, sc.ptr, None), "dd_lrpt_deint_scores")
    return sc.view(0, nseg * PERIOD_SYMBOLS * 8).to_host().astype(np.int64).reshape(nseg, PERIOD_SYMBOLS, 8)


def deint(soft, nsym, o, h, branches=INTERLEAVER_BRANCHES, delay=INTERLEAVER_DELAY):
    """deint_np on the device (dd_lrpt_deinterleave) -> device int8[2 nsym_out].  (`deinterleave` is section 4.15's, of the
    Reed-Solomon codewords.)"""
    out = DevArray(max(GROUP_BITS * (max(nsym, 0) // PERIOD_SYMBOLS), 1), np.int8)        # 36 pairs per period at the most
    nout = ctypes.c_int64(0)
    check(lib().dd_lrpt_deinterleave(soft.ptr, nsym, o, h, branches, delay, out.ptr, ctypes.byref(nout), None), "dd_lrpt_deinterleave")
    return out.view(0, 2 * nout.value)


def restagger(soft, nsym, s):
    """restagger_np on the device (dd_lrpt_restagger) -> device int8[2 (nsym - |s|)]"""
    nout = max(nsym - abs(s), 0) if s in (-1, 0, 1) else 0
    out = DevArray(max(2 * nout, 1), np.int8)
    check(lib().dd_lrpt_restagger(soft.ptr, nsym, s, out.ptr, None), "dd_lrpt_restagger")
    return out.view(0, 2 * nout)


def reed_solomon(bodies):
    """bodies (host uint8[n, 1020] or a device uint8 array of n * 1020 bytes) -> (fixed uint8[n, 1020], errors int32[n, 4]), both on
    the host: every codeword within 16 byte errors of a codeword corrected (parity included) with the count, the others unchanged
    with -1"""
    if isinstance(bodies, DevArray):
        if bodies.dtype != np.dtype(np.uint8) or bodies.n % BODY_BYTES:
            raise ValueError("reed_solomon: a device uint8 array of n * 1020 bytes expected")
        dev = bodies
    else:
        host = np.ascontiguousarray(bodies, dtype=np.uint8)
        if host.ndim != 2 or host.shape[1] != BODY_BYTES:
            raise ValueError("reed_solomon: uint8[n, 1020] expected")
        dev = DevArray.from_host(host)
    n = dev.n // BODY_BYTES
    fixed = DevArray(max(n * BODY_BYTES, 1), np.uint8)
    errors = DevArray(max(RS_DEPTH * n, 1), np.int32)
    check(lib().dd_lrpt_rs(dev.ptr, n, fixed.ptr, errors.ptr, None), "dd_lrpt_rs")
    return (fixed.view(0, n * BODY_BYTES).to_host().reshape(n, BODY_BYTES),
            errors.view(0, RS_DEPTH * n).to_host().reshape(n, RS_DEPTH))


# ------------------------------------------------------------------ section 4.16 in NumPy: the image packets' JPEG-like payload
DC_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
DC_VALUES = bytes(range(12))
AC_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)
AC_VALUES = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63], dtype=np.int64)
QUANT_STD = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                      87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                      72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
IDCT_M = np.array([[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
                   [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
                   [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
                   [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
                   [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
                   [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
                   [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
                   [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], dtype=np.int64)       # M[k][n] = round(8192 a_k cos((2n+1) k pi / 16))
MCU_PER_PACKET, MCU_PER_STRIP, IMAGE_WIDTH = 14, 196, 1568
IMAGE_HEADER_BYTES = 20                                   # a packet's entropy-coded data starts here
IMAGE_APIDS, IMAGE_PERIOD = (64, 65, 66), 43
IMAGE_INFO = np.dtype([("packet", np.int64), ("apid", np.int64), ("mcun", np.int64), ("q", np.int64), ("mcus", np.int64),
                       ("strip", np.int64), ("day", np.int64), ("ms", np.int64), ("us", np.int64)])


@functools.lru_cache(maxsize=None)
def huffman_tables():
    """{"dc", "ac"} -> {(length, code): value}: the canonical codes of the two luminance tables of T.81 Annex K -- within a length in
    value order, the first code of length 1 is 0, then code = (code + count) << 1"""
    out = {}
    for name, bits, values in (("dc", DC_BITS, DC_VALUES), ("ac", AC_BITS, AC_VALUES)):
        table, code, k = {}, 0, 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                table[(length, code)] = values[k]
                code += 1
                k += 1
            code <<= 1
        out[name] = table
    return out


def quantiser(q):
    """int64[64], row-major: the standard luminance table scaled for quality factor q (0..255)"""
    q = int(q)
    if 21 <= q <= 49:
        return np.maximum(1, (100 * QUANT_STD + q) // (2 * q))
    return np.maximum(1, (max(0, 200 - 2 * q) * QUANT_STD + 50) // 100)


def extend(v, n):
    """EXTEND of T.81: the n-bit field v as a signed value"""
    return v if n == 0 or v >= (1 << (n - 1)) else v - (1 << n) + 1


class _Bits:
    """a packet's bits, MSB first; a read past the last byte raises EOFError: nothing is padded"""

    def __init__(self, data):
        self.bits = np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8)).tolist()
        self.at = 0

    def take(self, n):
        if self.at + n > len(self.bits):
            raise EOFError
        v = 0
        for b in self.bits[self.at:self.at + n]:
            v = (v << 1) | b
        self.at += n
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.take(1)
            if (length, code) in table:
                return table[(length, code)]
        raise ValueError("no code matches within 16 bits")


def jpeg_blocks_np(payload):
    """A packet's entropy-coded bytes -> (coefficients int64[14, 64], row-major, not yet dequantised; mcus): the blocks decoded before
    the first failure (a code that does not exist, a position past 63, a needed bit past the last byte).  Rows from mcus on are 0."""
    tables = huffman_tables()
    rd = _Bits(payload)
    coef = np.zeros((MCU_PER_PACKET, 64), dtype=np.int64)
    pred = 0
    for m in range(MCU_PER_PACKET):
        block = np.zeros(64, dtype=np.int64)
        try:
            n = rd.symbol(tables["dc"])
            pred += extend(rd.take(n), n)
            block[0] = pred
            k = 1
            while k < 64:
                rs = rd.symbol(tables["ac"])
                run, size = rs >> 4, rs & 15
                if size == 0:
                    if run == 0:
                        break
                    if run != 15:
                        raise ValueError("size 0 with run %d" % run)
                    k += 16
                    if k > 63:
                        raise ValueError("run of sixteen past 63")
                    continue
                k += run
                if k > 63:
                    raise ValueError("run past 63")
                block[ZIGZAG[k]] = extend(rd.take(size), size)
                k += 1
        except (EOFError, ValueError):
            return coef, m
        coef[m] = block
    return coef, MCU_PER_PACKET


def idct_np(coef, table):
    """coefficients int[..., 64] (row-major, u vertical) and a quantiser table int[64] -> pixels uint8[..., 8, 8]: dequantised and
    clamped to -2048..2047, the column pass (+1024 >> 11), the row pass (+16384 >> 15), +128, clamped to 0..255"""
    coef = np.asarray(coef, dtype=np.int64)
    F = np.clip(coef * np.asarray(table, dtype=np.int64), -2048, 2047).reshape(coef.shape[:-1] + (8, 8))
    t = (np.einsum("uy,...uv->...yv", IDCT_M, F) + 1024) >> 11
    p = (np.einsum("...yv,vx->...yx", t, IDCT_M) + 16384) >> 15
    return np.clip(p + 128, 0, 255).astype(np.uint8)


def image_header(pkt, apids=IMAGE_APIDS):
    """A source packet's image header as a dict (apid, count, day, ms, us, mcun, q), or None when it is not an image packet: its
    APID is none of `apids`, it has no secondary header, it is shorter than 21 bytes, or mcun is no multiple of 14 up to 182"""
    pkt = bytes(pkt)
    if len(pkt) < IMAGE_HEADER_BYTES + 1:
        return None
    h = packet_header(pkt)
    mcun = pkt[14]
    if h["apid"] not in apids or not h["secondary"] or mcun % MCU_PER_PACKET or mcun > MCU_PER_STRIP - MCU_PER_PACKET:
        return None
    return dict(apid=h["apid"], count=h["count"], day=(pkt[6] << 8) | pkt[7], ms=int.from_bytes(pkt[8:12], "big"),
                us=(pkt[12] << 8) | pkt[13], mcun=mcun, q=pkt[19])


def place(heads, apids=IMAGE_APIDS, period=IMAGE_PERIOD):
    """image headers (image_header's dicts, in getPackets order) -> int64[n]: each packet's strip, or -1 where it is not placed.
    a = the sequence count unwrapped modulo 16384; base = a - mcun / 14 - 14 j for channel j; the first packet's base is the
    origin; strip = (base - origin) / period where that divides and is >= 0; of two packets with one (channel, strip, mcun) the
    later is placed."""
    strips = np.full(len(heads), -1, dtype=np.int64)
    a = prev = origin = None
    owner = {}
    for i, h in enumerate(heads):
        a = h["count"] if a is None else a + (h["count"] - prev) % 16384
        prev = h["count"]
        j = tuple(apids).index(h["apid"])
        base = a - h["mcun"] // MCU_PER_PACKET - MCU_PER_PACKET * j
        if origin is None:
            origin = base
        if base < origin or (base - origin) % period:
            continue
        strips[i] = (base - origin) // period
        key = (j, int(strips[i]), h["mcun"])
        if key in owner:
            strips[owner[key]] = -1
        owner[key] = i
    return strips


def image_packets(packets, apids=IMAGE_APIDS):
    """source packets -> (rows of the image packets among them, their image_header dicts)"""
    rows, heads = [], []
    for i, p in enumerate(packets):
        h = image_header(p, apids)
        if h is not None:
            rows.append(i)
            heads.append(h)
    return rows, heads


def _image_info(rows, heads, strips, mcus):
    info = np.zeros(len(rows), dtype=IMAGE_INFO)
    info["packet"], info["strip"], info["mcus"] = rows, strips, mcus
    for k in ("apid", "mcun", "q", "day", "ms", "us"):
        info[k] = [h[k] for h in heads]
    return info


def image_np(packets, apids=IMAGE_APIDS, period=IMAGE_PERIOD):
    """source packets (bytes, in getPackets order) -> (image uint8[H, 1568, 3], info IMAGE_INFO[m]): every image packet decoded
    (mcus), the placed ones' decoded blocks written into their channel's plane; zero wherever nothing was placed"""
    rows, heads = image_packets(packets, apids)
    strips = place(heads, apids, period)
    height = 8 * (int(strips.max()) + 1) if len(strips) else 0
    img = np.zeros((height, IMAGE_WIDTH, len(apids)), dtype=np.uint8)
    mcus = np.zeros(len(rows), dtype=np.int64)
    for i, (r, h) in enumerate(zip(rows, heads)):
        coef, mcus[i] = jpeg_blocks_np(packets[r][IMAGE_HEADER_BYTES:])
        if strips[i] < 0:
            continue
        pix = idct_np(coef[:mcus[i]], quantiser(h["q"]))
        for m in range(int(mcus[i])):
            x = 8 * (h["mcun"] + m)
            img[8 * strips[i]:8 * strips[i] + 8, x:x + 8, tuple(apids).index(h["apid"])] = pix[m]
    return img, _image_info(rows, heads, strips, mcus)


# ------------------------------------------------------------------ device stage of section 4.16
def jpeg_decode(payloads, q, dst, out, pitch):
    """payloads (bytes each: the packets' entropy-coded data), q and dst per packet (dst: the byte offset in the device uint8 array
    `out` of the packet's top-left pixel, -1: decode without writing), rows `pitch` bytes apart -> mcus int32[n] on the host"""
    n = len(payloads)
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(p) for p in payloads])
    q = np.ascontiguousarray(q, dtype=np.uint8)
    dst = np.ascontiguousarray(dst, dtype=np.int64)
    if len(q) != n or len(dst) != n:
        raise ValueError("jpeg_decode: one q and one dst per packet")
    lim = out.n - 7 * pitch - 8 * MCU_PER_PACKET
    if n and (dst.max() > lim or dst.min() < -1):
        raise ValueError("jpeg_decode: a packet's strip does not fit the output")
    data = DevArray.from_host(np.frombuffer(b"".join(payloads) or b"\0", dtype=np.uint8))
    mcus = DevArray(max(n, 1), np.int32)
    check(lib().dd_lrpt_jpeg(data.ptr, offsets.ctypes.data, q.ctypes.data, dst.ctypes.data, n, pitch, out.ptr, mcus.ptr, None),
          "dd_lrpt_jpeg")
    return mcus.view(0, n).to_host()


def image(packets, apids=IMAGE_APIDS, period=IMAGE_PERIOD, decode=jpeg_decode):
    """image_np's result with the blocks decoded on the device: one dd_lrpt_jpeg call per channel plane, into a plane zeroed on the
    device.  A packet that is not placed is decoded too, for its mcus, and writes nothing.  (`decode`: jpeg_decode, or the caller's
    wrapper of it that keeps the time.)"""
    rows, heads = image_packets(packets, apids)
    strips = place(heads, apids, period)
    height = 8 * (int(strips.max()) + 1) if len(strips) else 0
    img = np.zeros((height, IMAGE_WIDTH, len(apids)), dtype=np.uint8)
    mcus = np.zeros(len(rows), dtype=np.int64)
    for j, apid in enumerate(apids):
        mine = [i for i, h in enumerate(heads) if h["apid"] == apid]
        if not mine:
            continue
        plane = DevArray(max(height * IMAGE_WIDTH, 1), np.uint8)
        check(lib().dd_memset(plane.ptr, 0, plane.nbytes, None), "dd_memset")
        dst = [8 * strips[i] * IMAGE_WIDTH + 8 * heads[i]["mcun"] if strips[i] >= 0 else -1 for i in mine]
        mcus[mine] = decode([packets[rows[i]][IMAGE_HEADER_BYTES:] for i in mine], [heads[i]["q"] for i in mine], dst, plane,
                                 IMAGE_WIDTH)
        img[:, :, j] = plane.view(0, height * IMAGE_WIDTH).to_host().reshape(height, IMAGE_WIDTH)
    return img, _image_info(rows, heads, strips, mcus)
