"""
POCSAG paging: 2-FSK at 512, 1200 or 2400 baud, batches of a frame sync codeword and sixteen BCH(31,21) codewords (beyond the
reference; DESIGN.md section 4.24 defines every stage; device side: dd_pocsag.h): the constants, the block code, a NumPy restatement
`candidates_host` / `batches_host` of the two kernels, the device wrappers over the C entries, `decode`, the chain behind
decode_pocsag, which runs over either set of stages (`DeviceOps`, `HostOps`) so that the host logic is one piece of code for both,
the batch merge, the transmissions, the pages with their numeric and alphanumeric content, and `encode` / `encode_audio`, a
synthesiser.

The audio is the FM discriminator's output in radians per sample, quantised, positioned and summed as for AIS (ais.quantise,
ais.positions, ais.values): bit k of the start t is read around sample floor(t + (k + 0.5) sps), v(t, k) is the sum of the w samples
q around it.  The higher frequency is a 0: a bit is 0 when 32 v > S, S the sum of the sync codeword's 32 values.  A codeword is an
integer whose bit 31 is the first-sent bit.

The format is taken from public descriptions of POCSAG (CCIR Radiopaging Code No. 1, ITU-R M.584); INTEGRATION.md lists the limits.
"""
import math

import numpy as np

from . import _burst
from ._burst import Laps, need
from ._hip import DevArray, check, lib
from .ais import positions, quantise, values  # noqa: F401  (the same quantiser, positions and window sums)

BAUDS = (512, 1200, 2400)
SPS_MIN, SPS_MAX = 4.0, 128.0
W_MAX = 77                            # DD_POCSAG_W_MAX
SLACK_MAX = 8                         # DD_POCSAG_SLACK_MAX
FIX_MAX = 2
WORDS = 17                            # codewords per batch, the sync codeword included
BATCH_BITS = 544
TILE = 256                            # DD_POCSAG_TILE
FSC = 0x7CD215D8                      # the frame sync codeword
IDLE = 0x7A89C197                     # the idle codeword
GEN = 0x769                           # x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1 over bits 31 .. 1
UNCORRECTABLE = 255
OK, OUTSIDE = 0, 1
MIN_GOOD = 12                         # accepted codewords of the 16 that make a batch
FOLLOW_SLACK = 6                      # wrong places a followed batch's sync codeword may hold
PREAMBLE_BITS = 576
DEVIATION = 4500.0
CUT = 7000.0                          # the audio-rate channel filter's cut-off, Hz
NUMERIC = "0123456789*U -]["
FSC_BITS = np.array([(FSC >> (31 - k)) & 1 for k in range(32)], dtype=bool)      # first sent first

_F64 = np.dtype(np.float64)


def params(rate, baud, w=None, slack=2, fix=2):
    """(sps, w, slack, fix) for an audio rate and a baud rate: sps = rate / baud must lie in 4 .. 128; w None: the odd number
    nearest 0.6 sps, at most 77"""
    sps = float(rate) / float(baud) if baud and baud > 0 else float("nan")
    if not SPS_MIN <= sps <= SPS_MAX:              # (also false for a NaN)
        raise ValueError("pocsag: an audio rate of %r S/s at %r baud is %r samples per bit; %g to %g are supported"
                         % (rate, baud, sps, SPS_MIN, SPS_MAX))
    if w is None:
        w = min(W_MAX, 2 * int(math.floor((0.6 * sps - 1.0) / 2.0 + 0.5)) + 1)
    if int(w) != w or not 1 <= w <= W_MAX or not int(w) & 1:
        raise ValueError("pocsag: w must be an odd number from 1 to %d, got %r" % (W_MAX, w))
    if int(slack) != slack or not 0 <= slack <= SLACK_MAX:
        raise ValueError("pocsag: slack must be from 0 to %d, got %r" % (SLACK_MAX, slack))
    if int(fix) != fix or not 0 <= fix <= FIX_MAX:
        raise ValueError("pocsag: fix must be from 0 to %d, got %r" % (FIX_MAX, fix))
    return sps, int(w), int(slack), int(fix)


def reach(sps, w):
    """samples from a start to past the last one its sync codeword reads"""
    return int(math.floor(31.5 * sps)) + w // 2 + 1


def n_starts(n, sps, w):
    return max(0, int(n) - reach(sps, w) + 1)


# ------------------------------------------------------------------------------------------------------------------ the block code
def _ztable():
    z = np.zeros(32, dtype=np.int64)
    v = 1
    for p in range(1, 32):
        z[p] = v
        v <<= 1
        if v & 0x400:
            v ^= GEN
    return z


ZTABLE = _ztable()                    # z[p] = x^(p - 1) mod the generator: the syndrome of a lone error in bit p; z[0] = 0 (parity)


def popcount(words):
    w = np.asarray(words, dtype=np.int64)
    return ((w[..., None] >> np.arange(32)) & 1).sum(axis=-1)


def syndrome(words):
    """the remainder of bits 31 .. 1 modulo the generator: the XOR of the lone-bit remainders of the one bits"""
    w = np.asarray(words, dtype=np.int64)
    s = np.zeros(w.shape, dtype=np.int64)
    for p in range(1, 32):
        s ^= np.where((w >> p) & 1, ZTABLE[p], 0)
    return s if s.ndim else int(s)


def bch_encode(info):
    """the codeword of 21 bits (the flag and the 20 information bits): check bits in 10 .. 1, even parity in bit 0"""
    v = np.asarray(info, dtype=np.int64) << 11
    v = v | (np.asarray(syndrome(v), dtype=np.int64) << 1)
    v = v | (popcount(v) & 1)
    return v if v.ndim else int(v)


def _flip_table():
    """per syndrome: the bits 31 .. 1 to flip (-1: none of one or two bits has it) and how many"""
    mask, count = np.full(1024, -1, dtype=np.int64), np.zeros(1024, dtype=np.int64)
    mask[0] = 0
    for i in range(1, 32):
        mask[ZTABLE[i]], count[ZTABLE[i]] = 1 << i, 1
    for i in range(1, 32):
        for j in range(i + 1, 32):
            s = ZTABLE[i] ^ ZTABLE[j]
            assert mask[s] == -1                   # the 496 syndromes are distinct
            mask[s], count[s] = (1 << i) | (1 << j), 2
    return mask, count


FLIPS, NFLIPS = _flip_table()


def correct(words, fix=2):
    """(the codewords corrected, uint32; the errors repaired, uint8, 255 = uncorrectable): the syndrome of one or two bits flips
    them, odd parity after that flips bit 0 and counts as one more error, and more than `fix` errors leave the codeword as received"""
    w = np.asarray(words, dtype=np.int64)
    s = np.asarray(syndrome(w), dtype=np.int64)
    ok = FLIPS[s] >= 0
    fixed = np.where(ok, w ^ np.maximum(FLIPS[s], 0), w)
    odd = popcount(fixed) & 1
    fixed = np.where(ok & (odd == 1), fixed ^ 1, fixed)
    ne = NFLIPS[s] + odd
    ok = ok & (ne <= fix)
    out, errs = np.where(ok, fixed, w).astype(np.uint32), np.where(ok, ne, UNCORRECTABLE).astype(np.uint8)
    return (out, errs) if w.ndim else (int(out), int(errs))


# ------------------------------------------------------------------------------------------------------------------ the restatement
def sync_of(q, ts, sps, w):
    """(above bool[m, 32], S int64[m], score int64[m]) of the starts ts: above = 32 v > S, which reads 0 in the normal polarity"""
    v = values(q, ts, np.arange(32), sps, w)
    S = v.sum(axis=1).reshape(-1, 1)
    return 32 * v > S, S.reshape(-1), np.abs(32 * v - S).sum(axis=1)


def masks_host(audio, sps, w, slack=2, block=1 << 14):
    """the mask byte of every start: bit 0 pass, bit 1 the inverted sync codeword; uint8[n_starts]"""
    q = quantise(audio)
    total = n_starts(len(q), sps, w)
    out = np.zeros(total, dtype=np.uint8)
    for a in range(0, total, block):
        ts = np.arange(a, min(total, a + block), dtype=np.int64)
        mis = (~sync_of(q, ts, sps, w)[0] != FSC_BITS.reshape(1, -1)).sum(axis=1)
        out[a:a + len(ts)] = np.where(mis <= slack, 1, np.where(32 - mis <= slack, 3, 0))
    return out


def candidates_host(audio, sps, w, slack=2):
    """the ordered starts that pass the sync test, int64"""
    return np.flatnonzero(masks_host(audio, sps, w, slack) & 1).astype(np.int64)


def _empty_det(m=0):
    return {"t": np.zeros(m, np.int64), "words": np.zeros((m, WORDS), np.uint32), "errs": np.zeros((m, WORDS), np.uint8),
            "status": np.full(m, OUTSIDE, np.int32), "polarity": np.zeros(m, np.int32), "good": np.zeros(m, np.int32),
            "mis": np.zeros(m, np.int32), "score": np.zeros(m, np.int64)}


def batches_host(audio, sps, w, fix, ts):
    """the listed starts' batches: a dict of t, words uint32[m, 17], errs uint8[m, 17], status, polarity, good, mis, score"""
    q = quantise(audio)
    n = len(q)
    ts = np.asarray(ts, dtype=np.int64).reshape(-1)
    det = _empty_det(len(ts))
    det["t"] = ts
    weights = (1 << np.arange(31, -1, -1)).astype(np.int64)
    for a in range(0, len(ts), 256):
        idx = a + np.flatnonzero((ts[a:a + 256] >= 0) & (ts[a:a + 256] < n))
        if not len(idx):
            continue
        v = values(q, ts[idx], np.arange(BATCH_BITS), sps, w)
        S = v[:, :32].sum(axis=1).reshape(-1, 1)
        above = 32 * v > S
        far = (~above[:, :32] != FSC_BITS.reshape(1, -1)).sum(axis=1)
        inv = far > 16
        bits = np.where(inv.reshape(-1, 1), above, ~above)
        words = (bits.reshape(len(idx), WORDS, 32) * weights).sum(axis=2)
        fixed, errs = correct(words[:, 1:], fix)
        det["words"][idx, 0], det["words"][idx, 1:] = words[:, 0], fixed
        det["errs"][idx, 0], det["errs"][idx, 1:] = np.where(inv, 32 - far, far), errs
        det["status"][idx], det["polarity"][idx] = OK, inv
        det["good"][idx] = (errs != UNCORRECTABLE).sum(axis=1)
        det["mis"][idx] = np.where(inv, 32 - far, far)
        det["score"][idx] = np.abs(32 * v[:, :32] - S).sum(axis=1)
    return det


# ------------------------------------------------------------------------------------------------------------------ the device stages
def capacity(n, sps):
    """the default list capacity: a clean batch passes at about sps adjacent starts of its 544 sps samples, a share of 1 / 544 of the
    audio when batch follows batch; four times that and 1024"""
    return 1024 + int(n) // 136


def candidates(audio, sps, w, slack=2, cap=None):
    """float64 device audio -> (the survivors as a device int64 array, how many) (dd_pocsag_candidates); a list that proves too
    small is asked for again at the true count"""
    need(audio, _F64, "pocsag.candidates")
    cap = capacity(audio.n, sps) if cap is None else int(cap)
    def call(lst, cap, count):
        return lib().dd_pocsag_candidates(audio.ptr, audio.n, float(sps), int(w), int(slack), lst, cap, count, None)
    return _burst.candidates("dd_pocsag_candidates", cap, call)


def batches(audio, sps, w, fix, lst, m):
    """the first m starts of the device list -> the dict of batches_host, on the host (dd_pocsag_batches)"""
    need(audio, _F64, "pocsag.batches")
    if not isinstance(lst, DevArray):
        lst = DevArray.from_host(np.ascontiguousarray(lst, dtype=np.int64))
    det = _empty_det(m)
    if m == 0 or audio.n == 0:
        return det
    words, errs, meta, score = DevArray(WORDS * m, np.uint32), DevArray(WORDS * m, np.uint8), DevArray(4 * m, np.int32), DevArray(m, np.int64)
    check(lib().dd_pocsag_batches(audio.ptr, audio.n, float(sps), int(w), int(fix), lst.ptr, m, words.ptr, errs.ptr, meta.ptr, score.ptr,
                                  None), "dd_pocsag_batches")
    meta = meta.to_host().reshape(m, 4)
    det.update(t=lst.view(0, m).to_host(), words=words.to_host().reshape(m, WORDS), errs=errs.to_host().reshape(m, WORDS),
               status=meta[:, 0].copy(), polarity=meta[:, 1].copy(), good=meta[:, 2].copy(), mis=meta[:, 3].copy(), score=score.to_host())
    return det


def masks_device(audio, sps, w, slack=2):
    """the mask byte of every sample, uint8[n] on the host, 0 past the last start (dd_debug_pocsag_masks, a diagnostic)"""
    need(audio, _F64, "pocsag.masks_device")
    return _burst.masks("dd_debug_pocsag_masks", audio.n,
                        lambda mask: lib().dd_debug_pocsag_masks(audio.ptr, audio.n, float(sps), int(w), int(slack), mask, None))


class HostOps(Laps):
    """the stages of `decode` in NumPy"""

    def detect(self, audio, sps, w, slack, fix):
        return batches_host(audio, sps, w, fix, candidates_host(audio, sps, w, slack))

    def batches(self, audio, sps, w, fix, ts):
        return batches_host(audio, sps, w, fix, ts)


class DeviceOps(Laps):
    """the stages of `decode` on the device; `laps` collects seconds per stage, with a synchronisation after each"""

    def detect(self, audio, sps, w, slack, fix):
        lst, m = candidates(audio, sps, w, slack)
        self.lap("candidates")
        det = batches(audio, sps, w, fix, lst, m)
        self.lap("batches")
        return det

    def batches(self, audio, sps, w, fix, ts):
        det = batches(audio, sps, w, fix, ts, len(ts))
        self.lap("batches")
        return det


# ------------------------------------------------------------------------------------------------------------------ the host logic
def accepted(det):
    """the candidates that are batches: inside the audio, with at least MIN_GOOD of the 16 codewords accepted"""
    return [int(i) for i in np.flatnonzero((det["status"] == OK) & (det["good"] >= MIN_GOOD))]


def batch_of(det, i, baud, sps, followed=False):
    errs = det["errs"][i]
    return {"t": int(det["t"][i]), "baud": baud, "sps": sps, "words": det["words"][i].copy(), "errs": errs.copy(),
            "polarity": int(det["polarity"][i]), "good": int(det["good"][i]), "mis": int(det["mis"][i]), "score": int(det["score"][i]),
            "corrected": int(errs[1:][errs[1:] != UNCORRECTABLE].sum()), "followed": followed}


def merge(det, sps):
    """The accepted candidates of one baud rate -> (the kept indices in time order, how many duplicates were dropped): candidates
    whose starts lie within one bit time of the group's first are one batch; the one with the fewest corrected bits stays, then the
    largest score, then the earliest."""
    acc = sorted(accepted(det), key=lambda i: (int(det["t"][i]), i))
    t, score = det["t"].tolist(), det["score"].tolist()
    fixed = np.where(det["errs"][:, 1:] != UNCORRECTABLE, det["errs"][:, 1:], 0).sum(axis=1).tolist()
    keep, dup, a = [], 0, 0
    while a < len(acc):
        b = a
        while b < len(acc) and t[acc[b]] - t[acc[a]] <= sps:
            b += 1
        keep.append(min(acc[a:b], key=lambda j: (fixed[j], -score[j], t[j])))
        dup += b - a - 1
        a = b
    return keep, dup


def resolve(found):
    """Batches (batch_of) of several baud rates -> (those that stay, in time order; how many were dropped): of batches of different
    baud rates that overlap in time the one with the fewest corrected bits stays, then the most accepted codewords, then the lower
    baud rate."""
    kept = []
    for b in sorted(found, key=lambda b: (b["corrected"], -b["good"], b["baud"], b["t"])):
        lo, hi = b["t"], b["t"] + BATCH_BITS * b["sps"]
        if not any(k["baud"] != b["baud"] and k["t"] < hi and lo < k["t"] + BATCH_BITS * k["sps"] for k in kept):
            kept.append(b)
    return sorted(kept, key=lambda b: (b["t"], b["baud"])), len(found) - len(kept)


def next_start(t, sps):
    """where the batch behind the one at t starts"""
    return int(math.floor(t + BATCH_BITS * sps))


def _link(txs, sps):
    """transmissions joined where the first batch of one follows the last of another"""
    out = []
    for tx in sorted(txs, key=lambda tx: tx[0]["t"]):
        for prev in out:
            if prev[-1]["polarity"] == tx[0]["polarity"] and abs(tx[0]["t"] - next_start(prev[-1]["t"], sps)) <= 0.5 * sps:
                prev.extend(tx)
                break
        else:
            out.append(list(tx))
    return out


def chain(found, sps, extend=None, follow=0):
    """Batches of one baud rate -> transmissions, lists of batches in time order: a batch of the same polarity whose start lies
    within half a bit time of next_start follows.  Where none does, extend([(predicted start, polarity), ..]) may supply one per
    request or None (a batch whose sync codeword the candidate test lost; its `followed` is True), at most `follow` times in a row;
    every transmission that still lacks a successor is asked for in one call per round."""
    txs = _link([[b] for b in found], sps)
    ended = set()
    while extend is not None:
        ask = [tx for tx in txs if id(tx[-1]) not in ended and sum(1 for b in tx[-follow:] if b["followed"]) < min(follow, len(tx))]
        if not ask:
            break
        got = extend([(next_start(tx[-1]["t"], sps), tx[0]["polarity"]) for tx in ask])
        for tx, b in zip(ask, got):
            if b is None:
                ended.add(id(tx[-1]))
            else:
                tx.append(b)
        txs = _link(txs, sps)
    return txs


def numeric(bits):
    """20-bit fields -> numeric text: four bits per character, the least significant sent first; trailing spaces (the fill) dropped"""
    b = np.asarray(bits, dtype=np.int64).reshape(-1)
    b = b[:len(b) - len(b) % 4].reshape(-1, 4)
    return "".join(NUMERIC[v] for v in (b @ np.array([1, 2, 4, 8])).tolist()).rstrip(" ")


def alpha(bits):
    """20-bit fields -> text: 7-bit characters, the least significant bit sent first, packed without regard to codeword edges; an
    incomplete last character and trailing NUL, ETX and EOT are dropped"""
    b = np.asarray(bits, dtype=np.int64).reshape(-1)
    b = b[:len(b) - len(b) % 7].reshape(-1, 7)
    return "".join(chr(v) for v in (b @ (1 << np.arange(7))).tolist()).rstrip("\x00\x03\x04")


def numeric_bits(text):
    """numeric text -> bits, filled with spaces to whole codewords"""
    vals = [NUMERIC.index(ch) for ch in text]
    vals += [NUMERIC.index(" ")] * (-len(vals) % 5)
    return ((np.array(vals, dtype=np.int64).reshape(-1, 1) >> np.arange(4)) & 1).astype(np.uint8).reshape(-1)


def alpha_bits(text):
    """text -> bits, zero filled to whole codewords"""
    vals = [ord(ch) for ch in text]
    if any(v > 127 for v in vals):
        raise ValueError("pocsag.alpha_bits: 7-bit characters only")
    b = ((np.array(vals, dtype=np.int64).reshape(-1, 1) >> np.arange(7)) & 1).astype(np.uint8).reshape(-1)
    return np.concatenate((b, np.zeros(-len(b) % 20, dtype=np.uint8)))


def _printable(text):
    return all(32 <= ord(ch) < 127 or ch in "\r\n\t" for ch in text)


def _finish(page, fields, content):
    bits = np.array([(f >> (19 - j)) & 1 for f in fields for j in range(20)], dtype=np.uint8)
    page["nbits"], page["bits"] = len(bits), np.packbits(bits).tobytes()
    page["numeric"], page["alpha"] = numeric(bits), alpha(bits)
    if not len(bits):
        kind = "tone"
    elif content in ("numeric", "alpha"):
        kind = content
    elif page["function"] == 0:
        kind = "numeric"
    elif page["function"] == 3 or _printable(page["alpha"]):
        kind = "alpha"
    else:
        kind = "numeric"
    page["kind"], page["text"] = kind, {"tone": "", "numeric": page["numeric"], "alpha": page["alpha"]}[kind]
    return page


def pages(tx, rate, content="auto"):
    """A transmission (its batches in order) -> (pages, counts): the slots are walked in order; an address codeword opens a page; an
    address codeword, an idle codeword or the transmission's end closes it; an uncorrectable codeword closes it with complete False;
    a message codeword with no page open is an orphan.  An address is its 18 bits and the frame its position gives.  counts: the
    codewords by errors repaired, uncorrectable, idle, orphans."""
    out = []
    counts = {"codewords": {0: 0, 1: 0, 2: 0}, "uncorrectable": 0, "idle": 0, "orphans": 0}
    cur, fields = None, []

    def close(complete):
        nonlocal cur, fields
        if cur is not None:
            cur["complete"] = complete
            out.append(_finish(cur, fields, content))
        cur, fields = None, []
    for bi, b in enumerate(tx):
        for slot in range(1, WORDS):
            word, err = int(b["words"][slot]), int(b["errs"][slot])
            if err == UNCORRECTABLE:
                counts["uncorrectable"] += 1
                close(False)
                continue
            counts["codewords"][err] += 1
            if word == IDLE:
                counts["idle"] += 1
                close(True)
            elif not word >> 31:
                close(True)
                start = int(math.floor(b["t"] + 32.0 * slot * b["sps"]))
                cur = {"t": start / float(rate), "start": start, "baud": b["baud"], "polarity": b["polarity"],
                       "address": ((word >> 13) & 0x3FFFF) << 3 | (slot - 1) // 2, "function": (word >> 11) & 3, "corrected": err,
                       "batches": 1, "_last": bi}
            elif cur is None:
                counts["orphans"] += 1
            else:
                fields.append((word >> 11) & 0xFFFFF)
                cur["corrected"] += err
                cur["batches"] += bi != cur["_last"]
                cur["_last"] = bi
    close(True)
    for p in out:
        del p["_last"]
    return out, counts


def line(page):
    """the page as a line of text"""
    what = {"tone": "Tone", "numeric": "Numeric: " + page["numeric"], "alpha": "Alpha: " + page["alpha"]}[page["kind"]]
    return "POCSAG%d: Address: %7d Function: %d %s" % (page["baud"], page["address"], page["function"], what)


def decode(audio, rate, bauds=BAUDS, slack=2, fix=2, follow=2, content="auto", w=None, ops=None):
    """The chain behind decode_pocsag over one channel's audio (a float64 device array for DeviceOps, NumPy for HostOps) at `rate`
    S/s -> (pages in time order, frameInfo, the candidates' dict per baud rate, the batches in time order)."""
    ops = HostOps() if ops is None else ops
    if content not in ("auto", "numeric", "alpha"):
        raise ValueError("pocsag: content must be auto, numeric or alpha, got %r" % (content,))
    if int(follow) != follow or follow < 0:
        raise ValueError("pocsag: follow must be a count from 0 up, got %r" % (follow,))
    grids = {baud: params(rate, baud, w, slack, fix) for baud in bauds}
    n = len(audio)
    info = {"samples": n, "bauds": {}, "overlaps": 0, "batches": 0, "transmissions": 0, "codewords": {0: 0, 1: 0, 2: 0},
            "uncorrectable": 0, "idle": 0, "orphans": 0, "pages": 0}
    cands, found = {}, []
    for baud, (sps, wb, _, _) in grids.items():
        det = ops.detect(audio, sps, wb, slack, fix)
        cands[baud] = det
        keep, dup = merge(det, sps)
        info["bauds"][baud] = {"candidates": len(det["t"]), "accepted": len(keep), "duplicates": dup, "followed": 0}
        found += [batch_of(det, i, baud, sps) for i in keep]
        ops.lap("host")
    found, info["overlaps"] = resolve(found)
    out, kept = [], []
    for baud, (sps, wb, _, _) in grids.items():
        def extend(asks):
            inside = [i for i, (at, _) in enumerate(asks) if 0 <= at < n]
            out = [None] * len(asks)
            if inside:
                d = ops.batches(audio, sps, wb, fix, np.array([asks[i][0] for i in inside], dtype=np.int64))
                for j, i in enumerate(inside):
                    if d["status"][j] == OK and d["polarity"][j] == asks[i][1] and d["mis"][j] <= FOLLOW_SLACK and d["good"][j] >= MIN_GOOD:
                        out[i] = batch_of(d, j, baud, sps, True)
                        info["bauds"][baud]["followed"] += 1
            return out
        for tx in chain([b for b in found if b["baud"] == baud], sps, extend, follow):
            got, counts = pages(tx, rate, content)
            out += got
            kept += tx
            info["transmissions"] += 1
            for key in ("uncorrectable", "idle", "orphans"):
                info[key] += counts[key]
            for e in (0, 1, 2):
                info["codewords"][e] += counts["codewords"][e]
        ops.lap("host")
    out.sort(key=lambda p: (p["start"], p["baud"]))
    kept.sort(key=lambda b: (b["t"], b["baud"]))
    info["batches"], info["pages"] = len(kept), len(out)
    return out, info, cands, kept


# ------------------------------------------------------------------------------------------------------------------ the synthesiser
def address_word(address, function):
    """the address codeword: the address's upper 18 bits and the function (the low three bits are the frame it is sent in)"""
    return bch_encode(((int(address) >> 3) & 0x3FFFF) << 2 | (int(function) & 3))


def message_words(bits):
    """bits (a multiple of 20) -> message codewords"""
    b = np.asarray(bits, dtype=np.int64).reshape(-1, 20)
    return [bch_encode((1 << 20) | int(v)) for v in b @ (1 << np.arange(19, -1, -1))]


def page_bits(text, kind):
    if kind == "tone":
        return np.zeros(0, dtype=np.uint8)
    return numeric_bits(text) if kind == "numeric" else alpha_bits(text)


def transmission_words(paging):
    """Pages (address, function, text[, kind]) -> uint32[batches, 17]: each address codeword goes into the next slot of the frame
    its low three bits name, its message follows across frames and batches, idle codewords fill the rest.  kind None: numeric for
    function 0, else alpha."""
    slots = []
    for page in paging:
        address, function, text = page[:3]
        kind = page[3] if len(page) > 3 and page[3] else ("numeric" if function == 0 else "alpha")
        while (len(slots) % 16) // 2 != (int(address) & 7):
            slots.append(IDLE)
        slots.append(address_word(address, function))
        slots += message_words(page_bits(text, kind))
    slots += [IDLE] * (-len(slots) % 16 if slots else 16)
    body = np.array(slots, dtype=np.int64).reshape(-1, 16)
    return np.concatenate((np.full((len(body), 1), FSC, dtype=np.int64), body), axis=1).astype(np.uint32)


def transmission_bits(words, preamble=PREAMBLE_BITS, flips=None):
    """the bits on the air: `preamble` bits 1010.., then the codewords, bit 31 first; flips {(batch, codeword): XOR mask} spoils
    codewords on their way"""
    w = np.array(words, dtype=np.int64).reshape(-1, WORDS)
    for (b, c), mask in (flips or {}).items():
        w[b, c] ^= int(mask)
    bits = (w.reshape(-1, 1) >> np.arange(31, -1, -1)) & 1
    return np.concatenate(((np.arange(preamble) + 1) & 1, bits.reshape(-1))).astype(np.uint8)


def frequency(bits, rate, baud, start, n, polarity=0):
    """(float64[n] instantaneous frequency in Hz of the transmission that starts at the fractional sample `start`, float64[n] its
    envelope): a 0 is +4500 Hz and a 1 is -4500 Hz (the other way round for polarity 1), each transition smoothed over about a
    quarter of a bit; the envelope rises over the first two bits of the preamble and falls over two bit times of bare carrier behind
    the last bit"""
    spb = rate / float(baud)
    pos = (np.arange(n, dtype=np.float64) - start) / spb
    idx = np.floor(pos).astype(np.int64)
    on = (idx >= 0) & (idx < len(bits))
    lv = (1.0 - 2.0 * np.asarray(bits, dtype=np.float64)) * (-1.0 if polarity else 1.0)
    sq = np.where(on, lv[np.clip(idx, 0, len(bits) - 1)], 0.0)
    L = max(1, int(round(spb / 4.0)))
    f = np.convolve(sq, np.ones(L) / L, mode="same") * DEVIATION
    env = np.clip(np.minimum(pos / 2.0, (len(bits) + 2.0 - pos) / 2.0), 0.0, 1.0)
    return f, env


def _plan(transmissions, rate, starts, bauds, polarities, carrier_offsets, preamble, flips, n):
    starts = np.atleast_1d(np.asarray(starts, dtype=np.float64))
    if len(transmissions) != len(starts):
        raise ValueError("pocsag.encode: one start per transmission")
    bauds = np.broadcast_to(np.asarray(bauds), starts.shape)
    pols = np.broadcast_to(np.asarray(polarities), starts.shape)
    offs = np.broadcast_to(np.asarray(carrier_offsets, dtype=np.float64), starts.shape)
    pres = np.broadcast_to(np.asarray(preamble), starts.shape)
    flips = flips if flips is not None else [None] * len(starts)
    plan = []
    for tx, s, baud, pol, off, pre, fl in zip(transmissions, starts, bauds, pols, offs, pres, flips):
        bits = transmission_bits(transmission_words(tx), int(pre), fl)
        lo = max(int(math.floor(s)) - 1, 0)
        plan.append((bits, float(s), int(baud), int(pol), float(off), lo, lo + int(math.ceil((len(bits) + 2) * rate / float(baud))) + 4))
    if n is None:
        n = max([p[6] for p in plan] + [0])
    return plan, int(n)


def batch_start(rate, baud, start, batch=0, preamble=PREAMBLE_BITS):
    """the fractional sample at which batch `batch` of a transmission encoded at `start` begins"""
    return start + (preamble + BATCH_BITS * batch) * rate / float(baud)


def encode(transmissions, rate, starts, bauds=1200, polarities=0, offset=0.0, amplitudes=40.0, sigma=0.0, seed=0, carrier_offsets=0.0,
           n=None, preamble=PREAMBLE_BITS, flips=None):
    """A recording uint8[n, 2] at `rate` S/s that holds one transmission per list of pages (transmission_words) from the fractional
    samples `starts` on, at its baud rate and polarity: 2-FSK of +-4500 Hz around `offset` plus its carrier error (Hz), from a seeded
    random phase; Gaussian noise of `sigma` per rail; the u8 value is clip(rint(z + 127.5), 0, 255).  flips: per transmission None or
    {(batch, codeword): XOR mask}.  bauds, polarities, amplitudes, carrier_offsets and preamble: one value, or one per transmission.
    n None: long enough for the last transmission."""
    plan, n = _plan(transmissions, rate, starts, bauds, polarities, carrier_offsets, preamble, flips, n)
    amps = np.broadcast_to(np.asarray(amplitudes, dtype=np.float64), (len(plan),))
    rng = np.random.default_rng(seed)
    z = np.zeros(n, dtype=np.complex128)
    for (bits, s, baud, pol, off, lo, hi), a in zip(plan, amps):
        hi = min(n, hi)
        if hi <= lo:
            continue
        f, env = frequency(bits, rate, baud, s - lo, hi - lo, pol)
        phase = rng.uniform(0.0, 2.0 * np.pi) + 2.0 * np.pi * np.cumsum(f + offset + off) / rate
        z[lo:hi] += a * env * np.exp(1j * phase)
    v = np.stack((z.real, z.imag), axis=1) + rng.normal(0.0, 1.0, (n, 2)) * sigma + 127.5
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def encode_audio(transmissions, rate, starts, bauds=1200, polarities=0, sigma=0.0, seed=0, carrier_offsets=0.0, n=None,
                 preamble=PREAMBLE_BITS, flips=None):
    """The discriminator's view of `encode` without the radio: float64[n] audio at `rate` S/s in radians per sample,
    2 pi (f + carrier error) / rate inside a transmission and 0 outside, plus Gaussian noise of `sigma` radians"""
    plan, n = _plan(transmissions, rate, starts, bauds, polarities, carrier_offsets, preamble, flips, n)
    x = np.zeros(n)
    for bits, s, baud, pol, off, lo, hi in plan:
        hi = min(n, hi)
        if hi <= lo:
            continue
        f, env = frequency(bits, rate, baud, s - lo, hi - lo, pol)
        x[lo:hi] += 2.0 * np.pi * (f + off * (env > 0)) / rate
    if sigma:
        x = x + np.random.default_rng(seed).normal(0.0, sigma, n)
    return x


# ------------------------------------------------------------------------------------------------------------------ the front end, restated
def audio_host(raw, fs, offset, bw=48000.0, cut=CUT):
    """(float64 audio, its rate) of the channel at `offset` Hz of a uint8[N, 2] recording in float64 NumPy: decode_pocsag's front end
    restated, which is decode_ais's for one channel (ais.audio_host).  The device's float32 stages round differently: this is the
    same chain, not the same bits."""
    from . import ais
    return ais.audio_host(raw, fs, offset, bw, cut)
