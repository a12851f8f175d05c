"""
Meteor-M2 QPSK sync detection stages -- the reference's decode_meteorm2.getSyncs (decode_meteorm2.py:229-324), a Python loop over
every IQ sample there.  Device stages (dd_meteor.h): the Gardner / agc / costas walk (`Walker`), the per-sample lim values
(`Walker.lim`), the MINSYNC candidates (`minsync_candidates`) and the MAXSYNC correlations (`maxsync_argmax`).  Host stages: the
MINSYNC gating scan (`minsync_scan`) and the correlation-buffer bookkeeping (`maxsync_buffers`), both O(syncs); NumPy
restatements of the device arithmetic (`lim`, `limBin`, `correlate_same_blocks`) for the tests.
"""
import ctypes as C

import numpy as np

from . import _hip
from ._hip import DevArray, check, lib

SYMBOL_RATE = 72000
REP = int(2048000 / 72000)              # np.repeat count of the 2 MHz templates (decode_meteorm2.py:189), whatever the rate
NSYNC = 120
MIN_GAP = 0.1 * 72000                   # the MINSYNC gating, in symbols (7200.0)
COLLECT_LEAD = 2 * NSYNC                # the MAXSYNC pre-buffer starts 240 symbols before the gate
COLLECT_SPAN = 1 * 72000
SYNC = "0, 13, 13, 12, 13, 13, 13, 0, 0, 0, 13, 13, 0, 13, 13, 0, 13, 0, 0, 0, 13, 13, 13, 0, 0, 13, 0, 13, 0, 13, 0, 13, 13, 0, 0, 0, " \
       "13, 13, 0, 0, 0, 0, 13, 0, 13, 13, 0, 0, 0, 0, 0, 13, 1, 13, 0, 13, 13, 13, 13, 12, 0, 13, 0, 13, 0, 0, 13, 0, 13, 0, 13, " \
       "13, 0, 13, 13, 13, 0, 0, 0, 0, 13, 0, 13, 0, 13, 13, 13, 13, 13, 0, 13, 13, 13, 0, 0, 0, 0, 13, 13, 13, 0, 13, 0, 0, 0, 13, " \
       "0, 13, 13, 0, 13, 0, 13, 13, 0, 0, 0, 13, 13, 13"


def lim(x):
    """decode_meteorm2.lim: clamp to [-128, 127], (0, 1) -> 1, (-1, 0) -> -1, else int(x)"""
    if x < -128.0:
        return -128
    if x > 127.0:
        return 127
    if x > 0 and x < 1:
        return 1
    if x > -1 and x < 0:
        return -1
    return int(x)


def limBin(x):
    """decode_meteorm2.limBin: 0 for x <= 0, else 1"""
    if x <= 0:
        return 0
    else:
        return 1


def sync_patterns():
    """(sync72khz, sync72khz1, sync72khz2) as int64 0/1 arrays (decode_meteorm2.py:163-189)"""
    s = np.array([int(i) for i in SYNC.split(",")])
    s72 = (s >= 7).astype(np.int64)
    alt = np.arange(NSYNC) % 2
    s1 = np.where(alt == 0, s72, 1 - s72)
    s2 = np.where(alt == 1, s72, 1 - s72)
    return s72, s1, s2


def templates():
    """(sync2mhz, sync2mhz1, sync2mhz2): the patterns as 127 / -128, each value repeated 28 times (decode_meteorm2.py:191-204)"""
    return tuple(np.repeat(np.where(p == 1, 127, -128).astype(np.int64), REP) for p in sync_patterns())


def correlate_same_blocks(buf, t):
    """np.correlate(buf, np.repeat(t, 28), 'same') through 28-sample block sums: 120 terms per lag (what dd_meteor_maxcorr
    computes, in NumPy integers)"""
    buf = np.asarray(buf, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    L, tl = len(buf), len(t) * REP
    pad = np.zeros(L + 2 * tl, dtype=np.int64)
    pad[tl // 2:tl // 2 + L] = buf
    P = np.concatenate(([0], np.cumsum(pad)))
    W = P[REP:] - P[:-REP]                      # W[q] = sum of pad[q .. q+27]
    idx = np.arange(L)[:, None] + REP * np.arange(len(t))[None, :]
    return W[idx] @ t


def costas_coefficients(damping=0.70710678118, bw=0.008727):
    """costas.compAlphaBeta for bw and bw / 2: (alpha, beta, alpha_locked, beta_locked)"""
    def ab(d, b):
        denom = (1.0 + 2.0 * d * b + b * b)
        return (4 * d * b) / denom, (4 * b * b) / denom
    return ab(damping, bw) + ab(damping, bw / 2.0)


def hyp_table():
    """costas.hypstore: np.tanh(i - 128) for i in 0..255"""
    return np.array([np.tanh(i - 128) for i in range(256)], dtype=np.float64)


# DDMeteorState (dd_meteor.h)
_STATE = np.dtype([(f, np.float64) for f in ("timing", "b_re", "b_im", "c_re", "c_im", "dc_re", "dc_im", "amean", "freq", "phase",
                                             "pmean", "alpha", "beta")] + [(f, np.int64) for f in ("lock", "ctr", "bidx", "overflow")])


class Walker:
    """The symbol walk over a recording of `total` samples at `fs`, fed chunk by chunk in order (`walk`, then `lim`).  Per symbol k (device
    arrays, `nsym` long once fed): bidx, aidx (sample indices of the B and A samples), agc (agc.adjust of A, gardnerC), ph (the
    costas phasor active after the step), sym (the corrected symbol, gardnerA after pllObj.loop), pf ((phase, freq) after the step);
    `lim_values` = the int8 (re, im) pair of every sample fed.

    Device memory: room for total / (P / 2) symbols -- twice the nominal count -- at 96 B each, plus 2 B per sample of lim values:
    about 8 GB and 2.5 GB for a 10-minute pass at 2.048 MS/s.  A recording whose timing runs faster than one symbol per P / 2
    samples (the reference would keep decoding) raises RuntimeError."""

    def __init__(self, fs, total):
        _hip.require_gpu()
        P = fs / 72000
        a0, b0, a1, b1 = costas_coefficients()
        self.params = np.ascontiguousarray(np.concatenate(([P, P / 2, (P / 2) + 1, a0, b0, a1, b1], hyp_table())), dtype=np.float64)
        st = np.zeros(1, dtype=_STATE)
        st["amean"], st["freq"], st["pmean"], st["alpha"], st["beta"] = 3.0, 0.001, 1.0, a0, b0
        self.state = DevArray.from_host(st.view(np.uint8))
        self.total = int(total)
        self.cap = int(total / (P / 2)) + 64             # a symbol takes at least P/2 samples unless timing is thrown far
        cap = max(self.cap, 1)
        self.bidx, self.aidx = DevArray(cap, np.int64), DevArray(cap, np.int64)
        self.agc, self.ph, self.sym, self.pf = (DevArray(cap, np.complex128) for _ in range(4))
        self.lim_values = DevArray(max(self.total, 1), np.int16)    # int8 pairs
        self.fed = 0
        self.nsym = 0

    def _state(self):
        return self.state.to_host().view(_STATE)[0]

    def walk(self, x):
        """the symbol walk over the next chunk"""
        if x.dtype != np.dtype(np.complex128):
            raise TypeError("complex128 device array expected, got %s" % x.dtype)
        if self.fed + x.n > self.total:
            raise ValueError("more samples than the recording holds")
        dp = C.POINTER(C.c_double)
        P64 = C.POINTER(C.c_int64)
        check(lib().dd_meteor_walk(x.ptr, x.n, self.fed, self.state.ptr, self.params.ctypes.data_as(dp), self.cap,
                                   C.cast(self.bidx.ptr, P64), C.cast(self.aidx.ptr, P64), self.agc.ptr, self.ph.ptr, self.sym.ptr,
                                   self.pf.ptr, None), "dd_meteor_walk")
        st = self._state()
        if st["overflow"]:
            raise RuntimeError("meteor walk: more symbols than %d (timing thrown by the input)" % self.cap)
        self.nsym = int(st["ctr"])

    def lim(self, x):
        """the lim values of the chunk just walked (its samples take the phasors of the symbols walked so far)"""
        P64 = C.POINTER(C.c_int64)
        check(lib().dd_meteor_lim(x.ptr, x.n, self.fed, C.cast(self.aidx.ptr, P64), self.nsym, self.ph.ptr, self.lim_values.ptr,
                                  self.total, None), "dd_meteor_lim")
        self.fed += x.n

    def view(self, name):
        return getattr(self, name).view(0, self.nsym)


def mix(x, fs, offset):
    """commSignal.offsetFreq(offset) with the reference's arithmetic (dd_meteor_mix): raw u8 pairs (_hip.IQ8) or complex64 in,
    complex64 out.  The reference restarts the mixer phase in every chunk (no chunker reaches the signal), so k counts from 0."""
    if x.dtype == _hip.IQ8:
        raw, c64 = x.ptr, None
    elif x.dtype == np.dtype(np.complex64):
        raw, c64 = None, x.ptr
    else:
        raise TypeError("raw u8 pairs or complex64 expected, got %s" % x.dtype)
    out = DevArray(x.n, np.complex64)
    w = -1.0j * 2.0 * np.pi * offset                     # comm.py:77's operation order: the imaginary part is -2 pi f
    check(lib().dd_meteor_mix(raw, c64, x.n, float(w.imag), 1.0 / fs, out.ptr, None), "dd_meteor_mix")
    return out


def minsync_candidates(w, cap=1 << 20):
    """symbols k >= 59 whose contiguous 60-symbol window fires either score: int64[m, 3] = (k, mismatches1, mismatches2), sorted;
    and the device array of the symbols' bits (limBin(re) | limBin(im) << 1)"""
    nsym = w.nsym
    bits = DevArray(max(nsym, 1), np.uint8)
    if nsym == 0:
        return np.zeros((0, 3), dtype=np.int64), bits
    s72, s1, _ = sync_patterns()
    sb = np.ascontiguousarray(np.concatenate((s72, s1)), dtype=np.uint8)
    cand = DevArray(3 * cap, np.int64)
    cnt = DevArray(1, np.uint64)
    check(lib().dd_meteor_minsync(w.sym.ptr, nsym, sb.ctypes.data, bits.ptr, cap, cand.ptr, cnt.ptr, None), "dd_meteor_minsync")
    m = int(cnt.to_host()[0])
    if m > cap:
        raise RuntimeError("meteor MINSYNC: %d candidate windows, more than %d" % (m, cap))
    c = cand.view(0, 3 * m).to_host().reshape(m, 3) if m else np.zeros((0, 3), dtype=np.int64)
    return c[np.argsort(c[:, 0], kind="stable")], bits


_S72, _S1, _S2 = sync_patterns()


def _scores(bits_pairs):
    """(mismatches1, mismatches2) of a 60-symbol window given as (re, im) bit pairs"""
    re, im = bits_pairs[:, 0], bits_pairs[:, 1]
    b1 = np.stack((re, im), axis=1).ravel()
    b2 = np.stack((im, re), axis=1).ravel()
    return int(np.sum(np.abs(b1 - _S72))), int(np.sum(np.abs(b2 - _S1)))


def _fires(m):
    return abs(m - NSYNC / 2) > 30


def minsync_scan(cands, nsym, fetch_bits):
    """The reference's MINSYNC loop (decode_meteorm2.py:280-318) over the candidate list: bits are appended only for symbols past
    lastMin + 7200, so the 59 windows after each gap still hold bits from before it; those windows are recomputed here from the
    appended symbols (fetch_bits(lo, hi) -> int array of (re, im) pairs of symbols lo..hi-1).  -> [(symbol k, template)], ctr =
    k + 1 in the reference's terms; template 0 = sync2mhz (buff1corr fired), 1 = sync2mhz2 (buff4corr fired, which wins)."""
    events = []
    tail = None                                  # (indices, bits) of the last <= 60 appended symbols, when the window is not contiguous
    last = None
    ci = 0
    while True:
        if last is None:
            lo = NSYNC // 2 - 1
        else:
            g = int(last + MIN_GAP)              # first symbol index k with k + 1 > lastMin + 7200
            hit = None
            if g < nsym:
                hi = min(g + NSYNC // 2 - 1, nsym)
                new = fetch_bits(g, hi)
                idx, bb = tail
                for r in range(hi - g):
                    win = np.concatenate((bb[len(bb) - (NSYNC // 2 - 1 - r):], new[:r + 1]))
                    m1, m2 = _scores(win)
                    if _fires(m1) or _fires(m2):
                        hit = (g + r, m1, m2)
                        tail = (None, win)
                        break
            if hit is not None:
                k, m1, m2 = hit
                events.append((k, 1 if _fires(m2) else 0))
                last = k + 1
                continue
            lo = g + NSYNC // 2 - 1
        while ci < len(cands) and cands[ci, 0] < lo:
            ci += 1
        if ci >= len(cands):
            break
        k, m1, m2 = (int(v) for v in cands[ci])
        events.append((k, 1 if _fires(m2) else 0))
        last = k + 1
        tail = (None, fetch_bits(k - (NSYNC // 2 - 1), k + 1))
    return events


def maxsync_buffers(events, total, a_at, nsym):
    """The MAXSYNC buffer bookkeeping (decode_meteorm2.py:248-274) for the MINSYNC events [(k, template)]: a_at(k) = the sample
    of symbol k's A (k < nsym).  -> per correlation that runs: (intervals [(lo, n), ...], maxBuffStart, template).
    After the MINSYNC of symbol k (sample s = a_at(k), ctr m = k + 1) the next 6721 samples are appended untrimmed and the 6721st
    triggers the correlation.  Between syncs, samples with m + 6960 < ctr <= m + 72000 are collected, trimmed to the last 3360;
    after a fade (ctr past m + 72000) that stale window stays and the next sync's samples are appended to it."""
    out = []
    pre = []                                      # pending buffer: [(lo, n)]
    prev_m = None
    for k, tm in events:
        s = int(a_at(k))
        if prev_m is not None:
            j0 = int(a_at(prev_m + int(MIN_GAP - COLLECT_LEAD))) + 1      # first sample with ctr > lastMin + 6960
            kend = prev_m + COLLECT_SPAN
            ce = min(s, int(a_at(kend))) if kend < nsym else s           # last sample with ctr <= lastMin + 72000, up to s
            lo = max(j0, ce - (REP * NSYNC) + 1)
            pre = [(lo, ce - lo + 1)] if ce >= lo else []
        e = s + 2 * REP * NSYNC + 1                                      # the sample where maxBuffRetain reaches 0
        if e >= total:
            break
        ivs = pre + [(s + 1, 2 * REP * NSYNC + 1)]
        if len(ivs) == 2 and ivs[0][0] + ivs[0][1] == ivs[1][0]:
            ivs = [(ivs[0][0], ivs[0][1] + ivs[1][1])]
        out.append((ivs, ivs[0][0], tm))
        pre = []
        prev_m = k + 1
    return out


def maxsync_argmax(lim_values, bufs):
    """[(intervals, start, template)] -> int64[n, 2] = (argmax, max) of |np.correlate(buffer, template, 'same')| on the device"""
    n = len(bufs)
    out = np.zeros((n, 2), dtype=np.int64)
    if n == 0:
        return out
    desc = np.zeros((n, 5), dtype=np.int64)
    for i, (ivs, _, tm) in enumerate(bufs):
        if len(ivs) > 2:
            raise ValueError("a correlation buffer spans at most two sample intervals")
        (lo0, n0), (lo1, n1) = (ivs + [(0, 0)])[:2]
        desc[i] = (lo0, n0, lo1, n1, tm)
    _, _, s2 = sync_patterns()
    s72 = sync_patterns()[0]
    tt = np.ascontiguousarray(np.stack([np.where(s72 == 1, 127, -128), np.where(s2 == 1, 127, -128)]), dtype=np.int8)
    d = DevArray(2 * n, np.int64)
    check(lib().dd_meteor_maxcorr(lim_values.ptr, lim_values.n, desc.ctypes.data, n, tt.ctypes.data, d.ptr, None), "dd_meteor_maxcorr")
    return d.to_host().reshape(n, 2)
