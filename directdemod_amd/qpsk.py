"""
Meteor-M2 QPSK sync detection stages -- the reference's decode_meteorm2.getSyncs (decode_meteorm2.py:229-324), a Python loop over
every IQ sample there.  Device stages (dd_meteor.h; what the Funcube decoder shares is in symbolsync.py and dd_symbol_walk.h): the
Gardner / agc / costas walk (`Walker`, configured here), the per-sample lim values (`Walker.lim`), the MINSYNC candidates
(`minsync_candidates`) and the MAXSYNC correlations (`maxsync_argmax`).  Host stages: the MINSYNC gating scan (`minsync_scan`) and
the correlation-buffer bookkeeping (`maxsync_buffers`), both O(syncs); NumPy restatements of the device arithmetic (`lim`, `limBin`,
`correlate_same_blocks`) for the tests.
"""
import numpy as np

from . import symbolsync
from .symbolsync import _STATE, hyp_table, lim, limBin, mix  # noqa: F401  (the names this module has always offered)
from .symbolsync import interval_descriptors, maxcorr, minsync_fired

SYMBOL_RATE = 72000
COSTAS_BW = 0.008727
REP = int(2048000 / 72000)              # np.repeat count of the 2 MHz templates (decode_meteorm2.py:189), whatever the rate
NSYNC = 120
MIN_GAP = 0.1 * 72000                   # the MINSYNC gating, in symbols (7200.0)
COLLECT_LEAD = 2 * NSYNC                # the MAXSYNC pre-buffer starts 240 symbols before the gate
COLLECT_SPAN = 1 * 72000
SYNC = "0, 13, 13, 12, 13, 13, 13, 0, 0, 0, 13, 13, 0, 13, 13, 0, 13, 0, 0, 0, 13, 13, 13, 0, 0, 13, 0, 13, 0, 13, 0, 13, 13, 0, 0, 0, " \
       "13, 13, 0, 0, 0, 0, 13, 0, 13, 13, 0, 0, 0, 0, 0, 13, 1, 13, 0, 13, 13, 13, 13, 12, 0, 13, 0, 13, 0, 0, 13, 0, 13, 0, 13, " \
       "13, 0, 13, 13, 13, 0, 0, 0, 0, 13, 0, 13, 0, 13, 13, 13, 13, 13, 0, 13, 13, 13, 0, 0, 0, 0, 13, 13, 13, 0, 13, 0, 0, 0, 13, " \
       "0, 13, 13, 0, 13, 0, 13, 13, 0, 0, 0, 13, 13, 13"


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


def costas_coefficients(damping=0.70710678118, bw=COSTAS_BW):
    """costas.compAlphaBeta for bw and bw / 2: (alpha, beta, alpha_locked, beta_locked)"""
    return symbolsync.costas_coefficients(bw, damping)


class Walker(symbolsync.Walker):
    """symbolsync.Walker for decode_meteorm2: `lim_values` = the int8 (re, im) pair of every sample fed.  Device memory: about 8 GB
    of symbols and 2.5 GB of lim values for a 10-minute pass at 2.048 MS/s."""
    SYMBOL_RATE = SYMBOL_RATE
    COSTAS_BW = COSTAS_BW
    AMEAN0 = 3.0
    LIM_DTYPE = np.int16
    WALK, LIM = "dd_meteor_walk", "dd_meteor_lim"
    LABEL = "meteor"


def minsync_candidates(w, cap=1 << 20):
    """symbols k >= 59 whose contiguous 60-symbol window fires either score: int64[m, 3] = (k, mismatches1, mismatches2), sorted;
    and the device array of the symbols' bits (limBin(re) | limBin(im) << 1)"""
    s72, s1, _ = sync_patterns()
    return minsync_fired("dd_meteor_minsync", w, np.concatenate((s72, s1)), 3, cap, "meteor MINSYNC: %d candidate windows")


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
    desc = interval_descriptors(bufs, lambda buf, _: buf[2])
    s72, _, s2 = sync_patterns()
    tt = np.ascontiguousarray(np.stack([np.where(s72 == 1, 127, -128), np.where(s2 == 1, 127, -128)]), dtype=np.int8)
    return maxcorr("dd_meteor_maxcorr", lim_values, desc, tt.ctypes.data)
