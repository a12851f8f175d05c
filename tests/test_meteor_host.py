"""Meteor-M2 sync detection, host side: the synthesised recordings' hashes, lim / limBin, the sync patterns and templates, the
block-sum correlation against np.correlate, the MINSYNC gating scan against a direct restatement of the reference's loop, and the
MAXSYNC buffer model against the buffers the reference built (tests/golden/meteor_*.npz, tools/gen_golden.py --meteor)."""
import os

import numpy as np
import pytest

import _meteor
from _symbolwalk import skip as _skip
from directdemod_amd import qpsk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(_meteor.CASES)


def _load(name):
    return np.load(os.path.join(GOLDEN, "meteor_%s.npz" % name))


def _a_idx(g):
    if int(g["nsym"]) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate(([int(g["a_first"])], int(g["a_first"]) + np.cumsum(g["a_diff"].astype(np.int64))))


@pytest.mark.parametrize("name", NAMES)
def test_synthesis_hash(name):
    raw, off = _meteor.case(name)
    g = _load(name)
    assert _meteor.sha256(raw) == str(g["sha256"]), "synthesis drift (NumPy build), not a decoder bug"
    assert raw.shape[0] == int(g["n"]) and off == int(g["offset"])


def test_lim_limbin():
    cases = [(-1e9, -128), (-128.5, -128), (-128.0, -128), (-127.9, -127), (-1.0, -1), (-0.5, -1), (-1e-300, -1), (0.0, 0),
             (-0.0, 0), (1e-300, 1), (0.999, 1), (1.0, 1), (1.5, 1), (2.7, 2), (126.99, 126), (127.0, 127), (127.5, 127), (1e9, 127)]
    for x, want in cases:
        assert qpsk.lim(x) == want, x
        assert type(qpsk.lim(np.float64(x))) is int
    for x, want in [(-1.0, 0), (0.0, 0), (-0.0, 0), (1e-300, 1), (5.0, 1)]:
        assert qpsk.limBin(x) == want
    from directdemod_amd import decode_meteorm2
    assert decode_meteorm2.lim is qpsk.lim and decode_meteorm2.limBin is qpsk.limBin


def test_sync_patterns_and_templates():
    s72, s1, s2 = qpsk.sync_patterns()
    assert s72.tolist() == _meteor.sync_bits().tolist() and len(s72) == 120
    assert (s72[0], s72[1], s72[2], s72[52]) == (0, 1, 1, 0)          # "0, 13, 13, ..." and the lone "1" stays 0
    k = np.arange(120)
    assert np.array_equal(s1[k % 2 == 0], s72[k % 2 == 0]) and np.array_equal(s1[k % 2 == 1], 1 - s72[k % 2 == 1])
    assert np.array_equal(s2[k % 2 == 1], s72[k % 2 == 1]) and np.array_equal(s2[k % 2 == 0], 1 - s72[k % 2 == 0])
    t0, t1, t2 = qpsk.templates()
    for t, p in ((t0, s72), (t1, s1), (t2, s2)):
        assert len(t) == 3360 and set(np.unique(t).tolist()) == {-128, 127}
        assert np.array_equal(t[::28], np.where(p == 1, 127, -128)) and np.array_equal(t.reshape(120, 28), np.repeat(t[::28, None], 28, 1))


@pytest.mark.parametrize("L", [13442, 20162])
def test_block_correlation_matches_numpy(L):
    rng = np.random.default_rng(L)
    s72, _, s2 = qpsk.sync_patterns()
    for pat in (s72, s2):
        t = np.where(pat == 1, 127, -128)
        for buf in (rng.integers(-128, 128, L), rng.integers(-1, 2, L), np.zeros(L, dtype=np.int64)):
            ref = np.correlate(list(buf), np.repeat(t, 28), mode="same")
            got = qpsk.correlate_same_blocks(buf, t)
            assert np.array_equal(got, ref)
            assert int(np.argmax(np.abs(got))) == int(np.argmax(np.abs(ref)))     # first maximum, ties (the zero buffer) included


def _reference_minsync(bits):
    """decode_meteorm2.py:289-318 over per-symbol (re, im) bits: the MINSYNC ctr values and chosen templates"""
    s72, s1, _ = qpsk.sync_patterns()
    b1, b2, last, out = [], [], None, []
    for k in range(len(bits)):
        ctr = k + 1
        if last is None or ctr > last + 0.1 * 72000:
            b1 += [bits[k, 0], bits[k, 1]]
            b1 = b1[-120:]
            b2 += [bits[k, 1], bits[k, 0]]
            b2 = b2[-120:]
            c1 = c4 = 0
            if len(b1) == 120:
                c1 = np.abs(np.sum(np.abs(np.array(b1) - s72)) - 60)
                c4 = np.abs(np.sum(np.abs(np.array(b2) - s1)) - 60)
            if c1 > 30 or c4 > 30:
                out.append((ctr, 1 if c4 > 30 else 0))
                last = ctr
    return out


def test_minsync_scan_matches_reference_loop():
    rng = np.random.default_rng(5)
    n = 40000
    bits = rng.integers(0, 2, (n, 2))
    s72, s1, _ = qpsk.sync_patterns()
    pat0 = s72.reshape(60, 2)
    pat4 = s1.reshape(60, 2)[:, ::-1]                   # (im, re) = sync72khz1: fires buff4corr
    pos = [(100, pat0), (7600, pat4), (14830, pat0), (22500, pat0), (29740, pat4), (37000, 1 - pat0)]   # two straddle a gate
    for p, pat in pos:
        bits[p:p + 60] = pat
    want = _reference_minsync(bits)
    cands = []
    for k in range(59, n):
        w = bits[k - 59:k + 1]
        m1, m2 = qpsk._scores(w)
        if qpsk._fires(m1) or qpsk._fires(m2):
            cands.append((k, m1, m2))
    cands = np.array(cands, dtype=np.int64).reshape(-1, 3)
    got = qpsk.minsync_scan(cands, n, lambda lo, hi: bits[lo:hi])
    assert [(k + 1, t) for k, t in got] == want
    assert len(want) >= 4 and {t for _, t in want} == {0, 1}


@pytest.mark.parametrize("name", NAMES)
def test_maxsync_buffer_model_reproduces_reference(name):
    g = _load(name)
    a = _a_idx(g)
    events = [(int(m) - 1, int(t)) for m, t in zip(g["minsync"], np.r_[g["template"], np.zeros(len(g["minsync"]), np.int64)])]
    bufs = qpsk.maxsync_buffers(events, int(g["n"]), lambda k: a[k], len(a))
    assert len(bufs) == len(g["argmax"])
    iv = g["buf_intervals"]
    for i, (ivs, start, tm) in enumerate(bufs):
        assert ivs == [(int(lo), int(c)) for j, lo, c in iv if j == i]
        assert start == int(g["buf_start"][i]) and tm == int(g["template"][i])
        assert start + g["argmax"][i] / 2.0 == g["maxsync"][i]
    assert list(g["maxsync"][1:]) == list(g["syncs"])


def test_timing_jump_equals_single_steps():
    """the walk's jump over plain samples gives the timing the reference's one-by-one additions give, and skips no event"""
    P = 2048000 / 72000
    hP, hP1 = P / 2, P / 2 + 1
    rng = np.random.default_rng(3)
    n = 0
    for _ in range(40000):
        t = float(rng.uniform(1, 2) * 2.0 ** int(rng.integers(0, 5)) - rng.uniform(0, 1e-12) * int(rng.integers(0, 2)))
        if not (1 <= t < P) or hP <= t < hP1:
            continue
        T = hP if t < hP else P
        m = _skip(t, T, int(rng.integers(1, 40)))
        v = t
        for _ in range(m):
            assert v < T and not (hP <= v < hP1)
            v = v + 1.0
        assert v == t + m
        n += m > 1
    assert n > 10000
