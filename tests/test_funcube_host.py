"""Funcube sync detection, host side: the synthesised recordings' hashes, lim / limBin at their edges, the sync pattern, the block-sum
correlation against np.correlate, the run-skipping rule at Funcube's symbol period, and the MAXSYNC buffer model against the buffers
the reference built (tests/golden/funcube_*.npz, tools/gen_golden.py --funcube)."""
import collections
import math
import os

import numpy as np
import pytest

import _funcube
from _symbolwalk import skip as _skip
from directdemod_amd import bpsk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(_funcube.CASES)


def _load(name):
    return np.load(os.path.join(GOLDEN, "funcube_%s.npz" % name))


def _a_idx(g):
    if int(g["nsym"]) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate(([int(g["a_first"])], int(g["a_first"]) + np.cumsum(g["a_diff"].astype(np.int64))))


@pytest.mark.parametrize("name", NAMES)
def test_synthesis_hash(name):
    raw, off, corr = _funcube.case(name)
    g = _load(name)
    assert _funcube.sha256(raw) == str(g["sha256"]), "synthesis drift (NumPy build), not a decoder bug"
    assert raw.shape[0] == int(g["n"]) and off == int(g["offset"]) and int(corr) == int(g["corrfreq"])


def test_fixtures_hold_what_the_cases_are_for():
    """the reference fired MINSYNC at every planted sync word and ran the MAXSYNCs each case is meant to exercise"""
    for name, nmax, useful in (("a", 2, 0), ("b", 2, 0), ("c", 2, 0), ("d", 0, 0), ("e", 1, 0), ("f", 3, 1), ("g", 3, 1)):
        g = _load(name)
        assert len(g["maxsync"]) == nmax and int(g["useful"]) == useful and int(g["one_maxsync"]) == (nmax == 1)
        planted = [int(round(t * _funcube.BIT_RATE)) + bpsk.NSYNC for t in _funcube.CASES[name]["syncs"]]      # the word's last bit ends here
        for p in planted:
            assert np.any(np.abs(g["minsync"] - p * bpsk.SYMS) < 2 * bpsk.SYMS), (name, p)
        assert len(g["minsync"]) >= len(planted)
    g = _load("g")
    assert len(g["chunk_offset"]) == 2 and g["dopp_current"][1] != g["dopp_target"][1]       # the second chunk ends on the ramp


def test_lim_limbin():
    from directdemod_amd import decode_funcube
    cases = [(-1e9, -128), (-128.5, -128), (-128.0, -128), (-127.9, -127), (-127.0, -127), (-1.0, -1), (-0.5, -1), (-1e-300, -1),
             (0.0, 0), (-0.0, 0), (1e-300, 1), (0.999, 1), (1.0, 1), (1.5, 1), (126.99, 126), (127.0, 127), (127.5, 127), (128.0, 127),
             (1e9, 127)]
    for x, want in cases:
        assert decode_funcube.lim(x) == want, x
        assert type(decode_funcube.lim(np.float64(x))) is int
    for x, want in [(-1.0, 0), (0.0, 0), (-0.0, 0), (1e-300, 1), (5.0, 1)]:
        assert decode_funcube.limBin(x) == want


def test_sync_pattern_and_constants():
    s = bpsk.sync_bits()
    assert s.tolist() == _funcube.sync_bits().tolist() and len(s) == 33
    assert len(bpsk.sync12khz()) == 330 and np.array_equal(bpsk.sync12khz()[::10], s)
    assert bpsk.REP == 1706 and bpsk.TLEN == 56298 and bpsk.RETAIN == 112596
    assert set(bpsk.template_bits().tolist()) == {127, -128}
    a0, b0, a1, b1 = bpsk.costas_coefficients()
    bw = 0.05235833333 * 6
    d = 1.0 + 2.0 * 0.70710678118 * bw + bw * bw
    assert a0 == (4 * 0.70710678118 * bw) / d and b0 == (4 * bw * bw) / d and a1 < a0 and b1 < b0
    h = bpsk.hyp_table()
    assert len(h) == 256 and h[128] == 0.0 and h[0] == -1.0 and h[255] == 1.0 and h[129] == np.tanh(1)


@pytest.mark.parametrize("rep,L", [(3, 99), (3, 100), (3, 257), (4, 132), (4, 133), (7, 400)])
def test_block_correlation_matches_numpy(rep, L):
    """a short piecewise-constant template (the 33 sync bits, `rep` samples each); L = 33 rep is the shortest buffer 'same' keeps
    the buffer's length for; the zero buffer and the +-1 buffers give ties, where the first maximum counts"""
    rng = np.random.default_rng(1000 * rep + L)
    t = bpsk.template_bits()
    for buf in (rng.integers(-128, 128, L), rng.integers(-1, 2, L), np.zeros(L, dtype=np.int64), np.full(L, 127), np.full(L, -128)):
        ref = np.correlate(list(buf), np.repeat(t, rep), mode="same")
        got = bpsk.correlate_same_blocks(buf, t, rep)
        assert len(ref) == L and np.array_equal(got, ref)
        assert int(np.argmax(np.abs(got))) == int(np.argmax(np.abs(ref)))


def test_timing_jump_equals_single_steps_at_funcube_period():
    """at P = 170.67 a run between events is up to 85 samples and passes through up to seven binades: each jump stays below twice the
    power of two above its start, gives the timing the reference's one-by-one additions give, and skips no event; chained jumps
    reach the next event at the sample the single steps reach it"""
    P = 2048000 / 12000
    hP, hP1 = P / 2, P / 2 + 1
    rng = np.random.default_rng(4)
    n = long = 0
    for _ in range(40000):
        t = float(rng.uniform(1, 2) * 2.0 ** int(rng.integers(0, 8)) - rng.uniform(0, 1e-12) * int(rng.integers(0, 2)))
        if not (1 <= t < P) or hP <= t < hP1:
            continue
        T = hP if t < hP else P
        m = _skip(t, T, int(rng.integers(1, 1025)))
        _, e = math.frexp(t)
        assert t + m < math.ldexp(1.0, e + 1) or m == 0
        v = t
        for _ in range(m):
            assert v < T and not (hP <= v < hP1)
            v = v + 1.0
        assert v == t + m
        n += m > 1
        long += m > 28
    assert n > 10000 and long > 2000
    for _ in range(300):                                  # whole runs: from after an event to the next one
        t = float(rng.uniform(1.0, 3.0))
        v, steps = t, 0
        while not (hP <= v < hP1) and v < P:
            v, steps = v + 1.0, steps + 1
        u, jumped = t, 0
        while not (hP <= u < hP1) and u < P:
            m = _skip(u, hP if u < hP else P, 1024) if u >= 1.0 else 0
            u, jumped = (u + m, jumped + m) if m > 0 else (u + 1.0, jumped + 1)
        assert (u, jumped) == (v, steps)


def _reference_buffers(a, mins, total):
    """decode_funcube.py:240-296's statement order sample by sample over the A indices and the MINSYNC ctr values: (maxBuffStart,
    the samples in the buffer) of every correlation that runs"""
    fire = {int(a[m - 1]) for m in mins}
    is_a = bytearray(total)
    for s in a:
        is_a[s] = 1
    buf, start, retain, last, ctr, out = collections.deque(), 0, -1, None, 0, []
    for s in range(total):
        if last is not None and (ctr > last + (4.9 * 12000) - (2 * 330) or not retain == -1) and not ctr > last + (5.2 * 12000):
            if len(buf) == 0:
                start = s
            buf.append(s)
        if retain == -1:
            if len(buf) > 2 * 56298:
                start += 1
                buf.popleft()
        elif retain == 0:
            retain -= 1
            out.append((start, list(buf)))
            buf.clear()
        else:
            retain -= 1
        if is_a[s]:
            ctr += 1
            if s in fire:
                last = ctr
                retain = 2 * 56298
    return out


@pytest.mark.parametrize("mins,total", [([100, 101, 105], 130000), ([100, 60100, 60103], 1930000), ([100, 63100], 2010000),
                                        ([100, 60100], 1850000)])
def test_maxsync_buffer_model_matches_sample_loop(mins, total):
    """synthetic A indices (a symbol every 30 samples, so the 4.9 s .. 5.2 s collect span is longer than the sliding buffer) and
    MINSYNC lists that take every path: re-armed countdowns, a sync inside the collect span with the sliding pre-buffer, a sync after
    the span has passed (the stale window and its start), a countdown cut by the end of the recording"""
    a = [int(v) for v in range(7, total, 30)]
    want = _reference_buffers(a, mins, total)
    got = bpsk.maxsync_buffers([m - 1 for m in mins], total, lambda k: a[k], len(a))
    assert len(got) == len(want) and len(want) >= 1
    for (ivs, start), (wstart, wbuf) in zip(got, want):
        smp = np.concatenate([np.arange(lo, lo + n) for lo, n in ivs])
        assert start == wstart and np.array_equal(smp, wbuf)
        assert all(ivs[i][0] + ivs[i][1] < ivs[i + 1][0] for i in range(len(ivs) - 1))
    if mins == [100, 63100]:
        assert len(got[1][0]) == 2                       # the stale window, then the new sync's samples


@pytest.mark.parametrize("name", NAMES)
def test_maxsync_buffer_model_reproduces_reference(name):
    g = _load(name)
    a = _a_idx(g)
    bufs = bpsk.maxsync_buffers([int(m) - 1 for m in g["minsync"]], int(g["n"]), lambda k: a[k], len(a))
    assert len(bufs) == len(g["argmax"])
    iv = g["buf_intervals"]
    for i, (ivs, start) in enumerate(bufs):
        assert ivs == [(int(lo), int(c)) for j, lo, c in iv if j == i]
        assert start == int(g["buf_start"][i])
        assert start + g["argmax"][i] == g["maxsync"][i]
    assert list(g["maxsync"][1:]) == list(g["syncs"]) or int(g["one_maxsync"])


def test_import_and_construct_without_gpu():
    from directdemod_amd import decode_funcube

    class Src:
        sampFreq = 2048000
        length = 0
    o = decode_funcube.decode_funcube(Src(), 0, None, 145000000, 145025000, corrfreq=True)
    assert o.useful == 0 and o.minsyncs == [] and o.buffers == [] and o.argmax == [] and o.ramps == [] and o.timings == {}
