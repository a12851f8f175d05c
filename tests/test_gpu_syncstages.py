"""
The accurate-sync batch's envelope pre-filter and its correlation/peak tail, each alone (csrc/dd_audio_sync.h:
sync_prefilter_stage through dd_debug_sync_prefilter, sync_tail_stage through dd_debug_sync_tail -- the functions
dd_noaa_sync_windows_multi runs per batch), element by element against the restatements of tests/_syncstages.py.

Pre-filter: k_filtfilt_cos<Q, MODE> (csrc/dd_filtfilt_kernels.h), the prefix-sum form of a zero-phase FIR whose taps are a cosine
series, for Q = 1, 2, 3 at the tap counts and lengths where its staging, its lane segments (S = ceil(W / 512) changes at K = 514),
its table phase and its last partial tile change; against filtfilt_ld (long double) in units of s = max|x| (sum|b|)^2, beside
the tiled direct form (route 1) on the same taps.

Tail: k_scan_part / k_scan_final -> k_xcorr_runs_pk -> k_sync_peak.  Integer-valued hay and needles make every prefix sum and
product exact, so picks are equal and heights agree to the last bits of one division and one square root; the maximum is planted
on lane, wave and tile borders, tied, put at both ends, and moved across the i + 2 m < n rule.
"""
import ctypes as C
import os

import numpy as np
import pytest

import _syncstages as S

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
HAMMING = (0.54, -0.46)
BLACKMAN = (0.42, -0.5, 0.08)
BLACKMANHARRIS = (0.35875, -0.48829, 0.14128, -0.01168)

# Route 0 (prefix-sum form) against filtfilt_ld over every case below, measured on the MI355X, in units of s: 1.524e-14 for Q = 1
# (K = 64, 1e6 + noise), 6.118e-15 for Q = 2, 6.372e-15 for Q = 3; route 1 (tiled direct form): 4.3e-15, 4.2e-15, 3.3e-15 (DESIGN.md,
# beside the kernel's description).  The bound is 8 x the measurement -- the margin covers inputs not drawn here -- and never more
# than 1e-11 s, what test_filtfilt_tiled_tap_counts holds the tiled form to.
MEASURED_COS = {1: 1.524e-14, 2: 6.118e-15, 3: 6.372e-15}
TILED_BOUND = 1e-11
# heights of the real-valued tail cases against the restatement, measured: 3.0e-13 (two-sample needle in 4097 samples: the window's
# energy is a difference of prefix sums 2000 times its size), 1.2e-14 otherwise; bound 4 x, never more than the 1e-9 between routes
MEASURED_HEIGHT = 3.0e-13


def _cos_bound(Q):
    return min(8.0 * MEASURED_COS[Q], TILED_BOUND)


@pytest.fixture(scope="module")
def dd():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from directdemod_amd import _hip, filters
    _hip.require_gpu()

    class NS:
        pass
    ns = NS()
    ns.hip, ns.filters, ns.lib = _hip, filters, _hip.lib()
    return ns


# ---------------------------------------------------------------- pre-filter
def _fit(dd, b):
    b = np.ascontiguousarray(b, np.float64)
    a = (C.c_double * 4)()
    q = C.c_int(0)
    ok = dd.lib.dd_debug_cos_fit(b.ctypes.data_as(DP), len(b), a, C.byref(q))
    return (q.value, list(a)) if ok == 1 else None


def _taps(K, a):
    return S.cosine_taps_ld(K, a)


def _largest_accepted(dd, a):
    lo, hi = 64, 8192
    assert _fit(dd, _taps(lo, a).astype(np.float64)) and not _fit(dd, _taps(hi, a).astype(np.float64))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _fit(dd, _taps(mid, a).astype(np.float64)):
            lo = mid
        else:
            hi = mid
    return lo


POISON = -7.25e77


def _prefilter(dd, x, b64, route):
    """x [nwin][n] -> (rc, out [nwin][n]); the 16 doubles behind the output must come back untouched"""
    x = np.ascontiguousarray(x, np.float64)
    nwin, n = x.shape
    d_x = dd.hip.DevArray.from_host(x.reshape(-1))
    d_o = dd.hip.DevArray.from_host(np.full(nwin * n + 16, POISON))
    rc = dd.lib.dd_debug_sync_prefilter(d_x.ptr, n, nwin, b64.ctypes.data_as(DP), len(b64), route, d_o.ptr, None)
    out = d_o.to_host()
    assert np.all(out[nwin * n:] == POISON), "route %d wrote behind its output" % route
    return rc, out[:nwin * n].reshape(nwin, n)


def _lengths(K, T):
    m = (9 * K + 2) // T + 1                                             # smallest m with m T - 1 - 6 K > 3 K
    ns = [3 * K + 1] + [m * T + d - 6 * K for d in (-1, 0, 1)] + [v for v in (T - 1, T, T + 1, 2 * T + 1) if v > 3 * K]
    return sorted(set(ns))


def _signals(n, K, T, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    sig = [rng.standard_normal(n) + 0.5,
           np.abs(0.3 + 0.2 * np.sin(2 * np.pi * t / 493.0) + 0.05 * rng.standard_normal(n)),   # an envelope: positive, slow, noisy
           1e6 + rng.standard_normal(n)]
    for at in (0, n - 1, 3 * K, T - K if 0 <= T - K < n else n // 2):
        e = np.zeros(n)
        e[at] = 1.0
        sig.append(e)
    sig.append(np.full(n, 2.5))
    sig.append(rng.standard_normal(n) + 0.5)
    return np.array(sig)                                                 # [9][n]: three calls of three windows


LARGEST = {1: 1025, 2: 1560, 3: 921}              # the largest K dd_debug_cos_fit accepts per Q (test_prefilter_largest_tap_count finds them)
_COS_TAPS = [("hamming", HAMMING, 1, K) for K in (492, 64, 65, 513, 514, LARGEST[1])] + \
            [("blackman", BLACKMAN, 2, K) for K in (64, 301, 513, 514, LARGEST[2])] + [("a0+a2", (0.5, 0.0, 0.5), 2, 129)] + \
            [("blackmanHarris", BLACKMANHARRIS, 3, K) for K in ("getB151", 64, LARGEST[3])]
_COS_CASES = [c + (n,) for c in _COS_TAPS for n in _lengths(151 if c[3] == "getB151" else c[3], 2048 if c[2] == 1 else 1024)]
_worst = {}


def test_prefilter_largest_tap_count(dd):
    """the largest K the prefix-sum form takes, by bisecting dd_debug_cos_fit: K is accepted (and tested below), K + 1 is refused by route 0"""
    for Q, a in ((1, HAMMING), (2, BLACKMAN), (3, BLACKMANHARRIS)):
        K = _largest_accepted(dd, a)
        assert K == LARGEST[Q]
        rc, _ = _prefilter(dd, np.ones((1, 3 * (K + 1) + 1)), _taps(K + 1, a).astype(np.float64), 0)
        assert rc == dd.hip.DD_ERR_UNSUPPORTED


@pytest.mark.parametrize("name,a,Q,K,n", _COS_CASES, ids=["%s-%s-n%d" % (c[0], c[3], c[4]) for c in _COS_CASES])
def test_prefilter_cosine_form_vs_long_double(dd, name, a, Q, K, n):
    """Every output of both routes against filtfilt_ld, three windows per call (and the first alone: same bits), at n = 3 K + 1,
    n + 6 K around a multiple of the tile, n around one and two tiles.  Inputs: noise + 0.5, an envelope, 1e6 + noise, a single 1.0 at
    sample 0, n - 1, 3 K and TILE - K, a constant (output c (sum b)^2).  The shortest length again after LDS was filled with NaN
    patterns: same bits."""
    T = 2048 if Q == 1 else 1024
    if K == "getB151":
        K = 151
        b64 = np.ascontiguousarray(dd.filters.blackmanHarris(151).getB, np.float64)
    else:
        b64 = _taps(K, a).astype(np.float64)
    b = b64.astype(S.LD)                                                 # the reference filters with the taps the device is given
    fit = _fit(dd, b64)
    assert fit and fit[0] == Q, "these taps do not take the Q = %d form: %r" % (Q, fit)
    x = _signals(n, K, T, 1000 * Q + K + n)
    ref = np.array([S.filtfilt_ld(b, xi) for xi in x])
    s = np.array([S.filtfilt_scale(b, xi) for xi in x])[:, None]
    got = {}
    for route in (0, 1):
        outs = []
        for g in range(3):
            rc, o = _prefilter(dd, x[3 * g:3 * g + 3], b64, route)
            dd.hip.check(rc, "dd_debug_sync_prefilter")
            outs.append(o)
        got[route] = np.concatenate(outs)
        rc, one = _prefilter(dd, x[:1], b64, route)
        dd.hip.check(rc, "dd_debug_sync_prefilter")
        assert np.array_equal(one[0], got[route][0]), "a window alone differs from the same window in a batch of three"
    e0 = np.max(np.abs(got[0] - ref) / s, axis=1).astype(np.float64)
    e1 = np.max(np.abs(got[1] - ref) / s, axis=1).astype(np.float64)
    w = _worst.setdefault(Q, [0.0, 0.0])
    w[0], w[1] = max(w[0], float(e0.max())), max(w[1], float(e1.max()))
    print("Q %d K %4d n %5d: cosine form %.2e s (signal %d), tiled form %.2e s; Q %d so far %.3e / %.3e" %
          (Q, K, n, e0.max(), int(np.argmax(e0)), e1.max(), Q, w[0], w[1]))
    assert e1.max() <= TILED_BOUND
    k = int(np.argmax(e0))
    assert e0.max() <= _cos_bound(Q), "signal %d at sample %d" % (k, int(np.argmax(np.abs(got[0][k] - ref[k]))))
    c2 = 2.5 * np.sum(b) ** 2
    assert np.max(np.abs(got[0][7] - c2)) <= _cos_bound(Q) * float(s[7, 0])
    if n == 3 * K + 1:
        dd.hip.check(dd.lib.dd_debug_fill_lds(0xFFFFFFFF, None), "dd_debug_fill_lds")
        rc, again = _prefilter(dd, x[:3], b64, 0)
        dd.hip.check(rc, "dd_debug_sync_prefilter")
        assert np.array_equal(again, got[0][:3]), "stale LDS reaches the output"


def test_prefilter_refusals(dd):
    """route 0 on taps that are no cosine series: DD_ERR_UNSUPPORTED; n <= 3 K: the batch's own error (SciPy's padlen message)"""
    rng = np.random.default_rng(1)
    b = np.ascontiguousarray(rng.standard_normal(100) / 100)
    rc, _ = _prefilter(dd, np.ones((1, 400)), b, 0)
    assert rc == dd.hip.DD_ERR_UNSUPPORTED
    rc, out = _prefilter(dd, rng.standard_normal((2, 400)), b, 1)
    dd.hip.check(rc, "dd_debug_sync_prefilter")
    h = _taps(64, HAMMING).astype(np.float64)
    for route in (0, 1):
        rc, _ = _prefilter(dd, np.ones((1, 192)), h, route)
        assert rc == dd.hip.DD_ERR_INVALID and "padlen, which is 192" in dd.hip.last_error()
        rc, _ = _prefilter(dd, np.ones((1, 193)), h, route)
        assert rc == dd.hip.DD_OK


# ---------------------------------------------------------------- tail
def _tail(dd, hay, env, needles, group=None):
    hay = np.ascontiguousarray(hay, np.float64)
    env = np.ascontiguousarray(env, np.float64)
    needles = np.ascontiguousarray(np.atleast_2d(needles), np.float64)
    nwin, n = hay.shape
    d_h, d_e = dd.hip.DevArray.from_host(hay.reshape(-1)), dd.hip.DevArray.from_host(env.reshape(-1))
    peak = np.full(nwin, 12345, np.int64)
    height, tsync = np.full(nwin, POISON), np.full(nwin, POISON)
    g = None if group is None else np.ascontiguousarray(group, np.int32)
    dd.hip.check(dd.lib.dd_debug_sync_tail(d_h.ptr, d_e.ptr, n, nwin, needles.ctypes.data_as(DP), needles.shape[1], needles.shape[0],
                                           None if g is None else g.ctypes.data_as(C.POINTER(C.c_int)),
                                           peak.ctypes.data_as(C.POINTER(C.c_int64)), height.ctypes.data_as(DP), tsync.ctypes.data_as(DP), None),
                 "dd_debug_sync_tail")
    return peak, height, tsync


def _needles(m):
    """two piecewise-constant needles of m small integers: the Barker codes of 11 and 13 chips, +-2 and +-3, stretched to m samples
    (7 and 8 runs) -- a copy of such a needle in the hay correlates badly with every shift of it, whole or clipped.  The needles of
    two samples are (1, 4) and (2, 5): positive, since the +-1 background would be a copy of a signed one."""
    out = []
    for k, code in enumerate(("+++---+--+-", "+++++--++-+-+")):
        if m == 2:
            out.append(np.array([1.0 + k, 4.0 + k]))
            continue
        vals = np.array([(2 + k) * (1 if c == "+" else -1) for c in code])
        edges = np.linspace(0, m, len(vals) + 1).astype(int)
        out.append(np.repeat(vals, np.diff(edges)).astype(np.float64))
    return np.array(out)


def _planted(n, needle, outputs, sign=None):
    """+-1 alternating (energy everywhere, next to no correlation with a needle of long runs) with 50 x needle laid so that its
    correlation window is the one of output A, for every A of `outputs` (clipped at the ends of the window); a full plant has
    correlation exactly 1.0 = 50 vv / sqrt(2500 vv vv)"""
    m = len(needle)
    hay = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    for k, A in enumerate(outputs):
        idx = A - m // 2 + np.arange(m)
        ok = (idx >= 0) & (idx < n)
        hay[idx[ok]] = (50.0 if sign is None else 50.0 * sign[k]) * needle[ok]
    return hay


def _check_exact(dd, hay, env, needles, group, label, expect_peak=None):
    """integer-valued windows: equal picks, heights within 2 ulp, the post-sync mean equal to the one float64 division"""
    peak, height, tsync = _tail(dd, hay, env, needles, group)
    m = needles.shape[1]
    for w in range(len(hay)):
        i, h, ts, gap = S.tail_np(hay[w], env[w], needles[0 if group is None else group[w]])
        what = "%s, window %d: device (%d, %r, %r), restatement (%d, %r, %r)" % (label, w, peak[w], height[w], tsync[w], i, h, float(ts))
        if expect_peak is not None:
            assert i == expect_peak[w], "the case does not plant what it means to: " + what
        assert peak[w] == i, what
        if i == S.INT64_MIN:
            assert np.isnan(height[w]) and np.isnan(tsync[w]), what
            continue
        assert abs(height[w] - h) <= 2 * np.spacing(h), what
        if np.isnan(ts):
            assert np.isnan(tsync[w]) and i + 2 * m >= hay.shape[1], what
        else:
            assert tsync[w] == float(np.sum(env[w][i + m:i + 2 * m])) / float(m), what
    return peak, height, tsync


_NS = (None, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 4097)
_MS = (2, 255, 256, 257, 984, 1023, 1025, 1793)
_TAIL_SHAPES = sorted(set((m if n is None else n, m) for n in _NS for m in _MS if n is None or m <= n))


@pytest.mark.parametrize("n,m", _TAIL_SHAPES)
def test_tail_planted_maximum(dd, n, m):
    """The maximum planted at output 0 and n - 1, on both sides of a wave border (63 / 64), of the lane stride (255 / 256) and of a
    tile border (1023 / 1024, 2047 / 2048), where the pick is negative, and where i + 2 m is n - 1, n and n + 1; one window per plant
    in one call, two needles alternating, then the first 1, 7, 8, 9 and 17 windows (cycled) again: same answers."""
    needles = _needles(m)
    outs = [0, n - 1, 63, 64, 255, 256, 1023, 1024, 2047, 2048, m // 2 - 1, m // 2, n - 1 - 2 * m + m // 2, n - 2 * m + m // 2, n + 1 - 2 * m + m // 2]
    outs = [A for A in outs if 0 <= A < n]
    group = np.arange(len(outs)) % 2
    rng = np.random.default_rng(n + m)
    hay = np.array([_planted(n, needles[group[w]], [A]) for w, A in enumerate(outs)])
    env = rng.integers(0, 256, hay.shape).astype(np.float64)
    # a plant whose window is whole is the maximum (1.0) by construction; a clipped one is whatever the restatement says
    whole = [A - m // 2 if (A - m // 2 >= 0 and A - m // 2 + m <= n) else None for A in outs]
    peak, height, tsync = _check_exact(dd, hay, env, needles, group, "n %d m %d" % (n, m))
    for w, p in enumerate(whole):
        if p is not None:
            assert peak[w] == p and height[w] == 1.0
    for nwin in (1, 7, 8, 9, 17):
        sel = np.arange(nwin) % len(outs)
        p2, h2, t2 = _tail(dd, hay[sel], env[sel], needles, group[sel])
        assert np.array_equal(p2, peak[sel]) and np.array_equal(h2, height[sel], equal_nan=True) and np.array_equal(t2, tsync[sel], equal_nan=True), nwin


def test_tail_ends_of_the_window_hold_the_maximum(dd):
    """Output 0 and output n - 1 as the window's maximum (a clipped correlation window: the needle's matching part laid at the
    end, the rest of the window quiet).  n - 1 in a tile of its own (n = 1024 k + 1) is a per-tile record with one value: its
    second-largest is -inf, and the merge has to take the other tiles' maximum instead."""
    for n, m in ((1025, 256), (2049, 255), (3073, 984), (4097, 257), (2048, 2), (1024, 1023)):
        needles = _needles(m)
        hay, want = [], []
        for A in (0, n - 1):
            hay.append(_planted(n, needles[0], [A]))
            want.append(A - m // 2)
        hay = np.array(hay)
        env = np.random.default_rng(n).integers(0, 256, hay.shape).astype(np.float64)
        _check_exact(dd, hay, env, needles, None, "end plants n %d m %d" % (n, m), expect_peak=want)


@pytest.mark.parametrize("n,m", [(4097, 256), (3073, 255), (4097, 257), (4097, 2)])
def test_tail_equal_maxima_first_wins(dd, n, m):
    """Two and three maxima of exactly 1.0 in different lanes, waves and tiles, the earlier one in the lower lane and in the higher
    lane (output i sits in lane i mod 256 of tile i / 1024, so 522 is in a lower lane than 200): the first index wins, and the
    threshold sees m2 == m1."""
    needles = _needles(m)
    h = m // 2
    sets = [(h + 10, h + 10 + m + 3), (200 + h, 522 + m), (138 + h, 700 + m), (h + 60, 1024 + h + 2), (1023, 1024 + m), (700, 2048 + 5),
            (200 + h, 522 + m, 1500 + m), (h + 1, 1024 + h, 2048 + h), (1100, 1100 + m, 1100 + 2 * m + 1), (h, h + m, n - 1 - (m - 1 - h))]
    sets = [s for s in sets if all(b - a >= m for a, b in zip(s, s[1:])) and s[0] >= h and s[-1] - h + m <= n]
    assert len(sets) >= 8
    assert any((a % 256) > (b % 256) for a, b in (s[:2] for s in sets)) and any((a % 256) < (b % 256) for a, b in (s[:2] for s in sets))
    assert any(a // 1024 != b // 1024 for a, b in (s[:2] for s in sets)) and any(a // 1024 == b // 1024 and a % 256 // 64 != b % 256 // 64 for a, b in (s[:2] for s in sets))
    hay = np.array([_planted(n, needles[0], s) for s in sets])
    env = np.random.default_rng(n + m).integers(0, 256, hay.shape).astype(np.float64)
    for w, s in enumerate(sets):
        cor = S.xcorr_np(hay[w], needles[0])
        assert np.count_nonzero(cor == 1.0) == len(s) and np.max(cor) == 1.0, "the plants are not the only, equal maxima"
    peak, height, _ = _check_exact(dd, hay, env, needles[:1], None, "ties n %d m %d" % (n, m), expect_peak=[s[0] - h for s in sets])
    assert np.all(height == 1.0)


def test_tail_two_smallest_in_different_tiles(dd):
    """two correlations of exactly -1.0 (a negated plant) in different tiles beside one maximum"""
    n, m = 4097, 256
    needles = _needles(m)
    hay = np.array([_planted(n, needles[0], (300, 1500, 3000), sign=(-1, 1, -1)), _planted(n, needles[0], (3000, 300, 1500), sign=(1, -1, -1))])
    for w in range(2):
        assert np.count_nonzero(S.xcorr_np(hay[w], needles[0]) == -1.0) == 2
    env = np.random.default_rng(4).integers(0, 256, hay.shape).astype(np.float64)
    _check_exact(dd, hay, env, needles[:1], None, "two smallest", expect_peak=[1500 - 128, 3000 - 128])


def test_tail_not_found_and_nan(dd):
    """A window where every correlation is the same value has no candidate above the threshold: (INT64_MIN, NaN, NaN).  With
    zero-padded 'same' windows that takes n = m = 2, needle (1, 1) and hay (c, 0): both outputs are c / sqrt(2 c^2).  A constant
    hay is NOT such a window (the clipped windows at the ends correlate differently: the reference finds a peak there, and so does
    the device); an all-zero one is 0 / 0 everywhere.  A silent stretch as long as the needle, or one NaN sample, likewise give the
    documented triple, in every window count's last and first window."""
    peak, height, tsync = _tail(dd, np.array([[3.0, 0.0], [0.0, 3.0]]), np.ones((2, 2)), np.array([[1.0, 1.0]]))
    cor = S.xcorr_np([3.0, 0.0], [1.0, 1.0])
    assert cor[0] == cor[1] and not np.isnan(cor[0])
    assert peak[0] == S.INT64_MIN and np.isnan(height[0]) and np.isnan(tsync[0])
    _check_exact(dd, np.array([[3.0, 0.0], [0.0, 3.0]]), np.ones((2, 2)), np.array([[1.0, 1.0]]), None, "n = m = 2")
    for n, m in ((1025, 256), (2049, 984), (3073, 2), (257, 257)):
        needles = _needles(m)
        rng = np.random.default_rng(n)
        base = _planted(n, needles[0], [n // 2])
        const, zero, silent, nan0, nan1 = np.full(n, 7.0), np.zeros(n), base.copy(), base.copy(), base.copy()
        silent[n // 3:n // 3 + m] = 0.0
        nan0[0] = np.nan
        nan1[n - 1] = np.nan
        hay = np.array([base, const, zero, silent, nan0, nan1, base, const, base])
        env = rng.integers(0, 256, hay.shape).astype(np.float64)
        peak, _, _ = _check_exact(dd, hay, env, needles[:1], None, "n %d m %d" % (n, m))
        assert list(peak[2:6]) == [S.INT64_MIN] * 4 and peak[0] != S.INT64_MIN and peak[0] == peak[6] == peak[8]
        if n > m:
            assert peak[1] != S.INT64_MIN


_REAL_SHAPES = [(1023, 255), (1024, 256), (1025, 257), (2047, 984), (2048, 1023), (2049, 1025), (3073, 1793), (4097, 984), (4097, 2), (1793, 1793)]


@pytest.mark.parametrize("n,m", _REAL_SHAPES)
def test_tail_real_valued(dd, n, m):
    """Real-valued windows (noise with a scaled needle in it, 17 windows, two needles): the pick equals the restatement's wherever its
    best and second-best differ by more than 1e-9 (at least 90 % of the windows), heights within the bound, the post-sync mean within
    m 2^-53 max|env|, the summation's own bound."""
    needles = _needles(m) * 233.0 / 255.0 + 11.0 / 255.0
    rng = np.random.default_rng(7 * n + m)
    nwin = 17
    group = np.arange(nwin) % 2
    hay = 0.3 + 0.1 * rng.standard_normal((nwin, n))
    for w in range(nwin):
        p = int(rng.integers(0, n - m + 1))
        hay[w, p:p + m] += 0.4 * needles[group[w]]
    env = np.abs(0.3 + 0.1 * rng.standard_normal((nwin, n)))
    peak, height, tsync = _tail(dd, hay, env, needles, group)
    clear, worst = 0, 0.0
    for w in range(nwin):
        i, h, ts, gap = S.tail_np(hay[w], env[w], needles[group[w]])
        assert i != S.INT64_MIN
        if gap > 1e-9:
            clear += 1
            assert peak[w] == i, (w, peak[w], i)
            worst = max(worst, abs(height[w] - h))
            if np.isnan(ts):
                assert np.isnan(tsync[w])
            else:
                assert abs(S.LD(tsync[w]) - ts) <= m * 2.0 ** -53 * np.max(np.abs(env[w])), (w, tsync[w], float(ts))
    print("n %d m %d: %d of %d windows clear, heights within %.2e" % (n, m, clear, nwin, worst))
    assert clear >= 0.9 * nwin
    assert worst <= min(4.0 * MEASURED_HEIGHT, 1e-9)
