"""
CPU pins of tests/_syncstages.py, the restatements tests/test_gpu_syncstages.py holds the accurate-sync batch's pre-filter and
correlation/peak tail to: the long double zero-phase FIR against the oracle and SciPy, the correlation and two-peak pick against
the oracle's whole __correlateAndFindPeaks on a synthetic APT window.
"""
import numpy as np
import pytest

import _syncstages as S
from oracle import dd_oracle as O


def test_long_double_is_wider_than_double():
    """filtfilt_ld is a reference for float64 kernels only where long double carries more than 53 bits (x87: 64)"""
    assert np.finfo(np.longdouble).eps < 2e-19


def test_cosine_taps_ld_are_the_windows():
    # (the float64 closed forms round their phases k * ang: up to 3 * 2 pi * 2^-53 = 2e-15 of a coefficient <= 0.5)
    for K in (64, 151, 492):
        assert np.max(np.abs(S.cosine_taps_ld(K, (0.54, -0.46)).astype(np.float64) - O.win_hamming(K))) < 2e-15
        assert np.max(np.abs(S.cosine_taps_ld(K, (0.35875, -0.48829, 0.14128, -0.01168)).astype(np.float64) - O.win_blackmanharris(K))) < 2e-15


_TAPS = {"hamming64": lambda: O.win_hamming(64), "hamming492": lambda: O.win_hamming(492), "hamming1025": lambda: O.win_hamming(1025),
         "blackman301": lambda: S.cosine_taps_ld(301, (0.42, -0.5, 0.08)).astype(np.float64),
         "blackmanHarris151": lambda: O.win_blackmanharris(151)}


@pytest.mark.parametrize("name", sorted(_TAPS))
def test_filtfilt_ld_is_the_oracles_and_scipys(name):
    """Measured over these five tap sets and both inputs: at most 9.1e-16 s, s = max|x| (sum|b|)^2 -- float64 rounding of the two
    float64 references, not of the restatement.  Bound 4e-15 s."""
    import scipy.signal
    b = _TAPS[name]()
    K = len(b)
    rng = np.random.default_rng(K)
    n = 3 * K + 1 + 700
    for x in (rng.standard_normal(n) + 0.5, 1e6 + rng.standard_normal(n)):
        ref = S.filtfilt_ld(b, x)
        s = S.filtfilt_scale(b, x)
        e_o = float(np.max(np.abs(O.filtfilt(b, [1.0], x) - ref))) / s
        e_s = float(np.max(np.abs(scipy.signal.filtfilt(b, [1.0], x) - ref))) / s
        print("%s: oracle %.2e s, scipy %.2e s" % (name, e_o, e_s))
        assert e_o <= 4e-15 and e_s <= 4e-15


def test_filtfilt_ld_refuses_short_inputs_like_scipy():
    with pytest.raises(ValueError, match="padlen, which is 192"):
        S.filtfilt_ld(O.win_hamming(64), np.ones(192))


def test_filtfilt_ld_of_a_constant():
    b = O.win_hamming(65)
    y = S.filtfilt_ld(b, np.full(300, 3.0))
    assert np.max(np.abs(y - 3.0 * np.sum(b.astype(np.longdouble)) ** 2)) < 1e-15 * 3.0 * np.sum(b) ** 2


def test_xcorr_np_is_the_oracles():
    rng = np.random.default_rng(5)
    for n, m in ((700, 2), (700, 63), (1500, 256), (1500, 257), (984, 984)):
        hay = rng.standard_normal(n) + 1.0
        needle = np.repeat(rng.integers(0, 2, (m + 36) // 37).astype(np.float64) * 233 + 11, 37)[:m] / 255
        # (the oracle's default energy is a difference of running sums over the whole window: 1e-9, the stage's own tolerance)
        for exact, tol in ((True, 1e-12), (False, 1e-9)):
            assert np.max(np.abs(S.xcorr_np(hay, needle) - O.xcorr_norm(hay, needle, exact_energy=exact))) < tol


def test_tail_np_is_the_oracles_pick_on_an_apt_window():
    """A window of synthetic APT envelope around one sync word, shorter than 0.45 s: the oracle's __correlateAndFindPeaks with the
    extras finds one peak; tail_np names the same index, height and post-sync mean."""
    fs = 20800.0
    needle = O.sync_needle(O.NOAA_SYNCA, fs)
    m = len(needle)
    rng = np.random.default_rng(3)
    for lead, n in ((1500, 6000), (200, 5000), (4200, 6000)):
        assert n < 0.45 * fs
        env = 0.3 + 0.05 * rng.standard_normal(n)
        env[lead:lead + m] += 0.5 * needle
        peaks, heights, tsync = O.correlate_and_find_peaks(env, fs, O.NOAA_SYNCA, extra=True)
        assert len(peaks) == 1 and abs(int(peaks[0]) - lead) <= 2
        i, h, ts, gap = S.tail_np(env, env, needle)
        assert i == int(peaks[0]) and gap > 0
        assert abs(h - heights[0]) < 1e-12
        if tsync[0] is None:
            assert np.isnan(ts) and i + 2 * m >= n
        else:
            assert abs(float(ts) - tsync[0]) < 1e-14


def test_pick_np_edges():
    """ties (first index, threshold from m2 == m1), the no-candidate and NaN answers, the end-of-window rule"""
    env = np.arange(40.0)
    cor = np.zeros(40)
    cor[[7, 21]] = 1.0
    assert S.pick_np(cor, env, 4)[:2] == (5, 1.0) and S.pick_np(cor, env, 4)[3] == 0.0
    assert float(S.pick_np(cor, env, 4)[2]) == np.mean(env[9:13])
    assert S.pick_np(np.full(40, 0.25), env, 4)[0] == S.INT64_MIN and np.isnan(S.pick_np(np.full(40, 0.25), env, 4)[1])
    cor[30] = np.nan
    assert S.pick_np(cor, env, 4)[0] == S.INT64_MIN
    cor = np.zeros(40)
    cor[34] = 1.0                                                     # i = 32: i + 2 m = 40 = n, no mean
    assert S.pick_np(cor, env, 4)[0] == 32 and np.isnan(S.pick_np(cor, env, 4)[2])
    cor = np.zeros(40)
    cor[33] = 1.0                                                     # i = 31: i + 2 m = 39 < n
    assert float(S.pick_np(cor, env, 4)[2]) == np.mean(env[35:39])
    cor = np.zeros(40)
    cor[1] = 1.0                                                      # negative index
    assert S.pick_np(cor, env, 4)[0] == -1 and float(S.pick_np(cor, env, 4)[2]) == np.mean(env[3:7])
