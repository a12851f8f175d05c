"""
Plain restatements of two stages of the accurate-sync batch (csrc/dd_audio_sync.h), for the tests of their kernels:

* filtfilt_ld -- the zero-phase FIR's definition (scipy.signal.filtfilt(b, [1], x), filters.py:72-73) written out in
  np.longdouble: odd extension by 3 K, K - 1 copies of the pass's first sample as its history, plain convolution, reverse,
  the same again, reverse, crop.
* tail_np -- decode_noaa.py:671-673 (normalised correlation) and the pick of :713-762 for a window shorter than the
  0.45 s group distance (two expected peaks, one group): first index of the maximum, threshold from the two largest and the
  two smallest values, peak = argmax - m // 2, post-sync mean only when peak + 2 m < n.

tests/test_syncstages_host.py pins both to the oracle (and SciPy) on the CPU.
"""
import numpy as np

LD = np.longdouble
INT64_MIN = -2 ** 63


def cosine_taps_ld(K, a):
    """b[k] = sum_q a[q] cos(2 pi q k / (K - 1)), evaluated in long double (phase reduced exactly: q k mod (K - 1))."""
    k = np.arange(K, dtype=np.int64)
    w = 2 * np.arctan2(LD(0), LD(-1)) / LD(K - 1)
    b = np.zeros(K, LD)
    for q, aq in enumerate(a):
        b += LD(aq) * np.cos(w * ((q * k) % (K - 1)).astype(LD))
    return b


def _pass_ld(b, e):
    """y[i] = sum_k b[k] e[max(i - k, 0)]: lfilter whose history is the first sample (zi * e[0] for a FIR of any gain)"""
    K = len(b)
    h = np.concatenate([np.full(K - 1, e[0], LD), e])
    return np.convolve(h, b)[K - 1:K - 1 + len(e)]


def filtfilt_ld(b, x):
    b = np.asarray(b, LD)
    x = np.asarray(x, LD)
    K, n = len(b), len(x)
    edge = 3 * K
    if n <= edge:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % edge)
    ext = np.concatenate([2 * x[0] - x[edge:0:-1], x, 2 * x[-1] - x[-2:-(edge + 2):-1]])
    y = _pass_ld(b, ext)
    y = _pass_ld(b, y[::-1])[::-1]
    return y[edge:edge + n]


def filtfilt_scale(b, x):
    """s = max|x| (sum|b|)^2: the size a zero-phase output can reach, the unit of the filters' error bounds"""
    return float(np.max(np.abs(np.asarray(x, np.float64))) * float(np.sum(np.abs(np.asarray(b, LD)))) ** 2)


def xcorr_np(hay, needle):
    """decode_noaa.py:671-673, the three lines as they stand (direct sums: exact for integer-valued inputs)"""
    hay = np.asarray(hay, np.float64)
    needle = np.asarray(needle, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cor = np.correlate(hay, needle, "same")
        sums = np.convolve(hay * hay, np.ones(len(needle)), "same")
        return cor / np.sqrt(sums * np.sum(needle * needle))


def pick_np(cor, env, m):
    """(peak, height, tsync, gap) of one window from its correlation; gap = largest - second largest value.  Where the
    reference's code would meet a NaN (argpartition and the comparisons have no answer for one) or find no candidate above
    its threshold (it would append None), the answer is the device's documented triple (INT64_MIN, NaN, NaN).  tsync is the
    long double mean (NaN when the peak lies too close to the end, :755)."""
    n = len(cor)
    nan = float("nan")
    if np.any(np.isnan(cor)):
        return INT64_MIN, nan, LD(nan), nan
    order = np.sort(cor)
    hi = (0.0 + order[-2] + order[-1]) / 2.0                          # mean of the K = 2 largest (:717-721)
    thr = hi - 0.25 * (hi - (0.0 + order[0] + order[1]) / 2.0)        # NOAA_PEAKHEIGHTWIGGLE (:723)
    gap = float(order[-1] - order[-2])
    a = int(np.argmax(cor))                                           # first index of the maximum (:742, strict <)
    if not cor[a] > thr:
        return INT64_MIN, nan, LD(nan), gap
    i = a - m // 2                                                    # :749
    ts = LD(nan)
    if i + 2 * m < n:                                                 # :755
        ts = np.sum(np.asarray(env[i + m:i + 2 * m], LD)) / LD(m)
    return i, float(cor[a]), ts, gap


def tail_np(hay, env, needle):
    return pick_np(xcorr_np(hay, needle), env, len(needle))
