"""The SSTV chain on the device (dd_sstv.h through the C entries dd_sstv_lag, _classes, _runs, _pixels, _color, the wrappers of
directdemod_amd/sstv.py and decode_sstv) against the NumPy restatement in sstv.py.

The chain is defined so that no operation depends on a library (float64 + - * / comparisons, ceil and
rint, each rounded on its own; integers behind that), so every comparison is exact: bit patterns for the lag product, np.array_equal
for everything else.  The only tolerance is the end-to-end recording's distance from the picture that was sent, which
tests/test_sstv_host.py measures through a NumPy front end and this file doubles."""
import ctypes as C

import numpy as np
import pytest

import test_sstv_host as th
from directdemod_amd import sstv

pytestmark = pytest.mark.gpu

SPARE = 16
SENT_F = np.float64(-7.25e300)
SENT_I = np.int64(-0x5A5A5A5A5A5A5A5B)
RATE = th.RATE


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.int64)


def _taps(K, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(K), rng.standard_normal(K)


def dev_lag(hip, x, hr, hi):
    """dd_sstv_lag -> (re, im), with SPARE sentinel pairs behind the output checked"""
    n, K = len(x), len(hr)
    dx = hip.DevArray.from_host(np.ascontiguousarray(x, dtype=np.float64)) if n else hip.DevArray(1, np.float64)
    out = hip.DevArray.from_host(np.full(2 * (n + SPARE), SENT_F))
    taps = np.ascontiguousarray(np.concatenate((hr, hi)))
    hip.check(hip.lib().dd_sstv_lag(dx.ptr, n, _pd(taps), K, out.ptr, None), "dd_sstv_lag")
    got = out.to_host()
    assert np.array_equal(_bits(got[2 * n:]), _bits(np.full(2 * SPARE, SENT_F))), "written past n"
    return got[0:2 * n:2], got[1:2 * n:2]


def same_floats(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


# ------------------------------------------------------------------------------------------------------------------ dd_sstv_lag
@pytest.mark.parametrize("K", [1, 3, 131, 511])
def test_lag_lengths(hip, K):
    hr, hi = _taps(K, K)
    T = sstv.LAG_TILE
    x = np.random.default_rng(K + 1).standard_normal(2 * T + 3)
    for n in sorted({0, 1, K - 1, K, K + 1, T - 1, T, T + 1, 2 * T + 3}):
        gr, gi = dev_lag(hip, x[:n], hr, hi)
        wr, wi = sstv.lag_host(x[:n], hr, hi)
        assert same_floats(gr, wr) and same_floats(gi, wi), (K, n)


def test_lag_designed_taps_and_nan(hip):
    hr, hi = sstv.design(RATE)
    K = len(hr)
    x = sstv.synth([1200.0, 1900.0, 2300.0], [0.01, 0.012, 0.01], RATE)
    gr, gi = dev_lag(hip, x, hr, hi)
    wr, wi = sstv.lag_host(x, hr, hi)
    assert same_floats(gr, wr) and same_floats(gi, wi)
    at = 300
    x[at] = np.nan
    gr, gi = dev_lag(hip, x, hr, hi)
    wr, wi = sstv.lag_host(x, hr, hi)
    assert same_floats(gr, wr) and same_floats(gi, wi)
    bad = np.isnan(gr) | np.isnan(gi)
    assert np.array_equal(np.nonzero(bad)[0], np.arange(at, at + K + 1))    # d[n] reads x[n - K .. n]: those windows, no other


def test_lag_bad_arguments(hip):
    L = hip.lib()
    x, out, taps = hip.DevArray.from_host(np.ones(8)), hip.DevArray(16, np.float64), np.ones(2 * 513)
    assert L.dd_sstv_lag(x.ptr, -1, _pd(taps), 3, out.ptr, None) == hip.DD_ERR_INVALID
    for K in (0, 2, 510, 513, -3):
        assert L.dd_sstv_lag(x.ptr, 8, _pd(taps), K, out.ptr, None) == hip.DD_ERR_INVALID, K
    assert L.dd_sstv_lag(None, 8, _pd(taps), 3, out.ptr, None) == hip.DD_ERR_INVALID
    assert L.dd_sstv_lag(x.ptr, 8, _pd(taps), 3, None, None) == hip.DD_ERR_INVALID
    assert L.dd_sstv_lag(x.ptr, 8, None, 3, out.ptr, None) == hip.DD_ERR_INVALID
    assert L.dd_sstv_lag(None, 0, _pd(taps), 3, None, None) == hip.DD_OK


# ------------------------------------------------------------------------------------------------------------------ dd_sstv_classes
def dev_classes(hip, dr, di, e):
    n = len(dr)
    d = np.empty(2 * n)
    d[0::2], d[1::2] = dr, di
    dd = hip.DevArray.from_host(d) if n else hip.DevArray(2, np.float64)
    out = hip.DevArray.from_host(np.full(n + SPARE, 77, dtype=np.int8))
    hip.check(hip.lib().dd_sstv_classes(dd.ptr, n, _pd(np.ascontiguousarray(e)), out.ptr, None), "dd_sstv_classes")
    got = out.to_host()
    assert np.all(got[n:] == 77)
    return got[:n]


def test_classes_edges_and_specials(hip):
    e = sstv.edges(RATE)
    w = 2 * np.pi / RATE
    pts = []
    for f in sstv.EDGES_HZ:
        for df in (0.0, 1e-7, -1e-7, 1e-3, -1e-3):
            for r in (1.0, 3e-200, 7e150):
                pts.append((r * np.cos(w * (f + df)), r * np.sin(w * (f + df))))
    for j in range(6):                                                   # the edge phasors themselves, and one unit in the last place off
        for r in (1.0, 0.3):
            pts.append((r * e[j], r * e[6 + j]))
        pts.append((np.nextafter(e[j], 2.0), e[6 + j]))
        pts.append((np.nextafter(e[j], -2.0), e[6 + j]))
    centres = [(np.cos(w * f), np.sin(w * f)) for f in (1100.0, 1200.0, 1300.0, 1900.0, 1500.0, 2300.0, 500.0)]
    special = [(0.0, 0.0), (1.0, 0.0), (-1.0, 0.0), (0.5, -0.5), (-0.5, -1e-300), (np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan),
               (np.inf, 1.0), (1.0, np.inf), (-np.inf, np.inf), (0.0, 1.0), (-1.0, 1e-9)]
    dr, di = (np.array(v) for v in zip(*(pts + centres + special)))
    got = dev_classes(hip, dr, di, e)
    assert np.array_equal(got, sstv.classes_host(dr, di, e))
    k = len(pts)
    assert list(got[k:k + 7]) == [sstv.CLS_1100, sstv.CLS_1200, sstv.CLS_1300, sstv.CLS_LEADER, 0, 0, 0]
    assert list(got[k + 7:k + 15]) == [0] * 8                              # zero, imaginary part <= 0, NaN
    rng = np.random.default_rng(2)
    dr, di = rng.standard_normal(3001), rng.standard_normal(3001)
    assert np.array_equal(dev_classes(hip, dr, di, e), sstv.classes_host(dr, di, e))
    L = hip.lib()
    buf = hip.DevArray(8, np.float64)
    assert L.dd_sstv_classes(buf.ptr, -1, _pd(e), buf.ptr, None) == hip.DD_ERR_INVALID
    assert L.dd_sstv_classes(None, 4, _pd(e), buf.ptr, None) == hip.DD_ERR_INVALID
    assert L.dd_sstv_classes(buf.ptr, 4, _pd(e), None, None) == hip.DD_ERR_INVALID
    assert L.dd_sstv_classes(None, 0, _pd(e), None, None) == hip.DD_OK


# ------------------------------------------------------------------------------------------------------------------ dd_sstv_runs
def dev_runs(hip, cls, target, W, T, cap):
    """-> (return code, count, the whole list: cap + SPARE entries, sentinel where not written)"""
    cls = np.ascontiguousarray(cls, dtype=np.int8)
    dc = hip.DevArray.from_host(cls) if len(cls) else hip.DevArray(1, np.int8)
    pos = hip.DevArray.from_host(np.full(cap + SPARE, SENT_I))
    count = C.c_int64(-1)
    rc = hip.lib().dd_sstv_runs(dc.ptr, len(cls), target, W, T, pos.ptr, cap, C.byref(count), None)
    hip.sync()
    return rc, count.value, pos.to_host()


def check_runs(hip, cls, target, W, T, what):
    want = sstv.runs_host(cls, target, W, T)
    m = len(want)
    for cap in sorted({0, 1, max(m - 1, 0), m, m + 3}):
        rc, count, pos = dev_runs(hip, cls, target, W, T, cap)
        assert count == m, (what, cap, count, m)
        assert rc == (hip.DD_OK if cap >= m else hip.DD_ERR_INVALID), (what, cap, rc)
        k = min(cap, m)
        assert np.array_equal(pos[:k], want[:k]), (what, cap)
        assert np.all(pos[k:] == SENT_I), (what, cap, "written past min(count, cap)")
    return want


def test_runs_shapes(hip):
    W = 20
    for n in (W - 1, W, W + 1):                                          # no window, one, two
        for fill in (0, 2):
            check_runs(hip, np.full(n, fill, dtype=np.int8), 2, W, 14, (n, fill))
    cls = np.zeros(200, dtype=np.int8)
    cls[:25] = 2                                                         # a run touching index 0
    cls[60:80] = 2
    cls[83:103] = 2                                                      # two equal maxima in one run: counts 20 at 60 and at 83
    cls[-22:] = 2                                                        # and one touching the last index
    want = check_runs(hip, cls, 2, W, 14, "ends and a tie")
    assert list(want) == [0, 60, 178]
    assert list(check_runs(hip, cls, 2, W, 20, "full windows only")) == [0, 60, 83, 178]
    assert list(check_runs(hip, cls, 3, W, 1, "class absent")) == []
    assert list(check_runs(hip, np.full(5000, 2, dtype=np.int8), 2, 7, 7, "one run over every block")) == [0]


def test_runs_across_block_edges(hip):
    """runs that start, peak and end either side of the scan's 1024-element blocks, the 256-position launch blocks and the 64-lane
    steps of the peak walk; random classes at two densities; a window longer than a block"""
    rng = np.random.default_rng(8)
    n = 4 * 1024 + 37
    cls = np.zeros(n, dtype=np.int8)
    for at in (250, 1015, 1024, 2040, 3071, 4090):
        cls[at:at + 30] = 2
    cls[1500:1500 + 700] = 2                                             # a run of 700 positions: eleven 64-lane steps
    cls[1700] = 0
    check_runs(hip, cls, 2, 20, 14, "placed")
    for dens, W, T in ((0.5, 16, 10), (0.8, 50, 40), (0.7, 1500, 1050), (0.3, 1, 1)):
        c = (rng.uniform(size=n) < dens).astype(np.int8) * 4
        want = check_runs(hip, c, 4, W, T, (dens, W, T))
        assert len(want) > 0


def test_runs_bad_arguments(hip):
    L = hip.lib()
    cls = hip.DevArray.from_host(np.zeros(64, dtype=np.int8))
    pos = hip.DevArray(8, np.int64)
    cnt = C.c_int64(0)
    bad = [(cls.ptr, -1, 2, 8, 4, pos.ptr, 8), (cls.ptr, 64, 2, 0, 1, pos.ptr, 8), (cls.ptr, 64, 2, 8, 0, pos.ptr, 8),
           (cls.ptr, 64, 2, 8, 9, pos.ptr, 8), (cls.ptr, 64, 2, 8, 4, pos.ptr, -1), (None, 64, 2, 8, 4, pos.ptr, 8),
           (cls.ptr, 64, 2, 8, 4, None, 8)]
    for a in bad:
        assert L.dd_sstv_runs(*a, C.byref(cnt), None) == hip.DD_ERR_INVALID, a
    assert L.dd_sstv_runs(cls.ptr, 64, 2, 8, 4, pos.ptr, 8, None, None) == hip.DD_ERR_INVALID
    assert L.dd_sstv_runs(None, 0, 2, 8, 4, None, 0, C.byref(cnt), None) == hip.DD_OK and cnt.value == 0
    assert L.dd_sstv_runs(cls.ptr, 64, 2, 8, 4, None, 0, C.byref(cnt), None) == hip.DD_OK and cnt.value == 0     # no run, no list


# ------------------------------------------------------------------------------------------------------------------ dd_sstv_pixels
def dev_pixels(hip, dr, di, t0, W, step, c1):
    n, nseg = len(dr), len(t0)
    d = np.empty(2 * n)
    d[0::2], d[1::2] = dr, di
    dd = hip.DevArray.from_host(d) if n else hip.DevArray(2, np.float64)
    dt0 = hip.DevArray.from_host(np.ascontiguousarray(t0, dtype=np.float64))
    out = hip.DevArray.from_host(np.full(nseg * W + SPARE, 0xA5, dtype=np.uint8))
    empty = C.c_int64(-1)
    hip.check(hip.lib().dd_sstv_pixels(dd.ptr, n, dt0.ptr, nseg, W, step, c1, out.ptr, C.byref(empty), None), "dd_sstv_pixels")
    got = out.to_host()
    assert np.all(got[nseg * W:] == 0xA5)
    return got[:nseg * W].reshape(nseg, W), empty.value


@pytest.mark.parametrize("W", [1, 63, 64, 65, 640, 800])
def test_pixels(hip, W):
    """tones of every level so that all 256 outputs occur, then: a start exactly on a sample, before the first sample, a last pixel
    that ends at n, segments past n, intervals of 0 or 1 samples (step 0.4), of 4 or 5 (4.75) and of 40; a stretch of zeros"""
    c1 = RATE / (2 * np.pi)
    n = 36000
    f = 1400.0 + 1000.0 * (np.arange(n) % 3000) / 3000.0                  # below black to above white
    rng = np.random.default_rng(W)
    amp = 1.0 + 0.2 * rng.standard_normal(n)
    dr, di = amp * np.cos(f / c1) + 0.02 * rng.standard_normal(n), amp * np.sin(f / c1) + 0.02 * rng.standard_normal(n)
    dr[9000:9100] = di[9000:9100] = 0.0                                  # D = 0
    di[12000:12040] *= -1.0                                              # below the real axis
    total_empty = 0
    for step in (0.4, 4.75, 40.0):
        span = W * step
        t0 = np.array([0.0, 17.0, 8990.0, 11990.5, -3.25, -2.0 * span, n - span, n - span / 2, n + 5.0, 1234.567, 20000.0 / 3])
        if span > n:
            t0 = t0[:6]
        got, empty = dev_pixels(hip, dr, di, t0, W, step, c1)
        want, wempty = sstv.pixels_host(dr, di, t0, W, step, c1)
        assert np.array_equal(got, want), (W, step, np.argwhere(got != want)[:5])
        assert empty == wempty, (W, step)
        total_empty += empty
    assert total_empty > 0
    if W == 640:
        assert len(np.unique(want)) > 200


def test_pixels_no_samples_and_bad_arguments(hip):
    L = hip.lib()
    c1 = RATE / (2 * np.pi)
    got, empty = dev_pixels(hip, np.zeros(0), np.zeros(0), np.array([0.0, 5.0]), 65, 4.5, c1)
    assert np.all(got == 0) and empty == 130
    got, empty = dev_pixels(hip, np.ones(50), np.full(50, np.nan), np.array([0.0]), 10, 4.5, c1)
    assert np.array_equal(got, sstv.pixels_host(np.ones(50), np.full(50, np.nan), np.array([0.0]), 10, 4.5, c1)[0]) and empty == 0
    buf = hip.DevArray(64, np.float64)
    cnt = C.c_int64(0)
    for a in ((buf.ptr, -1, buf.ptr, 1, 8, 4.5, c1, buf.ptr), (buf.ptr, 4, buf.ptr, -1, 8, 4.5, c1, buf.ptr),
              (buf.ptr, 4, buf.ptr, 1, -8, 4.5, c1, buf.ptr), (buf.ptr, 4, buf.ptr, 1, 8, 0.0, c1, buf.ptr),
              (buf.ptr, 4, buf.ptr, 1, 8, float("nan"), c1, buf.ptr), (buf.ptr, 4, buf.ptr, 1, 8, 4.5, 0.0, buf.ptr),
              (None, 4, buf.ptr, 1, 8, 4.5, c1, buf.ptr), (buf.ptr, 4, None, 1, 8, 4.5, c1, buf.ptr),
              (buf.ptr, 4, buf.ptr, 1, 8, 4.5, c1, None)):
        assert L.dd_sstv_pixels(*a, C.byref(cnt), None) == hip.DD_ERR_INVALID, a
    assert L.dd_sstv_pixels(None, 0, None, 0, 8, 4.5, c1, None, C.byref(cnt), None) == hip.DD_OK and cnt.value == 0


# ------------------------------------------------------------------------------------------------------------------ dd_sstv_color
def test_colour(hip):
    rng = np.random.default_rng(4)
    W, pairs = 67, 5
    lv = rng.integers(0, 256, (pairs, 4, W), dtype=np.uint8)
    corners = np.array([(y, cr, cb, 255 - y) for y in (0, 255) for cr in (0, 255) for cb in (0, 255)] + [(128, 128, 128, 128)],
                       dtype=np.uint8)
    lv[0, :, :9] = corners.T
    dl = hip.DevArray.from_host(lv.ravel())
    got = sstv.color(dl, pairs, W)
    assert got.shape == (2 * pairs, W, 3) and np.array_equal(got, sstv.color_host(lv))
    assert hip.lib().dd_sstv_color(dl.ptr, -1, W, dl.ptr, None) == hip.DD_ERR_INVALID
    assert hip.lib().dd_sstv_color(None, 2, W, dl.ptr, None) == hip.DD_ERR_INVALID
    assert hip.lib().dd_sstv_color(dl.ptr, 2, W, None, None) == hip.DD_ERR_INVALID
    assert hip.lib().dd_sstv_color(None, 0, W, None, None) == hip.DD_OK


# ------------------------------------------------------------------------------------------------------------------ the chain
def same_result(obj, audio, rate, mode=None):
    images, infos = sstv.decode_host(audio, rate, mode)
    got = obj.getImages
    assert len(got) == len(images) and all(np.array_equal(a, b) for a, b in zip(got, images))
    assert obj.imageInfo == infos
    return images, infos


@pytest.mark.parametrize("mode", ["PD50", "PD120"])
@pytest.mark.parametrize("case", ["clean", "noisy", "slant"])
def test_from_audio_equals_restatement(hip, mode, case):
    from directdemod_amd import decode_sstv
    x = th.audio_of(mode, case)
    obj = decode_sstv.decode_sstv.fromAudio(x, RATE)
    images, infos = same_result(obj, x, RATE)
    assert len(images) == 1 and obj.useful == 1 and np.array_equal(obj.getImage, images[0]) and obj.audioRate == RATE
    th.check_errors(obj.getImage, mode, case)
    assert {"front_end", "lag", "classes", "runs", "headers", "pixels", "color"} <= set(obj.timings)
    dev = decode_sstv.decode_sstv.fromAudio(hip.DevArray.from_host(x), RATE, mode)       # a device array, and the mode forced
    same_result(dev, x, RATE, mode)
    assert np.array_equal(dev.audio().to_host(), x)


def test_complete_image_then_a_second_header(hip):
    """all 128 line pairs of PD50, then the header and two pairs of a PD120 image: the first image ends at its row count"""
    from directdemod_amd import decode_sstv
    a, b = th.audio_of("PD50", "clean", pairs=128), th.audio_of("PD120", "clean", pairs=2)
    x = np.concatenate((a, b))
    obj = decode_sstv.decode_sstv.fromAudio(x, RATE)
    images, infos = same_result(obj, x, RATE)
    assert [(i["mode"], i["rows"], i["syncs_expected"], i["syncs_matched"]) for i in infos] == [("PD50", 256, 128, 127), ("PD120", 4, 2, 1)]
    assert images[0].shape == (256, 320, 3)
    th.check_errors(images[0][:8], "PD50", "clean")


def test_noise_cut_forced_and_bad_arguments(hip):
    from directdemod_amd import decode_sstv
    D = decode_sstv.decode_sstv
    noise = np.random.default_rng(9).standard_normal(3 * RATE)
    obj = D.fromAudio(noise, RATE)
    assert obj.getImages == [] and obj.getImage is None and obj.useful == 0 and obj.imageInfo == []
    assert D.fromAudio(np.zeros(0), RATE).getImages == []
    a = th.audio_of("PD50", "clean")
    cut = a[:int(len(a) - 1.5 * sstv.line_time(sstv.MODES["PD50"]) * RATE)]
    _, infos = same_result(D.fromAudio(cut, RATE), cut, RATE)
    assert infos[0]["rows"] == 4
    bare = th.audio_of("PD50", "clean", vis=False)
    _, infos = same_result(D.fromAudio(bare, RATE, "PD50"), bare, RATE, "PD50")
    assert infos[0]["vis"] is None and infos[0]["rows"] == 8
    with pytest.raises(ValueError, match=r"8000.*1\.520"):
        D.fromAudio(np.zeros(10), 8000, "PD120")
    with pytest.raises(ValueError, match="S/s"):
        D.fromAudio(np.zeros(10), 300000)
    with pytest.raises(ValueError, match="PD7"):
        D.fromAudio(np.zeros(10), RATE, "PD7")


def test_iq_end_to_end(hip):
    """a VIS header and 4 line pairs of PD50 as FM (+-3 kHz, amplitude 60, sigma 2 on the u8 grid) at 240 kS/s, 12.5 kHz up, through
    decode_sstv(IQarray, 12500): within twice the restatement's error on this recording through a NumPy front end
    (test_sstv_host.MEASURED), and exactly the restatement fed the device's own audio"""
    from directdemod_amd import decode_sstv, source
    raw, fs, offset = th.iq_recording()
    obj = decode_sstv.decode_sstv(source.IQarray(raw, fs), offset)
    assert obj.audioRate == 24000
    audio = obj.audio().to_host()
    assert abs(len(audio) - len(raw) // 10) <= 2
    images, infos = same_result(obj, audio, obj.audioRate)
    assert len(images) == 1 and infos[0]["mode"] == "PD50" and infos[0]["rows"] == 8 and infos[0]["parity_ok"] is True
    th.check_errors(images[0], "PD50", "iq")
