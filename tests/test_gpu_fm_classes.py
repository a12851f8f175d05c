"""demod_fmAD, medianFilter and blackmanHarrisConv on the device (dd_fm_angle_diff_c64, dd_medfilt_*, dd_conv_same_*), each against
the NumPy / SciPy statement the reference makes, written out here.

demod_fmAD    np.diff(np.unwrap(np.angle(z))) in float64, differences compared wrapped (the sign at exactly +-pi cannot be pinned
              under a float32 arctangent), 2e-6 rad on every sample: the inputs are exact complex64, the polynomial is good to
              1.5e-7 rad and enters twice, and three float32 roundings at |phi| <= 2 pi (2.4e-7 each: the
              two angles near pi, the difference) come on top -- 1.1e-6 in all.
medianFilter  np.array_equal with scipy.signal.medfilt: the kernel selects, it does no arithmetic.
blackmanHarrisConv   np.convolve(x, w)[s : s + len(x)] in float64; real input within 1e-12 of max|y|, complex input (complex64
              out) within 2e-6 of max|y|: DESIGN.md section 5's FIR bounds.
"""
import warnings

import numpy as np
import pytest
import scipy.signal

pytestmark = pytest.mark.gpu
AD_ABS = 2e-6


@pytest.fixture(scope="module")
def dd():
    from directdemod_amd import _hip
    _hip.require_gpu()
    from directdemod_amd import demod_fm, filters
    return demod_fm, filters, _hip


def _ad_ref(z):
    return np.diff(np.unwrap(np.angle(np.asarray(z).astype(np.complex128))))


def _wrapped(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a, dtype=np.float64) - b))))


def _iq(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 40.0).astype(np.complex64)


# ------------------------------------------------------------------ demod_fmAD
@pytest.mark.parametrize("store", [True, False])
@pytest.mark.parametrize("n", [2, 3, 257, 4099])
def test_fmad_whole(dd, n, store):
    z = _iq(n, n)
    got = dd[0].demod_fmAD(storeState=store).demod(z)
    assert got.dtype == np.float64 and got.shape == (n - 1,)
    assert _wrapped(got, _ad_ref(z)).max() <= AD_ABS


def test_fmad_device_in_device_out(dd):
    hip = dd[2]
    z = _iq(1000, 3)
    out = dd[0].demod_fmAD(storeState=False).demod(hip.DevArray.from_host(z))
    assert isinstance(out, hip.DevArray) and out.dtype == np.float32 and out.n == 999
    assert _wrapped(out.to_host(), _ad_ref(z)).max() <= AD_ABS


@pytest.mark.parametrize("cuts", [(300,), (301,), (1, 2, 300, 301, 4098), (2048,)])
def test_fmad_chunked_equals_whole(dd, cuts):
    """storing calls: the first returns n - 1 values, later ones n (a 1-sample chunk included); together they are the whole"""
    z = _iq(4099, 77)
    whole = _ad_ref(z)
    obj = dd[0].demod_fmAD()
    edges = (0,) + tuple(cuts) + (len(z),)
    parts = []
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        p = obj.demod(z[a:b])
        assert len(p) == (b - a) - (1 if i == 0 else 0)
        parts.append(p)
    got = np.concatenate(parts)
    assert got.shape == whole.shape and _wrapped(got, whole).max() <= AD_ABS
    # the whole through one call gives the very same float32 values: the carried angle is the one the next call would form
    one = dd[0].demod_fmAD().demod(z)
    assert np.array_equal(one, got)


def test_fmad_without_state_every_call_is_alone(dd):
    z = _iq(600, 9)
    obj = dd[0].demod_fmAD(storeState=False)
    for a, b in ((0, 300), (300, 600)):
        got = obj.demod(z[a:b])
        assert got.shape == (b - a - 1,) and _wrapped(got, _ad_ref(z[a:b])).max() <= AD_ABS


def test_fmad_zero_samples_and_half_turns(dd):
    """a sample of exactly zero has angle 0 (the polar discriminator gives 0 on both sides of it, this one the neighbours' angles):
    mid-stream and as the last sample of a chunk; and the sequence of half and quarter turns"""
    z = _iq(64, 5)
    z[10] = 0
    z[31] = 0
    z[40:42] = 0
    ref = _ad_ref(z)
    assert abs(ref[9]) > 1e-3 and abs(ref[10]) > 1e-3              # not what a polar discriminator returns there
    got = dd[0].demod_fmAD(storeState=False).demod(z)
    assert _wrapped(got, ref).max() <= AD_ABS
    assert got[40] == 0.0
    obj = dd[0].demod_fmAD()
    parts = [obj.demod(z[:32]), obj.demod(z[32:])]                 # the carried angle is that of the zero sample
    assert _wrapped(np.concatenate(parts), ref).max() <= AD_ABS
    t = np.array([1, -1, 1, -1j, 1j, -1], dtype=np.complex64)
    for store in (True, False):
        got = dd[0].demod_fmAD(storeState=store).demod(t)
        assert _wrapped(got, _ad_ref(t)).max() <= AD_ABS
        assert np.all(np.abs(got) <= np.pi + AD_ABS)


def test_fmad_empty_input(dd):
    with pytest.raises(IndexError, match="index -1 is out of bounds for axis 0 with size 0"):
        dd[0].demod_fmAD().demod(np.zeros(0, dtype=np.complex64))
    assert dd[0].demod_fmAD(storeState=False).demod(np.zeros(0, dtype=np.complex64)).shape == (0,)
    assert dd[0].demod_fmAD(storeState=False).demod(np.ones(1, dtype=np.complex64)).shape == (0,)


# ------------------------------------------------------------------ medianFilter
def _medfilt(x, n):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                            # "kernel_size exceeds volume extent"
        return scipy.signal.medfilt(x, n)


def _med_lengths(n, tile):
    return sorted({1, 2, max(1, n // 2), n, 4097, tile - 1, tile, tile + 1, 2 * tile + n // 2})


_med_data = {}


def _med_input(kind, dtype):
    """one seeded array per (kind, dtype), sliced for every length (made once, read-only)"""
    key = (kind, np.dtype(dtype))
    if key not in _med_data:
        rng = np.random.Generator(np.random.PCG64(41))
        if kind == "gauss":
            a = rng.standard_normal(4608).astype(dtype)
        else:
            a = rng.integers(-3, 4, size=4608).astype(dtype)      # tie-heavy: 0..3 and their negatives
        a.setflags(write=False)
        _med_data[key] = a
    return _med_data[key]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 3, 5, 31, 255])
def test_median_equals_scipy(dd, n, dtype):
    filters = dd[1]
    tile = filters.medianFilter.TILE
    flt = filters.medianFilter(n)
    for kind in ("gauss", "ties"):
        src = _med_input(kind, dtype)
        for L in _med_lengths(n, tile):
            x = src[:L]
            got = flt.applyOn(x)
            assert got.dtype == np.dtype(dtype) and np.array_equal(got, _medfilt(x, n)), (kind, L)


def test_median_int32_host_array(dd):
    x = _med_input("ties", np.float64)[:3000].astype(np.int32) * 1000
    got = dd[1].medianFilter(5).applyOn(x)
    assert got.dtype == np.int32 and np.array_equal(got, _medfilt(x, 5))


def test_median_device_in_device_out(dd):
    hip = dd[2]
    for dtype in (np.float32, np.float64):
        x = _med_input("gauss", dtype)[:2500]
        out = dd[1].medianFilter(31).applyOn(hip.DevArray.from_host(x))
        assert isinstance(out, hip.DevArray) and out.dtype == np.dtype(dtype) and out.n == len(x)
        assert np.array_equal(out.to_host(), _medfilt(x, 31))


def test_median_above_the_cap(dd):
    filters, hip = dd[1], dd[2]
    cap = filters.medianFilter.MAX_N
    assert cap >= 255
    x = _med_input("gauss", np.float64)[:600]
    with pytest.raises(NotImplementedError, match=str(cap)):
        filters.medianFilter(max(257, cap + 2)).applyOn(x)
    d = hip.DevArray.from_host(x)
    out = hip.DevArray(len(x), np.float64)
    assert hip.lib().dd_medfilt_f64(d.ptr, out.ptr, len(x), cap + 2, None) == hip.DD_ERR_UNSUPPORTED
    assert hip.lib().dd_medfilt_f64(d.ptr, out.ptr, len(x), 4, None) == hip.DD_ERR_INVALID


# ------------------------------------------------------------------ blackmanHarrisConv
def _conv_ref(x, n):
    w = scipy.signal.windows.blackmanharris(n)
    s = (n - 1) // 2
    return np.convolve(np.asarray(x).astype(np.complex128 if np.iscomplexobj(x) else np.float64), w)[s:s + len(x)]


@pytest.mark.parametrize("L", [1, 40, 151, 4099])
@pytest.mark.parametrize("n", [1, 7, 150, 151])
def test_conv_same(dd, n, L):
    filters = dd[1]
    rng = np.random.Generator(np.random.PCG64(1000 * n + L))
    flt = filters.blackmanHarrisConv(n)
    xr = rng.standard_normal(L)
    ref = _conv_ref(xr, n)
    same = scipy.signal.convolve(xr, scipy.signal.windows.blackmanharris(n), mode="same")      # what the reference calls
    assert same.shape == ref.shape and np.abs(same - ref).max() <= 1e-12 * np.abs(ref).max()
    got = flt.applyOn(xr)
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    xc = (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(np.complex64)
    refc = _conv_ref(xc, n)
    gotc = flt.applyOn(xc)
    assert gotc.dtype == np.complex64 and gotc.shape == refc.shape
    assert np.abs(gotc - refc).max() <= 2e-6 * np.abs(refc).max()


def test_conv_same_device_in_device_out_and_stateless(dd):
    filters, hip = dd[1], dd[2]
    x = _iq(3000, 12)
    flt = filters.blackmanHarrisConv()
    d = hip.DevArray.from_host(x)
    a = flt.applyOn(d)
    b = flt.applyOn(d)                                             # no state: the second call gives the same bits
    assert isinstance(a, hip.DevArray) and a.dtype == np.complex64 and a.n == len(x)
    ref = _conv_ref(x, 151)
    assert np.array_equal(a.to_host(), b.to_host())
    assert np.abs(a.to_host() - ref).max() <= 2e-6 * np.abs(ref).max()
