"""The Doppler kernels at their edges, against restatements made on the CPU at test time (tests/_doppler.py; no golden files).

k_waterfall_fft / k_waterfall_rows: the bin order at every window size 16..8192 (pure tones, exact argmax); the values of every
window size at the row lengths where the segment split changes (1, 8 | 9, 128 | 129 with its empty sixteenth segment, 130) against
float64, within four times the error of an independent float32 pipeline on the CPU; silence, a constant, unaligned loads (exact).
k_band_argmax_f32: crafted rows -- ties, infinities, zeros of both signs, NaN -- against np.argmax.
k_nco_c64_ramp / k_nco_c64_freqs: against a longdouble restatement past one grid pass, at a running index of 2^40, on ramps that
rise, fall, land exactly on the target and start on it; bound one float32 ulp + 1e-12 |x| per component."""
import numpy as np
import pytest

import _doppler

pytestmark = pytest.mark.gpu
FS = _doppler.FS
WINDOWS = [16 << k for k in range(10)]                  # 16 .. 8192
LONG_ROWS_AT = (16, 32, 128, 2048, 8192)                # rows of 128..130 windows run at these window sizes only (time)


@pytest.fixture(scope="module")
def dd():
    from directdemod_amd import _hip
    _hip.require_gpu()
    from directdemod_amd import frequency_shift, source
    return frequency_shift, source, _hip


def _rows(fs, raw, window, every):
    dev, rows = fs.waterfall(np.asarray(raw).reshape(-1), window, every)
    return dev, rows, dev.to_host().reshape(rows, window)


# ---------------------------------------------------------------- 1. bin order
@pytest.mark.parametrize("n", WINDOWS)
def test_tone_lands_in_its_bin(dd, n):
    """one row per window (every = 1), window r a tone in bin k_r: the row's maximum is column (k_r + n/2) mod n.  In float64 the
    second-largest bin of such a quantised tone is 98.8 % below the peak: a float32 transform cannot flip it, a wrong digit order
    or twiddle index moves or smears it."""
    fs = dd[0]
    if n <= 512:
        bins = np.arange(n)
    else:
        rng = np.random.Generator(np.random.PCG64(n))
        bins = np.concatenate((rng.choice(n, size=64, replace=False), [0, 1, n // 2, n - 1]))
    dev, rows, wf = _rows(fs, _doppler.tones(n, bins), n, 1.0)
    assert rows == len(bins)
    want = (bins + n // 2) % n
    assert np.array_equal(fs.band_argmax(dev, rows, n, 0, n), want)
    assert np.array_equal(np.argmax(wf, axis=1), want)


# ---------------------------------------------------------------- 2. values
def _value_cases(n):
    """(row length, every, samples): two rows each; for 9 and 129 also a recording one pair longer than its last full window,
    whose partial slice closes the second row"""
    out = [(1, 1.0, 2 * n), (1, 0.5, 2 * n)]
    for row_len in (8, 9) + ((128, 129, 130) if n in LONG_ROWS_AT else ()):
        out.append((row_len, row_len - 0.5, 2 * row_len * n))
        if row_len in (9, 129):
            out.append((row_len, row_len - 0.5, (2 * row_len - 1) * n + 1))
    return out


_VALUE_CASES = [(n, k) for n in WINDOWS for k in range(len(_value_cases(n)))]
_value_bytes = {}


def _value_recordings(n):
    """the recordings of a window size's cases, drawn in case order from one generator seeded by the window size (made once)"""
    if n not in _value_bytes:
        rng = np.random.Generator(np.random.PCG64(1000 + n))
        _value_bytes[n] = [rng.integers(0, 256, size=2 * samples, dtype=np.uint8) for _, _, samples in _value_cases(n)]
    return _value_bytes[n]


def _value_id(p):
    row_len, every, samples = _value_cases(p[0])[p[1]]
    return "%d-rows%d-every%.1f%s" % (p[0], row_len, every, "-tail" if samples % p[0] else "")


@pytest.mark.parametrize("case", _VALUE_CASES, ids=_value_id)
def test_values_against_float64(dd, case):
    """random bytes; the split of a row into segments at 8 (one segment), 9 (5 + 4), 128 (16 x 8), 129 (the cap: 16 segments of
    9, the last one past the row's end) and 130; every <= 1.  Bound: _doppler.waterfall_check, four times the figure of a
    float32 pipeline on the CPU, per case.

    A row of one window is the log of single bins, and random bytes do produce bins hundreds of times below the spectrum's rms
    (the first window of [256-rows1-every1.0] has one of magnitude 6.04 under an rms of 1694): a float32 transform, off by
    1e-7 of the rms in every bin, missed this bound there by a factor 8 (2.68e-5 against 4 x 8.49e-7), which is why
    k_waterfall_fft transforms in float64."""
    fs = dd[0]
    n, k = case
    row_len, every, samples = _value_cases(n)[k]
    raw = _value_recordings(n)[k]
    _, rows, wf = _rows(fs, raw, n, every)
    assert rows == 2
    what = "window %d, rows of %d, every %.1f%s" % (n, row_len, every, ", partial tail" if samples % n else "")
    _doppler.waterfall_check(wf, raw, n, every, what)


# ---------------------------------------------------------------- 3. exact cases
@pytest.mark.parametrize("n", [16, 8192])
def test_silence_is_minus_infinity(dd, n):
    """all bytes 127: every sample is 0 + 0j, every sum 0, every output log(0) = -inf, and the first column of any band wins"""
    fs = dd[0]
    raw = np.full(2 * (3 * 9 * n), 127, dtype=np.uint8)
    dev, rows, wf = _rows(fs, raw, n, 8.5)
    assert rows == 3 and np.all(np.isneginf(wf))
    for a, b in ((0, n), (5, 6), (3, n), (n - 1, n)):
        assert np.array_equal(fs.band_argmax(dev, rows, n, a, b), np.zeros(rows, dtype=np.int32))


def _segment_sum_f32(m, row_len, full):
    """`full` windows of magnitude m (float32) summed like the kernels: the split of a row of `row_len` into segments, each summed
    from zero in window order, the segments then added in order"""
    nseg = min(16, -(-row_len // 8))
    per = -(-row_len // nseg)
    parts = []
    for seg in range(nseg):
        acc = np.float32(0)
        for _ in range(seg * per, min(min((seg + 1) * per, row_len), full)):
            acc = np.float32(acc + m)
        parts.append(acc)
    s = parts[0]
    for p in parts[1:]:
        s = np.float32(s + p)
    return s


@pytest.mark.parametrize("n", [32, 8192])
def test_constant_gives_one_column(dd, n):
    """all bytes 130: every sample is 3 + 3j.  Bin 0 is n (3 + 3j), formed from integers below 2^24 (exact); every butterfly
    difference is exactly zero, so every other column is log(0).  Rows of 9 (every 8.5), the second one closed by a partial
    slice and one window short."""
    fs = dd[0]
    every = 8.5
    raw = np.full(2 * (17 * n + 1), 130, dtype=np.uint8)
    _, rows, wf = _rows(fs, raw, n, every)
    assert rows == 2
    m = np.float32(np.sqrt(18.0 * n * n))                 # |n (3 + 3j)| from the float64 transform, rounded as the kernel adds it
    for r, full in ((0, 9), (1, 8)):
        s = _segment_sum_f32(m, 9, full)
        want = np.float32(np.log(np.float64(s) / n / every))
        # (nine float32 additions, one square root and one store: below 1e-6 of the closed form)
        assert abs(float(want) - np.log(np.sqrt(18.0) * n * full / n / every)) < 1e-6
        got = wf[r, n // 2]
        print("window %d, %d full windows: column n/2 %.9g, expected %.9g" % (n, full, got, want))
        assert abs(float(got) - float(want)) <= float(np.spacing(want))
        others = np.delete(wf[r], n // 2)
        assert np.all(np.isneginf(others))


@pytest.mark.parametrize("n", [32, 512])
def test_unaligned_loads_at_small_windows(dd, n):
    """a source narrowed to an odd sample offset starts 2 bytes off a 4-byte boundary: the 16-bit load path gives the bits of the
    32-bit path over a fresh upload of the same bytes (rows of 10 windows in two segments, a partial tail)"""
    fs, source = dd[0], dd[1]
    rng = np.random.Generator(np.random.PCG64(2000 + n))
    count = 20 * n + 3
    raw = rng.integers(0, 256, size=(count + 5, 2), dtype=np.uint8)
    src = source.IQarray(raw, FS)
    src.limitData(1, 1 + count)
    assert src.read_device_raw(0, src.length).ptr % 4 == 2
    odd, rows = fs.waterfall(src, n, 9.5)
    even, rows2 = fs.waterfall(raw[1:1 + count].reshape(-1), n, 9.5)
    assert rows == rows2 == 2
    assert odd.to_host().tobytes() == even.to_host().tobytes()
    _doppler.waterfall_check(odd.to_host().reshape(rows, n), raw[1:1 + count].reshape(-1), n, 9.5, "window %d, odd offset" % n)


# ---------------------------------------------------------------- 4. the band argmax on crafted rows
WIDTHS = (16, 300, 8192)


def _bands(w):
    """[0, w), [5, 6), 255 columns from 3, 257 columns from 1, [w - 1, w); a band that a row of 16 cannot hold ends at the row's end"""
    out = []
    for a, b in ((0, w), (5, 6), (3, 3 + 255), (1, 1 + 257), (w - 1, w)):
        if (a, min(b, w)) not in out:
            out.append((a, min(b, w)))
    return out


def _argmax(dd, rows, a, b):
    fs, _hip = dd[0], dd[2]
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    dev = _hip.DevArray.from_host(rows.reshape(-1))
    return fs.band_argmax(dev, rows.shape[0], rows.shape[1], a, b)


def _against_numpy(dd, rows, a, b):
    rows = np.asarray(rows, dtype=np.float32)
    got = _argmax(dd, rows, a, b)
    want = np.argmax(rows[:, a:b], axis=1)
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "band [%d, %d) of %d: row %d gives %d, np.argmax %d (%d rows differ)" % (
        a, b, rows.shape[1], bad[0], got[bad[0]], want[bad[0]], bad.size)
    assert got.min() >= 0 and got.max() < b - a


class _Rows:
    """rows of seeded noise in [-1, 1) with chosen values put at chosen columns (columns outside the row are left out)"""

    def __init__(self, w, seed):
        self.w = w
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.rows = []

    def put(self, cols, val=2.0, second=None):
        r = self.rng.uniform(-1.0, 1.0, self.w).astype(np.float32)
        for c in cols:
            if 0 <= c < self.w:
                r[c] = val
        for c, v in (second or ()):
            if 0 <= c < self.w:
                r[c] = v
        self.rows.append(r)


def _pair_starts(a, b, d):
    """first columns c of a pair (c, c + d): both in the band where it is wide enough, and one of the two just outside it"""
    return sorted({a, a + 1, (a + b) // 2, b - 1 - d, b - d, a - 1, a - d})


@pytest.mark.parametrize("w", WIDTHS)
def test_argmax_of_crafted_rows(dd, w):
    for a, b in _bands(w):
        R = _Rows(w, 31 * w + a)
        mid = (a + b) // 2
        for _ in range(1000 if w == 300 else 40):
            R.rows.append(R.rng.standard_normal(w).astype(np.float32))
        for _ in range(40):                                       # three values only: ties everywhere
            R.rows.append(R.rng.integers(0, 3, w).astype(np.float32))
        for d in (1, 256, 128):                                   # neighbours; one lane's stride; the reduction's first step
            for c in _pair_starts(a, b, d):
                R.put((c, c + d))
        R.put((a, b - 1))                                         # the band's first and last column
        R.put((a - 1,)), R.put((b,)), R.put((a - 1, b))           # a larger value just outside, the band's own maximum is noise
        R.put((a - 1, b), second=((mid, 1.5), (b - 1, 1.5)))
        R.put((mid,), np.inf), R.put((a, b - 1), np.inf), R.put((mid, mid + 1, mid + 256), np.inf)
        R.put((a - 1, b), np.inf, second=((b - 1, 2.0),))
        R.rows.append(np.full(w, -np.inf, dtype=np.float32))
        R.put((mid,), -np.inf), R.put((a,), -np.inf)
        r = np.full(w, -np.inf, dtype=np.float32)
        r[b - 1] = -3.0e38
        R.rows.append(r)
        for first, then in ((0.0, -0.0), (-0.0, 0.0)):            # +0.0 == -0.0: the first one wins
            r = np.full(w, -1.0, dtype=np.float32)
            r[b - 1] = then
            r[a] = first
            R.rows.append(r)
            r = np.full(w, then, dtype=np.float32)
            r[mid] = first
            R.rows.append(r)
        R.rows.append(np.full(w, 3.25, dtype=np.float32))         # one repeated value
        R.rows.append(np.full(w, -3.4e38, dtype=np.float32))
        _against_numpy(dd, np.stack(R.rows), a, b)


@pytest.mark.parametrize("w", WIDTHS)
def test_argmax_with_nan_follows_numpy(dd, w):
    """np.argmax counts a NaN as the largest value: the first NaN of the band wins, NaNs outside the band are not seen, and an
    all-NaN band gives 0 -- never an index outside the band"""
    nan = np.float32(np.nan)
    for a, b in _bands(w):
        R = _Rows(w, 57 * w + a)
        mid = (a + b) // 2
        for m in sorted({a, mid, b - 1}):                         # the maximum at m, one NaN below or above it
            for q in sorted({a, a + 1, m - 1, m + 1, m - 256, m + 256, m - 128, m + 128, b - 1}):
                if q != m:
                    R.put((m,), 2.0, second=((q, nan),))
        for d in (1, 256, 128):                                   # two NaNs
            for c in _pair_starts(a, b, d):
                R.put((c, c + d), nan)
        R.put((a, b - 1), nan)
        R.put((a - 1,), nan), R.put((b,), nan), R.put((a - 1, b), nan)          # NaN outside the band only
        R.put((mid,), np.inf, second=((b - 1, nan),)), R.put((b - 1,), np.inf, second=((a, nan),))
        R.put((mid,), nan, second=((a, -np.inf),))
        R.rows.append(np.full(w, nan, dtype=np.float32))          # all NaN
        r = R.rng.uniform(-1.0, 1.0, w).astype(np.float32)        # the band all NaN, the rest numbers
        r[a:b] = nan
        R.rows.append(r)
        r = np.full(w, -np.inf, dtype=np.float32)
        r[b - 1] = nan
        R.rows.append(r)
        for _ in range(40):                                       # NaN sprinkled over noise, one column in 64
            r = R.rng.standard_normal(w).astype(np.float32)
            r[R.rng.random(w) < 1.0 / 64] = nan
            R.rows.append(r)
        _against_numpy(dd, np.stack(R.rows), a, b)


def test_argmax_entry_point(dd):
    _hip = dd[2]
    lib = _hip.lib()
    rows = _hip.DevArray.from_host(np.arange(64, dtype=np.float32))
    out = _hip.DevArray.from_host(np.full(4, -77, dtype=np.int32))
    _hip.check(lib.dd_band_argmax_f32(rows.ptr, 0, 16, 0, 16, out.ptr, None), "dd_band_argmax_f32")      # no rows: nothing touched
    _hip.check(lib.dd_band_argmax_f32(None, 0, 16, 0, 16, None, None), "dd_band_argmax_f32")
    _hip.sync()
    assert np.array_equal(out.to_host(), np.full(4, -77, dtype=np.int32))
    for a, b in ((5, 5), (6, 5), (-1, 4), (0, 17), (16, 17)):
        with pytest.raises(ValueError):
            _hip.check(lib.dd_band_argmax_f32(rows.ptr, 4, 16, a, b, out.ptr, None), "dd_band_argmax_f32")
    _hip.sync()
    assert np.array_equal(out.to_host(), np.full(4, -77, dtype=np.int32))
    _hip.check(lib.dd_band_argmax_f32(rows.ptr, 4, 16, 0, 16, out.ptr, None), "dd_band_argmax_f32")
    _hip.sync()
    assert np.array_equal(out.to_host(), np.full(4, 15, dtype=np.int32))


# ---------------------------------------------------------------- 5. the mixers
STARTS = (0, 4099, 2 ** 40 + 12345)
RAMPS = {           # name -> (f0, delta, target); delta as dopplerRamp forms it, (start + d) - start
    "rising": (73000.0, (73000.0 + 1e-4) - 73000.0, 73000.2),                   # reaches the target near sample 2000
    "falling": (73000.2, (73000.2 - 1e-4) - 73000.2, 72999.9),                  # near sample 3000
    "lands": (73000.0, 2.0 ** -13, 73000.25),                                   # f0 + 2048 delta == target, all exact in binary
    "at target": (73000.0, (73000.0 - 1e-4) - 73000.0, 73000.0),                # target == start: every sample at the target
}
_ulps = {}


def _mixer_input(n):
    rng = np.random.Generator(np.random.PCG64(78))
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * 50


def test_ramps_are_what_they_claim():
    """(CPU) the exact landing, the clipping of the other ramps inside 4099 samples"""
    f0, delta, target = RAMPS["lands"]
    raw = f0 + np.arange(4099, dtype=np.float64) * delta
    assert np.nonzero(raw == target)[0].tolist() == [2048]
    assert np.array_equal(_doppler.ramp_freqs(f0, delta, target, 4099)[2048:], np.full(2051, target))
    for name in ("rising", "falling"):
        f = _doppler.ramp_freqs(*RAMPS[name], 4099)
        assert f[0] == RAMPS[name][0] and f[1] != f[0] and f[-1] == RAMPS[name][2] and f[255] != RAMPS[name][2]
    assert np.array_equal(_doppler.ramp_freqs(*RAMPS["at target"], 255), np.full(255, 73000.0))


@pytest.mark.parametrize("n", [1, 255, 4099, 2048 * 256 + 257])
def test_mixers_against_longdouble(dd, n):
    """both kernels, every start index and ramp: |got - want| <= ulp32(want) + 1e-12 |x| per component (one float32 rounding,
    the rare double rounding; the float64 sincospi and multiply-add).  2048 * 256 + 257 samples is one grid pass and a lane more."""
    _hip = dd[2]
    lib = _hip.lib()
    x = _mixer_input(n)
    xd = _hip.DevArray.from_host(x)
    ax = np.abs(x).astype(np.float64)
    for start in STARTS:
        for name, (f0, delta, target) in RAMPS.items():
            f = _doppler.ramp_freqs(f0, delta, target, n)
            out = _hip.DevArray(n, np.complex64)
            _hip.check(lib.dd_nco_c64_ramp(xd.ptr, out.ptr, n, f0, delta, target, float(FS), start, None), "dd_nco_c64_ramp")
            ramp = out.to_host()
            fd = _hip.DevArray.from_host(f)
            out2 = _hip.DevArray(n, np.complex64)
            _hip.check(lib.dd_nco_c64_freqs(xd.ptr, out2.ptr, n, fd.ptr, float(FS), start, None), "dd_nco_c64_freqs")
            arr = out2.to_host()
            assert ramp.tobytes() == arr.tobytes(), (name, start)
            re, im = _doppler.mixer_expected(x, f, start, FS)
            for kernel, got in (("ramp", ramp), ("array", arr)):
                for part, g, want in (("re", got.real, re), ("im", got.imag, im)):
                    err = np.abs(g.astype(np.longdouble) - want).astype(np.float64)
                    ulp = _doppler.ulp32(want.astype(np.float64))
                    worst = float((err / ulp).max())
                    _ulps[(kernel, n, start, name, part)] = worst
                    bad = np.nonzero(err > ulp + 1e-12 * ax)[0]
                    assert bad.size == 0, "%s kernel, %s, start %d, %s: sample %d off by %.3g ulp (%d samples)" % (
                        kernel, name, start, part, bad[0], err[bad[0]] / ulp[bad[0]], bad.size)
    k = max(_ulps, key=_ulps.get)
    print("n = %d: largest mixer error so far %.3f float32 ulp %s" % (n, _ulps[k], k))


def test_mixers_in_place_and_of_no_samples(dd):
    """in place (in == out) gives the bits of out of place; n = 0 touches nothing"""
    _hip = dd[2]
    lib = _hip.lib()
    n = 4099
    x = _mixer_input(n)
    f0, delta, target = RAMPS["lands"]
    out = _hip.DevArray(n, np.complex64)
    xd = _hip.DevArray.from_host(x)
    _hip.check(lib.dd_nco_c64_ramp(xd.ptr, out.ptr, n, f0, delta, target, float(FS), STARTS[2], None), "dd_nco_c64_ramp")
    _hip.check(lib.dd_nco_c64_ramp(xd.ptr, xd.ptr, n, f0, delta, target, float(FS), STARTS[2], None), "dd_nco_c64_ramp")
    assert out.to_host().tobytes() == xd.to_host().tobytes()
    fd = _hip.DevArray.from_host(_doppler.ramp_freqs(f0, delta, target, n))
    _hip.check(lib.dd_nco_c64_freqs(xd.ptr, xd.ptr, 0, fd.ptr, float(FS), 0, None), "dd_nco_c64_freqs")
    assert out.to_host().tobytes() == xd.to_host().tobytes()
