"""Host side of directdemod_amd.frequency_shift (no GPU): rolling_window / correct_shift / the smoothed track against the
reference's own runs (tests/golden/doppler_*.npz, tools/gen_golden_doppler.py), dopplerRamp against NumPy's arange and clip
bit for bit, the inputs the reference cannot handle, and the sources' memmap property."""
import os

import numpy as np
import pytest

import _doppler

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(_doppler.CASES)


@pytest.fixture(scope="module")
def fs():
    from directdemod_amd import frequency_shift
    return frequency_shift


def _load(name):
    return np.load(os.path.join(GOLDEN, "doppler_%s.npz" % name))


def _df():
    xf = np.fft.fftshift(np.fft.fftfreq(8192, 1.0 / _doppler.FS))
    return xf[1] - xf[0]


@pytest.mark.parametrize("name", NAMES)
def test_track_and_positions_from_golden_argmax(fs, name):
    g = _load(name)
    track = fs.smooth_track(g["argmax"], _doppler.BANDWIDTH, _df())
    assert np.array_equal(track, g["track"])
    got = [fs.correct_shift(track, c / k) for c, k in _doppler.POSITIONS]       # position 0, 1 and in between
    assert got == g["correct"].tolist()
    assert fs.correct_shift(track, 0) == track[0] and fs.correct_shift(track, 1) == track[-1]


@pytest.mark.parametrize("n, window", [(163, 16), (250, 25), (30, 3), (11, 1), (12, 7), (8, 8), (9, 12)])
def test_rolling_window_edge_branches(fs, n, window):
    """head (i < window // 2), tail (i > n - window // 2: the mean over the last -window // 2 entries, floor division of the
    NEGATIVE number) and the middle, restated with plain sums"""
    rng = np.random.Generator(np.random.PCG64(n * 100 + window))
    x = list(rng.standard_normal(n) * 40.0)
    got = fs.rolling_window(x, window)
    assert len(got) == n
    for i in range(n):
        if i < window // 2:
            want = np.mean(x[:window])
        elif i > n - window // 2:
            want = np.mean(x[len(x) - ((window + 1) // 2):])
        else:
            want = np.mean(x[i - window // 2:i - window // 2 + window])
        assert got[i] == want, i


def _numpy_ramp(cur, target, n, bw):
    """decode_funcube.py:215-226 with NumPy itself"""
    if target > cur:
        d = bw
        f = np.arange(cur, cur + (n * d) + (10 * d), d)[:n]
        f[f > target] = target
    else:
        d = -1 * bw
        f = np.arange(cur, cur + (n * d) + (10 * d), d)[:n]
        f[f < target] = target
    return f


def _expand(r):
    f = r.start + np.arange(r.n, dtype=np.float64) * r.delta
    if r.target > r.start:
        f[f > r.target] = r.target
    else:
        f[f < r.target] = r.target
    return f


def test_doppler_ramp_against_numpy(fs):
    from directdemod_amd import constants
    bw = 2000.0 / constants.PROC_CHUNKSIZE
    offset = 73200.0
    # first call (starts at the target), rising, rising with the target reached mid-chunk, target == current, falling,
    # falling with the target reached mid-chunk, and a run of three rising chunks: `current` carries over throughout
    steps = [(-2750.0, 4099), (-2749.0, 5000), (-2748.7, 20000), (-2748.7, 333), (-2751.3, 7001), (-2751.9, 60000),
             (3250.0, 100000), (3250.0, 100001), (3250.0, 1)]
    rmp = fs.dopplerRamp(offset)
    cur = None
    kinds = set()
    for shift, n in steps:
        target = offset + shift
        if cur is None:
            cur = target
        want = _numpy_ramp(cur, target, n, bw)
        r = rmp.next(shift, n)
        assert isinstance(r, fs.ramp) and r.n == n and r.start == cur and r.target == target
        got = _expand(r)
        assert got.tobytes() == want.tobytes()
        assert rmp.current == want[-1]
        kinds.add((target > cur, bool(np.any(want == target)) and want[0] != target))
        cur = want[-1]
    assert kinds == {(False, False), (True, False), (True, True), (False, True)}
    with pytest.raises(ValueError):
        rmp.next(0.0, 0)


def test_errors_name_their_case(fs):
    raw = np.full(2 * 8192 * 12, 127, dtype=np.uint8)
    args = (_doppler.FS, _doppler.CENTER, _doppler.CHANNEL, _doppler.BANDWIDTH)
    with pytest.raises(ValueError, match="fewer than 10"):
        fs.find_shift(raw[:2 * 8192 * 9], *args)                       # 9 slices, every < 1: 9 rows, N = 0
    with pytest.raises(ValueError, match="partial last window"):
        fs.make_fft(8192, _doppler.FS, 250.0, 1.0, raw[:2 * 8192 * 3 + 100])
    with pytest.raises(ValueError, match="shorter than one window"):
        fs.make_fft(8192, _doppler.FS, 250.0, 2.0, raw[:2 * 8191])
    with pytest.raises(ValueError, match="leaves"):
        fs.find_shift(raw, _doppler.FS, _doppler.CENTER, _doppler.CENTER + 1020000, _doppler.BANDWIDTH)    # past the top
    with pytest.raises(ValueError, match="leaves"):
        fs.find_shift(raw, _doppler.FS, _doppler.CENTER, _doppler.CENTER - 1020000, _doppler.BANDWIDTH)    # below column 0
    with pytest.raises(ValueError, match="odd number"):
        fs.make_fft(8192, _doppler.FS, 250.0, 2.0, raw[:2 * 8192 * 3 + 1])
    with pytest.raises(ValueError, match="power of two"):
        fs.make_fft(6000, _doppler.FS, 250.0, 2.0, raw)
    with pytest.raises(ValueError, match="fewer than 10"):
        fs.smooth_track(np.arange(9), _doppler.BANDWIDTH, 250.0)


def test_sources_memmap_property(tmp_path):
    from directdemod_amd import source
    rng = np.random.Generator(np.random.PCG64(5))
    raw = rng.integers(0, 256, size=(1000, 2), dtype=np.uint8)
    src = source.IQarray(raw, _doppler.FS)
    assert src.memmap.dtype == np.uint8 and src.memmap.shape == (2000,)
    assert np.array_equal(src.memmap, raw.reshape(-1))
    src.limitData(100, 600)
    assert src.memmap.shape == (2000,)                                  # the whole recording, whatever limitData says
    p = tmp_path / "x.dat"
    raw.tofile(p)
    dat = source.IQdat(str(p))
    assert np.array_equal(dat.memmap, raw.reshape(-1)) and np.shares_memory(dat.memmap, dat._data)
