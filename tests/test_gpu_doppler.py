"""frequency_shift on the device (dd_waterfall_u8, dd_band_argmax_f32, dd_nco_c64_ramp) against the reference's own runs on the
recordings of tests/_doppler.py (tests/golden/doppler_*.npz, tools/gen_golden_doppler.py).

Exact: the row count; for the carrier cases a-c the per-row argmax, the smoothed track and correct() (every best/second-best gap
of those fixtures is >= 1e-3, the generator asserts it); two runs of the waterfall; the ramp mixer against the array mixer.
Toleranced: the bin the device picks is within PICK_REL (1e-4, relative, no exclusions) of the reference row's maximum -- for
the BPSK case d, whose flat top has gaps down to 1.6e-4, that is all that can be asked; the waterfall values in the log domain
within LOG_ABS (ten times the largest difference measured over the four cases, below the 5e-4 that is half
the smallest gap the carrier fixtures may have)."""
import os

import numpy as np
import pytest

import _doppler

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(_doppler.CASES)
CARRIER = [n for n in NAMES if "baud" not in _doppler.CASES[n]]
PICK_REL = 1e-4
LOG_ABS = 1.4e-5
WINDOW = 8192


@pytest.fixture(scope="module")
def dd():
    from directdemod_amd import _hip
    _hip.require_gpu()
    from directdemod_amd import frequency_shift, source, comm, chunker
    return frequency_shift, source, comm, chunker, _hip


def _load(name):
    return np.load(os.path.join(GOLDEN, "doppler_%s.npz" % name))


_runs = {}


def _run(dd, name):
    """(source, dopplerTrack, waterfall rows on the host [rows, WINDOW]) of a case, computed once"""
    if name not in _runs:
        fs, source, _, _, _ = dd
        raw = _doppler.case(name)
        g = _load(name)
        assert _doppler.sha(raw) == str(g["sha256"]), "the recording is not the one the fixture was made from"
        src = source.IQarray(raw, _doppler.FS)
        trk = fs.dopplerTrack(src, _doppler.CENTER, _doppler.CHANNEL, _doppler.BANDWIDTH)
        dev, rows = fs.waterfall(src, WINDOW, float(g["every"]))
        _runs[name] = (src, trk, dev.to_host().reshape(rows, WINDOW))
    return _runs[name]


@pytest.mark.parametrize("name", NAMES)
def test_rows_and_picked_bin(dd, name):
    g = _load(name)
    _, trk, wf = _run(dd, name)
    assert wf.shape[0] == int(g["rows"]) == len(trk.argmax)
    band = g["band"]
    pick = trk.argmax
    assert pick.dtype == np.int32 and pick.min() >= 0 and pick.max() < band.shape[1]
    rel = 1.0 - np.exp(band[np.arange(len(pick)), pick] - band.max(axis=1))
    print("case %s: picked bin below the reference row's maximum by at most %.3g (relative)" % (name, rel.max()))
    assert rel.max() <= PICK_REL
    # the device's argmax kernel follows np.argmax's tie rule on the device's own rows
    assert np.array_equal(pick, np.argmax(wf[:, int(g["band_start"]):int(g["band_stop"])], axis=1))
    if name in CARRIER:
        assert np.array_equal(pick, g["argmax"])


@pytest.mark.parametrize("name", CARRIER)
def test_track_and_correct_exact(dd, name):
    fs = dd[0]
    g = _load(name)
    src, trk, _ = _run(dd, name)
    assert np.array_equal(trk.track, g["track"])
    assert [trk.shift(c, k) for c, k in _doppler.POSITIONS] == g["correct"].tolist()
    if name == "a":          # the drop-in functions on the flat u8 view (uploads the recording again: once is enough)
        args = (src.memmap, _doppler.FS, _doppler.CENTER, _doppler.CHANNEL, _doppler.BANDWIDTH)
        assert np.array_equal(fs.find_shift(*args), g["track"])
        c, k = _doppler.POSITIONS[2]
        assert fs.correct(*args, c, k) == g["correct"][2]


@pytest.mark.parametrize("name", NAMES)
def test_waterfall_values(dd, name):
    g = _load(name)
    _, _, wf = _run(dd, name)
    d_band = np.abs(wf[:, int(g["band_start"]):int(g["band_stop"])].astype(np.float64) - g["band"]).max()
    d_seed = np.abs(wf[:, g["cols"]].astype(np.float64) - g["seeded"]).max()
    print("case %s: largest log-domain difference %.3g in the band, %.3g in the seeded columns" % (name, d_band, d_seed))
    assert max(d_band, d_seed) <= LOG_ABS


def test_waterfall_is_deterministic_and_make_fft_matches(dd):
    fs = dd[0]
    src, _, wf = _run(dd, "c")
    g = _load("c")
    again, rows = fs.waterfall(src, WINDOW, float(g["every"]))
    assert again.to_host().tobytes() == wf.tobytes()
    dev = fs.make_fft(WINDOW, _doppler.FS, 250.0, float(g["every"]), src, device=True)
    assert dev.n == rows * WINDOW and dev.dtype == np.float32


def test_last_row_of_a_partial_tail(dd):
    """case a: 326 slices, the last one partial; it counts towards the row it closes and adds nothing.  The last row equals,
    bit for bit, a run over the recording's last full window followed by a single pair (a tail with other content that still
    closes the row); the rows before it equal a run over the recording cut back to its last full window, which closes one row
    fewer."""
    fs = dd[0]
    raw = _doppler.case("a")
    every = float(_load("a")["every"])
    _, _, wf = _run(dd, "a")
    n_full = raw.shape[0] // WINDOW
    assert raw.shape[0] % WINDOW and n_full % 2 == 1                     # the last row is [full, partial]
    one, rows = fs.waterfall(raw[(n_full - 1) * WINDOW:n_full * WINDOW + 1].reshape(-1), WINDOW, every)
    assert rows == 1 and one.to_host().tobytes() == wf[-1].tobytes()
    host = fs.make_fft(WINDOW, _doppler.FS, 250.0, every, raw[:n_full * WINDOW].reshape(-1))
    assert len(host) == n_full // 2 and host[0].dtype == np.float64
    assert np.array_equal(np.asarray(host, dtype=np.float32), wf[:-1])


def test_source_narrowed_to_an_odd_sample_offset(dd):
    """limitData with an odd initOffset hands the kernel a pointer that is 2-byte but not 4-byte aligned: the 16-bit load path
    (low byte I, high byte Q) gives the bits of the 32-bit path over a fresh, aligned upload of the same bytes"""
    fs, source = dd[0], dd[1]
    raw = _doppler.case("a")[:5 * WINDOW]
    n = 4 * WINDOW + 100
    src = source.IQarray(raw, _doppler.FS)
    src.limitData(1, 1 + n)
    assert src.read_device_raw(0, src.length).ptr % 4 == 2
    odd, rows = fs.waterfall(src, WINDOW, 2.0)
    even, rows2 = fs.waterfall(raw[1:1 + n].reshape(-1), WINDOW, 2.0)
    assert rows == rows2 == 2 and odd.to_host().tobytes() == even.to_host().tobytes()


@pytest.mark.parametrize("window, every, n", [(256, 11.0, 256 * 45 + 77), (64, 19.5, 64 * 70), (16, 3.0, 16 * 11 + 5)])
def test_uneven_split_against_float64(dd, window, every, n):
    """rows whose windows do not divide evenly over the segments of the split (11 -> 6 + 5, 20 -> 7 + 7 + 6), small windows
    (4^k) and a tail that closes a row, against the float64 statement of make_fft's sums (_doppler.waterfall_f64).  Bound:
    _doppler.waterfall_check, four times the error of a float32 pipeline on the CPU over the same bytes (a few 1e-7 to 1e-6)."""
    fs = dd[0]
    rng = np.random.Generator(np.random.PCG64(window))
    raw = rng.integers(0, 256, size=2 * n, dtype=np.uint8)
    dev, rows = fs.waterfall(raw, window, every)
    row_len = int(np.ceil(every))
    n_slices = -(-n // window)
    assert rows == n_slices // row_len and rows >= 1
    _doppler.waterfall_check(dev.to_host().reshape(rows, window), raw, window, every, "window %d, rows of %d" % (window, row_len))


def _mixer_input(n):
    rng = np.random.Generator(np.random.PCG64(77))
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * 50


@pytest.mark.parametrize("n", [4099, 256, 1])
@pytest.mark.parametrize("with_chunker", [False, True])
def test_ramp_mixer_equals_array_mixer(dd, n, with_chunker):
    fs, _, comm, chunker, _hip = dd
    x = _mixer_input(n)

    class _Src:
        length = 3 * 4099 + 17

    # rising with the target reached inside the chunk (1e-4 Hz per sample, 0.2 Hz to go), then falling (0.3 Hz to go)
    for start, target in ((73000.0, 73000.2), (73000.2, 72999.9)):
        d = 2000.0 / 20000000 * (1 if target > start else -1)
        r = fs.ramp(start, (start + d) - start, target, n)
        f = start + np.arange(n, dtype=np.float64) * r.delta
        if target > start:
            f[f > target] = target
        else:
            f[f < target] = target
        assert np.any(f == target) == (n > 3100)
        outs = []
        for arg in (r, f):
            ck = None
            if with_chunker:
                ck = chunker.chunker(_Src(), 4099)
                comm.commSignal(_doppler.FS, _mixer_input(4099), ck).offsetFreq(1000.0).signal      # moves the running index on
            outs.append(np.asarray(comm.commSignal(_doppler.FS, x.copy(), ck).offsetFreq(arg).signal))
        assert outs[0].dtype == np.complex64 and outs[0].tobytes() == outs[1].tobytes()
        assert n == 1 and not with_chunker or not np.array_equal(outs[0], x)        # (sample 0 of a fresh signal has phase 0)
        # the C entry point itself, in place
        buf = _hip.DevArray.from_host(x)
        _hip.check(_hip.lib().dd_nco_c64_ramp(buf.ptr, buf.ptr, n, r.start, r.delta, r.target, float(_doppler.FS),
                                              4099 if with_chunker else 0, None), "dd_nco_c64_ramp")
        assert buf.to_host().tobytes() == outs[0].tobytes()
    with pytest.raises(ValueError):
        comm.commSignal(_doppler.FS, x.copy()).offsetFreq(fs.ramp(1.0, 1e-4, 2.0, n + 1))


def test_ramp_mixer_of_no_samples(dd):
    _hip = dd[4]
    buf = _hip.DevArray.from_host(_mixer_input(4))
    _hip.check(_hip.lib().dd_nco_c64_ramp(buf.ptr, buf.ptr, 0, 1.0, 1e-4, 2.0, float(_doppler.FS), 0, None), "dd_nco_c64_ramp")
    assert np.array_equal(buf.to_host(), _mixer_input(4))


def test_track_is_cached(dd):
    g = _load("b")
    _, trk, _ = _run(dd, "b")
    want = dict(zip(_doppler.POSITIONS, g["correct"].tolist()))
    for pos in ((0, 10), (5, 10), (9, 10)):                             # chunk 0, a middle chunk, the last chunk of ten
        assert trk.shift(*pos) == want[pos]
    assert trk.computed == 1 and trk.track is trk.track and trk.argmax is trk.argmax
