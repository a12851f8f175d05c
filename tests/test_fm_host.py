"""CPU-side checks of decode_fm, demod_fmAD, medianFilter, blackmanHarrisConv and sink: the names and constructor defaults of the
reference's surface, the recordings behind tests/golden/fm_*.npz, loud failure without a GPU, medianFilter's argument errors before
any device call, and the three sinks against files read back (sink_csv.txt is the reference's own sink.csv output,
tools/gen_golden_fm.py)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import _fm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from directdemod_amd import _hip
    _hip.load()
    return _hip


def _defaults(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}


def test_surface(hip):
    import directdemod_amd
    from directdemod_amd import decode_fm, demod_fm, filters, sink
    assert "decode_fm" in directdemod_amd.__all__ and "sink" in directdemod_amd.__all__
    sig = inspect.signature(decode_fm.decode_fm.__init__)
    assert list(sig.parameters)[:5] == ["self", "sigsrc", "offset", "bw", "audioFreq"]
    assert _defaults(decode_fm.decode_fm.__init__) == dict(bw=None, audioFreq=None, chunkSize=None, use_device_raw=True)
    assert isinstance(decode_fm.decode_fm.getAudio, property)
    assert _defaults(demod_fm.demod_fmAD.__init__) == dict(storeState=True) and callable(demod_fm.demod_fmAD.demod)
    assert _defaults(filters.medianFilter.__init__) == dict(n=5) and callable(filters.medianFilter.applyOn)
    assert _defaults(filters.blackmanHarrisConv.__init__) == dict(n=151) and callable(filters.blackmanHarrisConv.applyOn)
    assert filters.medianFilter.MAX_N >= 255 and filters.medianFilter.MAX_N % 2 == 1
    for cls in (sink.wavFile, sink.image, sink.csv):
        assert isinstance(cls.write, property)
    assert isinstance(sink.image.show, property)
    assert _defaults(sink.csv.__init__) == dict(titles=None)


def test_noaa_and_fm_share_one_loop(hip):
    from directdemod_amd import decode_fm, noaa_sync
    assert noaa_sync.fm_audio_chunks is decode_fm.fm_audio_chunks
    assert "fm_audio_chunks" in inspect.getsource(noaa_sync.noaa_sync.audio)
    assert "fm_audio_chunks" in inspect.getsource(decode_fm.decode_fm)


@pytest.mark.parametrize("name", sorted(_fm.CASES))
def test_recordings_are_the_fixtures(name):
    g = np.load(os.path.join(GOLDEN, "fm_%s.npz" % name))
    raw = _fm.case(name)
    assert raw.shape == (_fm.CASES[name]["n"], 2) and raw.dtype == np.uint8
    assert _fm.sha(raw) == str(g["sha256"])
    assert g["audio"].dtype == np.float64 and int(g["chunk_len"].sum()) == len(g["audio"])
    fs, _, bw, _ = _fm.told(name)
    assert int(g["decim"]) == int(fs / (30000 if bw is None else bw))


def _have_gpu(hip):
    n = ctypes.c_int(0)
    return hip.lib().dd_device_count(ctypes.byref(n)) == 0 and n.value > 0


def test_no_cpu_fallback(hip):
    """Without a GPU the four compute entries raise; nothing silently runs on the host."""
    if _have_gpu(hip):
        pytest.skip("GPU present")
    from directdemod_amd import decode_fm, demod_fm, filters, source
    with pytest.raises(hip.HipError):
        decode_fm.decode_fm(source.IQarray(_fm.case("c")[:4096], 2400000), 0.0).getAudio.signal
    with pytest.raises(hip.HipError):
        demod_fm.demod_fmAD().demod(np.ones(10, dtype=np.complex64))
    with pytest.raises(hip.HipError):
        filters.medianFilter(5).applyOn(np.ones(10))
    with pytest.raises(hip.HipError):
        filters.blackmanHarrisConv(7).applyOn(np.ones(10))


def test_median_filter_argument_errors_need_no_device(hip, monkeypatch):
    """every way applyOn reaches the device -- the library handle, a device allocation, an upload -- is closed off first, so the
    check bites with and without a GPU"""
    from directdemod_amd import filters

    def no_device(*a, **k):
        raise AssertionError("device call before the argument check")
    for mod, name in ((filters, "lib"), (hip, "lib"), (hip, "require_gpu"), (hip, "_pool_alloc")):
        monkeypatch.setattr(mod, name, no_device)
    monkeypatch.setattr(hip.DevArray, "from_host", staticmethod(no_device))
    x = np.ones(16)
    with pytest.raises(ValueError, match=r"^Each element of kernel_size should be odd\.$"):
        filters.medianFilter(4).applyOn(x)
    with pytest.raises(ValueError, match=r"^dtype=complex64 is not supported by medfilt$"):
        filters.medianFilter(5).applyOn(x.astype(np.complex64))
    cap = filters.medianFilter.MAX_N
    for dtype in (np.float64, np.float32):
        with pytest.raises(NotImplementedError, match=str(cap)):
            filters.medianFilter(cap + 2).applyOn(x.astype(dtype))
    with pytest.raises(AssertionError, match="device call"):       # the guard itself: a valid call does reach the device
        filters.medianFilter(5).applyOn(x)


def test_median_entry_rejects_without_a_launch(hip):
    """the C entries classify the width before they touch a buffer: even -> DD_ERR_INVALID, above the cap -> DD_ERR_UNSUPPORTED"""
    lib = hip.lib()
    for fn in (lib.dd_medfilt_f32, lib.dd_medfilt_f64):
        assert fn(None, None, 16, 4, None) == hip.DD_ERR_INVALID
        assert fn(None, None, 16, hip.DD_MEDFILT_MAX + 2, None) == hip.DD_ERR_UNSUPPORTED
        assert fn(None, None, 0, 5, None) == hip.DD_OK


class _Sig:
    """what sink.wavFile reads of a commSignal"""

    def __init__(self, rate, data):
        self.sampRate, self.reads, self._d = rate, 0, data

    @property
    def signal(self):
        self.reads += 1
        return self._d


def test_sink_wav_round_trip(tmp_path):
    import scipy.io.wavfile
    from directdemod_amd import sink
    rng = np.random.Generator(np.random.PCG64(5))
    for data in (rng.standard_normal(1000), (rng.standard_normal(333) * 1000).astype(np.int16), rng.standard_normal(10).astype(np.float32)):
        p = str(tmp_path / ("a_%s.wav" % data.dtype))
        s = _Sig(15000, data)
        w = sink.wavFile(p, s)
        assert w.write is w and s.reads == 1
        rate, back = scipy.io.wavfile.read(p)
        assert rate == 15000 and back.dtype == data.dtype and np.array_equal(back, data)


def test_sink_wav_takes_a_commsignal(tmp_path, hip):
    import scipy.io.wavfile
    from directdemod_amd import comm, sink
    data = np.linspace(-1.0, 1.0, 501)
    p = str(tmp_path / "c.wav")
    sink.wavFile(p, comm.commSignal(20800, data)).write
    rate, back = scipy.io.wavfile.read(p)
    assert rate == 20800 and np.array_equal(back, data)


def test_sink_csv_is_the_references(tmp_path):
    from directdemod_amd import sink
    p = str(tmp_path / "t.csv")
    c = sink.csv(p, [[0, 1, 2, 3], [0.5, -1.25, "x"]], titles=["sample", "value"])
    assert c.write is c
    assert open(p).read() == open(os.path.join(GOLDEN, "sink_csv.txt")).read()
    p2 = str(tmp_path / "u.csv")
    sink.csv(p2, [[1, 2], [3, 4]]).write
    assert open(p2).read() == "1,3,\n2,4,\n"


def test_sink_image_round_trip(tmp_path):
    import sys
    before = "PIL" in sys.modules
    from directdemod_amd import sink
    assert ("PIL" in sys.modules) == before              # importing the module does not import PIL
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(6))
    for mat in (rng.integers(0, 256, size=(13, 29), dtype=np.uint8), rng.integers(0, 256, size=(7, 5, 3), dtype=np.uint8)):
        p = str(tmp_path / ("i%d.png" % mat.ndim))
        im = sink.image(p, mat)
        assert im.write is im
        assert np.array_equal(np.asarray(Image.open(p)), mat)
