"""decode_fm.getAudio on the device against the reference's own getAudio runs on the recordings of tests/_fm.py
(tests/golden/fm_*.npz, tools/gen_golden_fm.py), every sample, no exclusions.

Two tiers, because the strict resample of a chunk spreads that chunk's angle errors over that chunk only:
  chunks 1 and later   every product |y[n] conj(y[n-1])| is at least 0.1 of the median there (the generator asserts it), so every
                       angle is in the project's 2e-5 rad tier;
  chunk 0              holds the one to two start-up angles of the 151-tap filter over its history of ones, whose products are
                       down to 4e-4 of the median: the float32 error of y is that much larger in the angle.
Each bound is ten times the largest difference measured on an MI355X over the three cases: LATER_ABS from MEASURED_LATER,
FIRST_ABS from MEASURED_FIRST (below).  The start-up angles do not show: chunk 0 measures what the later chunks do, 2e-7 for audio
peaks of 1.0 to 1.5 rad -- the resample spreads an angle's error over its chunk's few hundred samples.  Whatever is measured, the
bounds may not exceed 2e-4 (later) and 2e-3 (chunk 0) of the audio's peak; the test asserts that too.
"""
import os

import numpy as np
import pytest

import _fm

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(_fm.CASES)
MEASURED_LATER = 2.17e-7      # rad, largest |audio - fixture| in chunks 1.. on an MI355X: a 2.16e-7, b 9.5e-8, c 2.00e-7
MEASURED_FIRST = 2.07e-7      # rad, the same in chunk 0: a 2.06e-7, b 1.07e-7, c 1.99e-7
LATER_ABS = 10 * MEASURED_LATER
FIRST_ABS = 10 * MEASURED_FIRST


@pytest.fixture(scope="module")
def dd():
    from directdemod_amd import _hip
    _hip.require_gpu()
    from directdemod_amd import decode_fm, source
    return decode_fm, source, _hip


def _load(name):
    return np.load(os.path.join(GOLDEN, "fm_%s.npz" % name))


_runs = {}


def _run(dd, name, **kw):
    """(decoder, audio commSignal) of a case, decoded once per route"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _runs:
        dfm, source, _ = dd
        raw = _fm.case(name)
        assert _fm.sha(raw) == str(_load(name)["sha256"]), "the recording is not the one the fixture was made from"
        fs, offset, bw, audioFreq = _fm.told(name)
        obj = dfm.decode_fm(source.IQarray(raw, fs), offset, bw, audioFreq, chunkSize=_fm.CHUNK, **kw)
        _runs[key] = (obj, obj.getAudio)
    return _runs[key]


@pytest.mark.parametrize("name", NAMES)
def test_rate_and_length(dd, name):
    g = _load(name)
    obj, audio = _run(dd, name)
    assert audio.sampRate == int(g["sampRate"]) and audio.length == len(g["audio"])
    assert obj.getAudio is audio                                   # cached on the object
    s = audio.signal
    assert s.dtype == np.float64 and s.shape == g["audio"].shape


@pytest.mark.parametrize("name", NAMES)
def test_audio_against_the_reference(dd, name):
    g = _load(name)
    ref = g["audio"]
    got = _run(dd, name)[1].signal
    n0 = int(g["chunk_len"][0])
    peak = float(np.max(np.abs(ref)))
    d = np.abs(got - ref)
    first, later = float(d[:n0].max()), float(d[n0:].max())
    print("fm_%s: peak %.4f; |audio - reference| chunk 0 %.3g (bound %.3g), later chunks %.3g (bound %.3g)" %
          (name, peak, first, FIRST_ABS, later, LATER_ABS))
    assert LATER_ABS <= 2e-4 * peak and FIRST_ABS <= 2e-3 * peak   # the caps hold whatever was measured
    assert later <= LATER_ABS
    assert first <= FIRST_ABS


@pytest.mark.parametrize("name", NAMES)
def test_plain_read_gives_the_same(dd, name):
    """The chunks uploaded one by one through plain `read` are held to the reference exactly as the resident route is, and the two
    routes to each other within the tighter of those bounds.  Equal bits cannot be promised in general: an uploaded chunk is
    aligned where a slice of the resident recording at an odd offset is not, and short or unaligned chunks take another
    decimating kernel whose NCO phasors round differently (the randomized chunk-loop test); on these three
    recordings the difference measured on an MI355X is 0."""
    g = _load(name)
    ref, n0 = g["audio"], int(g["chunk_len"][0])
    a = _run(dd, name)[1]
    b = _run(dd, name, use_device_raw=False)[1]
    assert a.sampRate == b.sampRate and a.length == b.length == len(ref)
    sa, sb = a.signal, b.signal
    d = float(np.max(np.abs(sa - sb)))
    db = np.abs(sb - ref)
    print("fm_%s: resident raw pairs against plain read: %.3g; plain read against the reference: chunk 0 %.3g, later %.3g" %
          (name, d, db[:n0].max(), db[n0:].max()))
    assert db[n0:].max() <= LATER_ABS and db[:n0].max() <= FIRST_ABS
    assert d <= min(LATER_ABS, FIRST_ABS)


def test_recorded_chunk_loop_is_one_launch(dd):
    """case a over the resident recording: four chunks, ONE fused launch (/68 is not one of the wave-per-row kernels' decimations:
    k_chain_decim_multi); case b's /34 takes the block-sum kernel; chunk by chunk through plain read it is a launch per chunk"""
    hip = dd[2]
    obj = _run(dd, "a")[0]
    assert len(_load("a")["chunk_len"]) == 4
    assert obj._launch_count() == 1
    assert obj._decode_filter()._last_kernel() == hip.DD_KERNEL_DECIM_MULTI
    b = _run(dd, "b")[0]
    assert b._launch_count() == 1 and b._decode_filter()._last_kernel() == hip.decim_wave_kernel(151, 34) == hip.DD_KERNEL_DECIM_BLOCKS
    assert _run(dd, "a", use_device_raw=False)[0]._launch_count() == 4


def test_noaa_audio_is_what_it_was(dd):
    """noaa_sync.audio now calls the loop it shares with decode_fm: bit for bit the loop it held before (restated here with the
    public classes), strict and not, and the crude sync index lists of tests/golden/noaa_c4.npz still come out of the public class"""
    from directdemod_amd import chunker, comm, constants, demod_fm, filters, noaa_sync, source
    from oracle import dd_oracle as O
    g = np.load(os.path.join(GOLDEN, "noaa_c4.npz"))
    raw = O.synth_apt_iq(float(g["dur"]), 2048000, seed=1)
    src = source.IQarray(raw, 2048000)
    ns = noaa_sync.noaa_sync(src, 30000.0)
    sa, sb = ns.getCrudeSync()
    assert np.array_equal(sa, g["crude_syncA"]) and np.array_equal(sb, g["crude_syncB"])

    def before(audioFreq, strictness, chunkSize):
        audioOut = comm.commSignal(audioFreq)
        bh, fm, ck = filters.blackmanHarris(151), demod_fm.demod_fm(), chunker.chunker(src, chunkSize)
        for a, b in ck.getChunks:
            audioOut.extend(comm.commSignal(src.sampFreq, src.read_device_raw(a, b), ck).offsetFreq(30000.0).filter(bh)
                            .bwLim(constants.NOAA_FMBW, uniq="First").funcApply(fm.demod).bwLim(audioFreq, strictness))
        return audioOut
    for audioFreq, strict, chunk in ((constants.NOAA_CRUDESYNCSAMPRATE, False, 300001), (constants.NOAA_AUDSAMPRATE, True, 1 << 20)):
        now, was = ns.audio(audioFreq, strict, chunkSize=chunk), before(audioFreq, strict, chunk)
        assert now.sampRate == was.sampRate and now.length == was.length
        assert np.array_equal(now.signal, was.signal), (audioFreq, strict, chunk)


def test_wav_sink_fetches_a_device_resident_audio_once(dd, tmp_path, monkeypatch):
    """sink.wavFile on getAudio as it comes: the samples live on the device, one download serves this and every later write"""
    import scipy.io.wavfile
    from directdemod_amd import sink
    dfm, source, hip = dd
    fs, offset, bw, audioFreq = _fm.told("c")
    audio = dfm.decode_fm(source.IQarray(_fm.case("c"), fs), offset, bw, audioFreq, chunkSize=_fm.CHUNK).getAudio
    assert isinstance(audio.device_signal, hip.DevArray) and audio._host is None
    calls = []
    to_host = hip.DevArray.to_host
    monkeypatch.setattr(hip.DevArray, "to_host", lambda self, *a, **k: (calls.append(self.n), to_host(self, *a, **k))[1])
    p = str(tmp_path / "audio.wav")
    w = sink.wavFile(p, audio)
    assert w.write is w and calls == [audio.length]
    assert w.write is w and len(calls) == 1
    rate, back = scipy.io.wavfile.read(p)
    assert rate == audio.sampRate == 15000 and back.dtype == np.float64
    assert np.array_equal(back, audio.signal) and np.array_equal(back, _run(dd, "c")[1].signal)
