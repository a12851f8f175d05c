"""The FM stereo chain's NumPy restatement (directdemod_amd/fmstereo.py) on the CPU: what it separates, what
it reports about the pilot, its de-emphasis, its bit budget, the options and the formats.  The device is held to this restatement
bit for bit in test_gpu_fmstereo.py."""
import numpy as np
import pytest

import _fmstereo as T
import _rds
from directdemod_amd import decode_fmstereo, decode_rds, fmstereo as F, rds, sink


def decode(x, rate, **kw):
    kw.setdefault("deemphasis", None)
    out, info, lock = decode_fmstereo.decode_audio_host(x, rate, **kw)
    return out, info, lock, rate / F.params(rate)[0]


# ---------------------------------------------------------------------------------------------------------------- separation
@pytest.mark.parametrize("rate", [240000.0, 250000.0])
@pytest.mark.parametrize("clock_ppm", [0.0, -100.0])
@pytest.mark.parametrize("freq", [1000.0, 8000.0])
def test_a_tone_in_one_channel_stays_there(rate, clock_ppm, freq):
    seen = freq / (1.0 + clock_ppm * 1e-6)                               # the tone as the receiver's clock sees it
    for channel in (0, 1):
        out, info, lock, arate = decode(T.tone_multiplex(rate, freq, clock_ppm, channel), rate)
        sep = T.separation_db(out, seen, arate, channel)
        print("rate %g clock %+g ppm %g Hz channel %d: %.1f dB" % (rate, clock_ppm, freq, channel, sep))
        assert lock.all() and F.is_stereo(info) == 1
        assert sep >= 60.0
        level = T.levels(out, seen, arate)[channel] * F.audio_scale(rate)
        assert abs(level - 0.9 * T.TONE_LEVEL) < 0.005                   # the synthesiser's level of 0.9 times the tone's 0.8


@pytest.mark.parametrize("fs,offset", [(1200000, 0.0), (2400000, 300000.0)])
def test_a_tone_through_the_front_end(fs, offset):
    """the float64 restatement of the front end takes some 15 % from the 38 kHz band; the default difference gain makes up for it"""
    raw = T.tone_recording(fs, offset)
    mpx, rate = rds.audio_host(raw, fs, offset, decode_fmstereo.BW)
    arate = rate / F.params(rate)[0]
    out, info, _ = decode_fmstereo.decode_host(raw, fs, offset, deemphasis=None)
    plain, _, _ = decode_fmstereo.decode_host(raw, fs, offset, deemphasis=None, diffGain=1.0)
    sep, sep_plain = T.separation_db(out, 1000.0, arate), T.separation_db(plain, 1000.0, arate)
    print("fs %d offset %g: gain %.4f, %.1f dB, with a gain of 1 %.1f dB" % (fs, offset, F.diff_gain(fs, rate), sep, sep_plain))
    assert F.is_stereo(info) == 1 and 1.0 < F.diff_gain(fs, rate) < 1.5
    assert sep >= 36.0
    assert sep_plain < sep


# ---------------------------------------------------------------------------------------------------------------- the pilot
@pytest.mark.parametrize("sigma", [0.0, 0.02])
def test_without_a_pilot_every_block_is_mono(sigma):
    rate = 240000.0
    n = int(0.1 * rate)
    x = F.encode_mpx(F.tone(1000.0, 0.8, n, rate), F.tone(3000.0, 0.5, n, rate), rate, pilot=0.0, sigma=sigma, seed=1)
    out, info, lock, _ = decode(x, rate)
    assert info["blocks"] == n // F.B and info["locked"] == 0 and not lock.any() and F.is_stereo(info) == 0
    assert info["level"] <= 0.01
    assert np.array_equal(out[:, 0], out[:, 1]) and np.abs(out).max() > 0


def test_pilot_level_and_frequency():
    rate = 240000.0
    _, info, _, _ = decode(T.tone_multiplex(rate, 1000.0, 0.0, 0), rate)
    assert 0.08 <= info["level"] <= 0.095 and abs(info["freqError"]) < 0.3
    _, fast, _, _ = decode(T.tone_multiplex(rate, 1000.0, 100.0, 0), rate)
    print("level %.4f, %.3f Hz at +100 ppm" % (fast["level"], fast["freqError"]))
    assert 0.08 <= fast["level"] <= 0.095
    assert abs(fast["freqError"] - (-1.9)) < 0.3                         # 19 kHz * 1e-4 low for a clock 100 ppm fast


def test_a_short_multiplex_has_no_block():
    rate = 240000.0
    out, info, lock, _ = decode(T.tone_multiplex(rate, 1000.0)[:F.B - 1], rate)
    assert info == {"blocks": 0, "locked": 0, "level": 0.0, "freqError": 0.0} and len(lock) == 0
    assert out.shape == ((F.B - 1 + 4) // 5, 2) and np.array_equal(out[:, 0], out[:, 1])
    out, info, _, _ = decode(np.zeros(0), rate)
    assert out.shape == (0, 2) and info["blocks"] == 0


# ---------------------------------------------------------------------------------------------------------------- de-emphasis
@pytest.mark.parametrize("tau", [50e-6, 75e-6, None])
def test_deemphasis(tau):
    rate = 240000.0
    n = int(0.1 * rate)
    amp = {}
    for freq in (1000.0, 10000.0):
        t = F.tone(freq, 0.5, n, rate)
        out, _, _, arate = decode(F.encode_mpx(t, t, rate), rate, deemphasis=tau)
        amp[freq] = T.levels(out, freq, arate)[0]
    ratio = amp[10000.0] / amp[1000.0]
    if tau is None:
        assert abs(ratio - 1.0) < 0.01
    else:
        want = np.sqrt(1.0 + (2.0 * np.pi * 1e3 * tau) ** 2) / np.sqrt(1.0 + (2.0 * np.pi * 1e4 * tau) ** 2)
        print("tau %g: %.4f against %.4f" % (tau, ratio, want))
        assert abs(ratio / want - 1.0) < 0.05


def test_preemphasis_undoes_deemphasis():
    rate = 240000.0
    n = int(0.1 * rate)
    t = F.tone(10000.0, 0.2, n, rate)
    out, _, _, arate = decode(F.encode_mpx(t, t, rate, preemphasis=50e-6), rate, deemphasis=50e-6)
    assert abs(T.levels(out, 10000.0, arate)[0] * F.audio_scale(rate) / (0.9 * 0.2) - 1.0) < 0.01


# ---------------------------------------------------------------------------------------------------------------- the bit budget
@pytest.mark.parametrize("rate,tau", [(240000.0, 50e-6), (500000.0, 75e-6), (125000.0, None)])
def test_full_scale_stays_inside_the_budget(rate, tau):
    D, _, step38 = F.params(rate)
    h, d0 = F.taps(rate, tau)
    n = 3 * F.B * D + len(h)
    o = (n // D) // 2
    assert len(h) <= F.TAPS_MAX and int(np.abs(h.astype(np.int64)).sum()) <= F.TAPS_SUM_MAX
    for channel in (0, 1):
        x, u, G = T.full_scale(rate, tau, o, n, channel)
        ab = F.mix_host(x, step38, u, G)
        assert 1 << 23 <= np.abs(ab).max() <= F.AB_MAX                  # the mixer reaches its bound and fits 32 bits
        sums = (np.convolve(ab[:, channel], h.astype(np.int64))[d0::D])[:(n + D - 1) // D]
        assert np.abs(sums).max() < 1 << 41 and abs(int(sums[o])) == int((np.abs(ab[:, channel])[o * D + d0 - np.arange(len(h))] * np.abs(h)).sum())
        out = F.fir_host(ab, h, D, d0)
        assert np.array_equal(out[:, channel], sums >> F.OUT_SHIFT)
        assert (1 << 22) < np.abs(out).max() < F.OUT_MAX
        assert np.array_equal(F.audio_host(x, step38, u, G, h, D, d0).astype(np.int64), out)      # nothing wraps in 32 bits


def test_carrier_budget_and_floor_division():
    P = np.array([[1 << 27, -(1 << 27)]] * 40 + [[-(1 << 27), 1 << 27]] * 3, np.int64)
    S, u, lock = F.carrier_host(P, 1 << 38)                              # (|S| / cnt)^2 is 2^39 where all 17 blocks agree
    assert np.abs(S).max() == 17 << 19 and not lock.all() and lock.any()
    assert np.abs(u).max() <= 1 << F.Q
    S, u, lock = F.carrier_host([[256 * 3, 256 * 4]], 25)
    assert S.tolist() == [[3, 4]] and lock.tolist() == [1]
    assert u.tolist() == [[(-((9 - 16) << 14)) // 25, (-((24) << 14)) // 25]] == [[4587, -15729]]
    assert F.carrier_host([[256 * 3, 256 * 4]], 26)[2].tolist() == [0]
    assert F.carrier_host([[0, 0]], 0)[2].tolist() == [0]


# ---------------------------------------------------------------------------------------------------------------- options and formats
def test_options():
    rate = 240000.0
    x = np.zeros(1000)
    for kw in ({"deemphasis": 60e-6}, {"pilotMin": 0.0}, {"pilotMin": 0.6}, {"diffGain": 1.6}, {"diffGain": 0.1}):
        with pytest.raises(ValueError, match="fmstereo"):
            decode_fmstereo.decode_audio_host(x, rate, **kw)
        with pytest.raises(ValueError, match="decode_fmstereo"):
            decode_fmstereo.decode_fmstereo.fromAudio(x, rate, **kw)
    for bad in (100000.0, 600000.0, 0, None):
        with pytest.raises(ValueError, match="decode_fmstereo"):
            decode_fmstereo.decode_fmstereo.fromAudio(x, bad)

    class Src:
        sampFreq = 1200000
    with pytest.raises(ValueError, match="decode_fmstereo"):
        decode_fmstereo.decode_fmstereo(Src(), 0.0, bw=2000000)
    with pytest.raises(ValueError, match="decode_fmstereo"):
        decode_fmstereo.decode_fmstereo(Src(), 0.0, bw=100000)
    assert [F.params(r)[0] for r in (125000.0, 171000.0, 240000.0, 250000.0, 384000.0, 500000.0)] == [3, 4, 5, 5, 8, 10]
    assert F.params(240000.0)[2] == 2 * F.params(240000.0)[1]
    for r in (125000.0, 240000.0, 500000.0):
        for tau in F.DEEMPHASIS:
            h, d0 = F.taps(r, tau)
            assert len(h) <= F.TAPS_MAX and abs(int(h.sum()) - 32768) < 64 and (tau is not None or h[d0] == h.max())


def test_formats_and_a_stereo_wav(tmp_path):
    from scipy.io import wavfile
    rate = 240000.0
    out, _, _, arate = decode(T.tone_multiplex(rate, 1000.0), rate)
    audio, pcm = F.to_float(out, rate), F.to_pcm(out, rate)
    assert audio.dtype == np.float32 and pcm.dtype == np.int16 and audio.shape == pcm.shape == out.shape
    assert np.array_equal(audio, (out * F.audio_scale(rate)).astype(np.float32))
    assert 0.70 < np.abs(audio[:, 0]).max() < 0.74 and np.abs(audio[1000:-1000, 1]).max() < 0.005            # (the ends: the filter runs in)
    assert np.array_equal(F.to_pcm(np.array([[1 << 26, -(1 << 26)]]), rate), [[32767, -32768]])
    path = str(tmp_path / "stereo.wav")
    sink.wavFile(path, F.StereoSignal(arate, pcm)).write
    got_rate, got = wavfile.read(path)
    assert got_rate == 48000 and got.shape == pcm.shape and np.array_equal(got, pcm)


def test_rds_from_the_same_multiplex():
    """the multiplex that gives left and right also carries the station's groups"""
    rate = 240000.0
    bits = np.concatenate((np.zeros(24, np.uint8), rds.air_bits(_rds.station_groups())))      # some 20 ms of lead
    n = rds.stream_length(len(bits) // rds.BITS + 1, rate)
    x = F.encode_mpx(F.tone(1000.0, 0.5, n, rate), np.zeros(n), rate, rds_bits=bits)
    out, info, _, arate = decode(x, rate)
    assert F.is_stereo(info) == 1 and T.separation_db(out, 1000.0, arate) >= 60.0
    groups, _ = decode_rds.decode_audio_host(x, rate)
    _rds.same_station(decode_rds.stations_host(groups)[_rds.PI])
