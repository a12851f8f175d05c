"""The FM stereo kernels on the device (dd_fmstereo.h through dd_fms_pilot, dd_fms_carrier, dd_fms_audio and the diagnostics
dd_debug_fms_mix and dd_debug_fms_audio_route, the wrappers of directdemod_amd/fmstereo.py and decode_fmstereo) against the NumPy
restatement in fmstereo.py.

Everything behind the quantiser is integer, so every comparison of the kernels is exact equality; only the
end-to-end test, whose float32 front end rounds differently from the float64 restatement, compares separations."""
import numpy as np
import pytest

import _fmstereo as T
import _rds
from directdemod_amd import decode_fmstereo, decode_rds, fmstereo as F, rds, source

pytestmark = pytest.mark.gpu

SENT32 = np.int32(-0x5A5A5A5B)
SENT8 = np.uint8(0xA5)
SPARE = 16
RATES = [171000.0, 240000.0, 250000.0, 384000.0]
B = F.B


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def dev_f64(hip, x):
    return hip.DevArray.from_host(np.ascontiguousarray(x if len(x) else np.zeros(1), dtype=np.float64))


def dev_i32(hip, a):
    a = np.ascontiguousarray(a, dtype=np.int32).ravel()
    return hip.DevArray.from_host(a if len(a) else np.zeros(2, np.int32))


def rough_multiplex(n, seed):
    """noise at a third of full scale with a NaN, infinities, +-pi exactly, values just inside and beyond the clip"""
    x = np.random.default_rng(seed).normal(0.0, 1.0, n)
    special = [np.nan, np.inf, -np.inf, np.pi, -np.pi, np.nextafter(np.pi, 4.0), 3.2, -3.2, 1e300, 0.0, -0.0]
    for k, v in enumerate(special):
        if 7 * k + 3 < n:
            x[7 * k + 3] = v
    return x


# ---------------------------------------------------------------------------------------------------------------- pilot blocks
def dev_pilot(hip, x, step19):
    """dd_fms_pilot with sentinels behind its output -> int32[n // 256, 2]"""
    nb = len(x) // B
    out, xd = hip.DevArray.from_host(np.full(2 * nb + SPARE, SENT32, np.int32)), dev_f64(hip, x)
    rc = hip.lib().dd_fms_pilot(xd.ptr, len(x), step19, rds.table_device().ptr, out.ptr, None)
    hip.sync()
    got = out.to_host()
    assert rc == 0 and np.all(got[2 * nb:] == SENT32)
    return got[:2 * nb].reshape(nb, 2)


@pytest.mark.parametrize("rate", RATES)
def test_pilot(hip, rate):
    step19 = F.params(rate)[1]
    for n in (0, 1, B - 1, B, B + 1, 2 * B - 1, 17 * B + 5):
        x = rough_multiplex(n, n + int(rate))
        want = F.pilot_host(x, step19)
        got = dev_pilot(hip, x, step19)
        assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want), n


def test_pilot_at_full_scale(hip):
    """every sample at +-pi with the sign of the phasor's component: |P| reaches its bound's neighbourhood and nothing wraps"""
    step19 = F.params(240000.0)[1]
    n = 5 * B + 9
    for comp in (0, 1):
        x = np.where(rds.table()[rds.phases(0, n, step19), comp] >= 0, np.pi, -np.pi)
        want = F.pilot_host(x, step19)
        assert (1 << 26) < np.abs(want[:, comp]).min() and np.abs(want).max() <= 1 << 27
        assert np.array_equal(dev_pilot(hip, x, step19).astype(np.int64), want)


# ---------------------------------------------------------------------------------------------------------------- carrier
def dev_carrier(hip, P, thr):
    """dd_fms_carrier with sentinels behind its three outputs -> (S, u, lock)"""
    P = np.asarray(P, dtype=np.int32).reshape(-1, 2)
    nb = len(P)
    S, u = (hip.DevArray.from_host(np.full(2 * nb + SPARE, SENT32, np.int32)) for _ in range(2))
    lock = hip.DevArray.from_host(np.full(nb + SPARE, SENT8, np.uint8))
    Pd = dev_i32(hip, P)
    rc = hip.lib().dd_fms_carrier(Pd.ptr, nb, int(thr), S.ptr, u.ptr, lock.ptr, None)
    hip.sync()
    S, u, lock = S.to_host(), u.to_host(), lock.to_host()
    assert rc == 0 and np.all(S[2 * nb:] == SENT32) and np.all(u[2 * nb:] == SENT32) and np.all(lock[nb:] == SENT8)
    return S[:2 * nb].reshape(nb, 2), u[:2 * nb].reshape(nb, 2), lock[:nb]


def check_carrier(hip, P, thr):
    want = F.carrier_host(P, thr)
    got = dev_carrier(hip, P, thr)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g.astype(np.int64), w.astype(np.int64))
    return want


@pytest.mark.parametrize("nb", [0, 1, 2, F.W, F.W + 1, 2 * F.W, 2 * F.W + 1, 2 * F.W + 2, 100])
def test_carrier_sizes(hip, nb):
    rng = np.random.default_rng(nb)
    P = rng.integers(-(1 << 27), (1 << 27) + 1, (nb, 2))
    for thr in (0, 1 << 30, 1 << 36, F.THR_MAX):
        check_carrier(hip, P, thr)
    check_carrier(hip, np.where(P >= 0, 1 << 27, -(1 << 27)), 1 << 38)      # every component at its bound


def test_carrier_at_the_threshold(hip):
    """blocks whose |S|^2 is exactly thr cnt^2 lock, one below does not; S = 0 never locks"""
    one = np.array([[256 * 3, 256 * 4]])                                  # S = (3, 4), cnt = 1: |S|^2 = 25
    assert check_carrier(hip, one, 25)[2].tolist() == [1] and check_carrier(hip, one, 26)[2].tolist() == [0]
    P = np.tile(np.array([[256 * 300, -256 * 400]]), (40, 1))             # S = cnt (300, -400): |S|^2 = 250000 cnt^2 in every block
    S, u, lock = check_carrier(hip, P, 250000)
    assert lock.all() and len(set(map(tuple, u.tolist()))) == 1
    assert not check_carrier(hip, P, 250001)[2].any()
    zero = np.zeros((20, 2), np.int64)
    for thr in (0, 1):
        S, u, lock = check_carrier(hip, zero, thr)
        assert not lock.any() and not u.any()
    P[7] = (-256 * 300 * 16, 256 * 400 * 16)                              # the blocks whose sums cancel around block 7 give S = 0
    S, u, lock = check_carrier(hip, P, 0)
    assert (np.abs(S).sum(axis=1) == 0).any() and not lock[np.abs(S).sum(axis=1) == 0].any()


# ---------------------------------------------------------------------------------------------------------------- mixer and filter
def lock_patterns(nb, seed):
    """u of nb blocks: all unlocked; alternating locked (unit phasors in Q14 as the carrier stage gives them) and unlocked"""
    ang = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, nb)
    unit = np.stack((np.floor(16384.0 * np.cos(ang)), np.floor(16384.0 * np.sin(ang))), axis=1).astype(np.int64)
    alt = unit.copy()
    alt[1::2] = 0
    return [np.zeros((nb, 2), np.int64), alt, unit]


def dev_audio(hip, x, step38, u, G, h, D, d0, route=None):
    """dd_fms_audio (or the route diagnostic) with sentinels behind its output -> int32[ceil(n / D), 2]"""
    nout = (len(x) + D - 1) // D
    out = hip.DevArray.from_host(np.full(2 * nout + SPARE, SENT32, np.int32))
    hd, xd, ud = dev_i32(hip, h), dev_f64(hip, x), dev_i32(hip, u)            # (held until the call has run)
    args = (xd.ptr, len(x), step38, rds.table_device().ptr, ud.ptr, len(u), G, hd.ptr, len(h), D, d0)
    if route is None:
        rc = hip.lib().dd_fms_audio(*args, out.ptr, None)
    else:
        rc = hip.lib().dd_debug_fms_audio_route(*args, route, out.ptr, None)
    hip.sync()
    got = out.to_host()
    assert rc == 0 and np.all(got[2 * nout:] == SENT32)
    return got[:2 * nout].reshape(nout, 2)


def dev_mix(hip, x, step38, u, G):
    n = len(x)
    out, xd, ud = hip.DevArray.from_host(np.full(2 * n + SPARE, SENT32, np.int32)), dev_f64(hip, x), dev_i32(hip, u)
    rc = hip.lib().dd_debug_fms_mix(xd.ptr, n, step38, rds.table_device().ptr, ud.ptr, len(u), G, out.ptr, None)
    hip.sync()
    got = out.to_host()
    assert rc == 0 and np.all(got[2 * n:] == SENT32)
    return got[:2 * n].reshape(n, 2)


@pytest.mark.parametrize("rate", RATES)
def test_mix(hip, rate):
    _, _, step38 = F.params(rate)
    for n in (0, 1, B - 1, B, B + 1, 3 * B + 7):
        x = rough_multiplex(n, n + int(rate))
        for u in lock_patterns(n // B, n):
            for g in (1.0, 1.5):
                want = F.mix_host(x, step38, u, F.gain_word(g))
                assert np.abs(want).max(initial=0) <= F.AB_MAX
                assert np.array_equal(dev_mix(hip, x, step38, u, F.gain_word(g)).astype(np.int64), want)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("tau", [None, 75e-6])
def test_audio(hip, rate, tau):
    """tau None gives the shortest taps of a rate, 75 us the longest; both arithmetic routes give the restatement's bits"""
    D, _, step38 = F.params(rate)
    h, d0 = F.taps(rate, tau)
    tile = D * 256
    assert D == {171000.0: 4, 240000.0: 5, 250000.0: 5, 384000.0: 8}[rate]
    for k, n in enumerate((0, 1, B - 1, B, B + 1, tile - 1, tile, tile + 1, 2 * tile + len(h) + 3)):
        x = rough_multiplex(n, n + int(rate))
        u = lock_patterns(n // B, n)[k % 3]
        G = F.gain_word((1.0, 1.5)[k % 2])
        want = F.audio_host(x, step38, u, G, h, D, d0)
        for route in (None, 0, 1):
            got = dev_audio(hip, x, step38, u, G, h, D, d0, route)
            assert got.shape == want.shape and np.array_equal(got, want), (n, route)


@pytest.mark.parametrize("ntaps", [1, 2, 1023, 1024])
def test_audio_at_the_taps_limits(hip, ntaps):
    """one tap, and the 1024 the entry allows, with every lock pattern and both gains"""
    rate = 240000.0
    D, _, step38 = F.params(rate)
    rng = np.random.default_rng(ntaps)
    h = rng.integers(-127, 128, ntaps).astype(np.int32)                  # the sum of |h| stays below 2^17
    n = 2 * D * 256 + ntaps + 3
    x = rough_multiplex(n, ntaps)
    for d0 in sorted({0, ntaps // 2, ntaps - 1}):
        for u in lock_patterns(n // B, ntaps):
            for g in (1.0, 1.5):
                want = F.audio_host(x, step38, u, F.gain_word(g), h, D, d0)
                assert np.array_equal(dev_audio(hip, x, step38, u, F.gain_word(g), h, D, d0), want), (d0, g)
    assert np.array_equal(dev_audio(hip, x, step38, np.zeros((0, 2)), 8192, h, D, 0), F.audio_host(x, step38, np.zeros((0, 2)), 8192, h, D, 0))


@pytest.mark.parametrize("rate,tau", [(240000.0, 50e-6), (500000.0, 75e-6), (125000.0, None)])
def test_audio_at_full_scale(hip, rate, tau):
    """the full-scale case of test_fmstereo_host.py: the largest |a|, |b| and the largest sum, by both routes"""
    D, _, step38 = F.params(rate)
    h, d0 = F.taps(rate, tau)
    n = 3 * B * D + len(h)
    o = (n // D) // 2
    for channel in (0, 1):
        x, u, G = T.full_scale(rate, tau, o, n, channel)
        want = F.audio_host(x, step38, u, G, h, D, d0)
        assert np.abs(want.astype(np.int64)).max() > 1 << 22
        assert np.array_equal(dev_mix(hip, x, step38, u, G).astype(np.int64), F.mix_host(x, step38, u, G))
        for route in (None, 0, 1):
            assert np.array_equal(dev_audio(hip, x, step38, u, G, h, D, d0, route), want), route


def test_entries_refuse_what_they_do_not_serve(hip):
    lib, t = hip.lib(), rds.table_device().ptr
    x, u, h, out = dev_f64(hip, np.zeros(600)), dev_i32(hip, np.zeros(4)), dev_i32(hip, np.ones(8)), dev_i32(hip, np.zeros(2000))
    ok = (x.ptr, 600, 1, t, u.ptr, 2, 8192, h.ptr, 8, 5, 3)
    assert lib.dd_fms_audio(*ok, out.ptr, None) == 0
    for pos, bad in ((1, -1), (2, 1 << 32), (5, -1), (6, F.G_MAX + 1), (6, -1), (8, 0), (8, F.TAPS_MAX + 1), (9, 0), (9, F.D_MAX + 1),
                     (10, -1), (10, 8)):
        args = list(ok)
        args[pos] = bad
        assert lib.dd_fms_audio(*args, out.ptr, None) == hip.DD_ERR_INVALID, (pos, bad)
    assert lib.dd_debug_fms_audio_route(*ok, 2, out.ptr, None) == hip.DD_ERR_INVALID
    assert lib.dd_fms_carrier(u.ptr, 2, -1, out.ptr, out.ptr, out.ptr, None) == hip.DD_ERR_INVALID
    assert lib.dd_fms_carrier(u.ptr, 2, F.THR_MAX + 1, out.ptr, out.ptr, out.ptr, None) == hip.DD_ERR_INVALID
    assert lib.dd_fms_pilot(x.ptr, -1, 1, t, out.ptr, None) == hip.DD_ERR_INVALID
    hip.sync()


# ---------------------------------------------------------------------------------------------------------------- the decoder
def same_outputs(obj, want_out, want_info, want_lock, rate):
    assert np.array_equal(obj.getSamples, want_out) and obj.pilotInfo == want_info and np.array_equal(obj.lockInfo, want_lock)
    assert np.array_equal(obj.getAudio, F.to_float(want_out, rate)) and np.array_equal(obj.getPCM, F.to_pcm(want_out, rate))
    assert obj.stereo == F.is_stereo(want_info) and obj.useful == (1 if len(want_out) else 0)
    st = obj.getStereo
    arate = rate / F.params(rate)[0]
    assert st.sampRate == int(round(arate)) and np.array_equal(st.signal, F.to_pcm(want_out, rate))
    audio = F.to_float(want_out, rate).astype(np.float64)
    for sig, want in ((obj.getLeft, audio[:, 0]), (obj.getRight, audio[:, 1]), (obj.getMono, 0.5 * (audio[:, 0] + audio[:, 1]))):
        assert sig.sampRate == int(round(arate)) and np.array_equal(np.asarray(sig.signal, dtype=np.float64), want)
    assert obj.audioRate == arate and obj.multiplexRate == rate


@pytest.mark.parametrize("rate,kw", [(240000.0, {}), (250000.0, {"deemphasis": 75e-6, "diffGain": 1.25}),
                                     (171000.0, {"deemphasis": None, "pilotMin": 0.2})])
def test_from_audio_against_the_restatement(hip, rate, kw):
    x = T.tone_multiplex(rate, 1000.0, -100.0, 0, 0.05)
    obj = decode_fmstereo.decode_fmstereo.fromAudio(x, rate, **kw)
    want_out, want_info, want_lock = decode_fmstereo.decode_audio_host(x, rate, **kw)
    same_outputs(obj, want_out, want_info, want_lock, rate)
    assert obj.stereo == (0 if "pilotMin" in kw else 1) and set(obj.timings) >= {"pilot", "carrier", "audio", "download", "host"}
    short = decode_fmstereo.decode_fmstereo.fromAudio(x[:B - 1], rate, **kw)
    same_outputs(short, *decode_fmstereo.decode_audio_host(x[:B - 1], rate, **kw), rate)
    assert short.stereo == 0 and np.array_equal(short.getSamples[:, 0], short.getSamples[:, 1])


def test_rds_from_the_decoder_s_multiplex(hip):
    """decode_rds.fromAudio over decode_fmstereo's device multiplex: one front-end pass serves both"""
    rate = 240000.0
    bits = np.concatenate((np.zeros(24, np.uint8), rds.air_bits(_rds.station_groups())))
    n = rds.stream_length(len(bits) // rds.BITS + 1, rate)
    x = F.encode_mpx(F.tone(1000.0, 0.5, n, rate), np.zeros(n), rate, rds_bits=bits)
    obj = decode_fmstereo.decode_fmstereo.fromAudio(x, rate)
    assert obj.stereo == 1 and T.separation_db(obj.getSamples, 1000.0, obj.audioRate) >= 60.0
    r = decode_rds.decode_rds.fromAudio(obj.multiplex(), obj.multiplexRate)
    _rds.same_station(r.getStations[_rds.PI])
    assert r.getGroups == decode_rds.decode_audio_host(x, rate)[0]


def test_end_to_end_through_the_front_end(hip):
    """one 0.2 s recording at 1.2 MS/s through the real float32 front end.  Its stages round differently from the float64
    restatement, so bits cannot match; the crosstalk that remains comes from the front end's frequency response, which is systematic
    and the same on both paths, while rounding noise near 2e-7 rad lies far below it: the device's separation may fall short of the
    host restatement's on the same recording by 6 dB at the most."""
    raw = np.asarray(T.tone_recording())
    obj = decode_fmstereo.decode_fmstereo(source.IQarray(np.array(raw), T.FS), T.CHANNEL, deemphasis=None)
    host_out, host_info, _ = decode_fmstereo.decode_host(raw, T.FS, T.CHANNEL, deemphasis=None)
    arate = obj.audioRate
    dev_sep, host_sep = T.separation_db(obj.getSamples, 1000.0, arate), T.separation_db(host_out, 1000.0, arate)
    info = obj.pilotInfo
    print("device separation %.1f dB, host restatement %.1f dB; pilot level %.4f, freqError %.3f Hz (host %.3f)"
          % (dev_sep, host_sep, info["level"], info["freqError"], host_info["freqError"]))
    assert obj.stereo == 1 and obj.multiplexRate == 240000.0 and abs(len(obj.getSamples) - len(host_out)) <= 1
    assert abs(info["freqError"] - host_info["freqError"]) < 0.3
    assert dev_sep >= host_sep - 6.0
    assert abs(obj.diffGain - F.diff_gain(T.FS, 240000.0)) < 1e-12
