"""AFSK1200 frame logic on the device (dd_peakdetect_f64, dd_afsk_bits_f64, dd_afsk_frames_check / _pack) and decode_afsk1200 end to
end, against the reference's own getMsg runs (tests/golden/afsk_frames_*.npz) and the host restatements in tests/_ax25.py."""
import os

import numpy as np
import pytest

import _ax25

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPB = 22050 // 1200


@pytest.fixture(scope="module")
def dd():
    from directdemod_amd import _hip
    _hip.require_gpu()
    import directdemod_amd as pkg
    from directdemod_amd import afsk, decode_afsk1200, peakdetect, source
    return pkg, afsk, decode_afsk1200, peakdetect, source


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def _pd(afsk, y, L, delta=0.0):
    (mp, mv), (np_, nv) = afsk.peak_lists(np.asarray(y, dtype=np.float64), L, delta)
    return list(zip(mp.to_host().tolist(), mv.to_host().tolist())), list(zip(np_.to_host().tolist(), nv.to_host().tolist()))


@pytest.mark.parametrize("name", ["afsk_frames_a.npz", "afsk_frames_b.npz"])
def test_peakdetect_on_the_reference_input(dd, name):
    _, afsk, _, peakdetect, _ = dd
    g = _load(name)
    y = np.abs(g["edge_sums"].astype(np.float64) / SPB)
    mx, mn = peakdetect.peakdetect(y, lookahead=int(g["pd_lookahead"]))
    assert [p[0] for p in mx] == g["pd_max_x"].tolist() and [p[1] for p in mx] == g["pd_max_y"].tolist()
    assert [p[0] for p in mn] == g["pd_min_x"].tolist() and [p[1] for p in mn] == g["pd_min_y"].tolist()
    xs = np.arange(len(y)) * 2.5                                   # an x axis maps positions on the host
    mx2, _ = peakdetect.peakdetect(y, xs, lookahead=int(g["pd_lookahead"]))
    assert [p[0] for p in mx2] == (g["pd_max_x"] * 2.5).tolist()


def _cases():
    rng = np.random.default_rng(5)
    out = [("ties", rng.integers(0, 4, 3000).astype(np.float64), 7, 0.0),
           ("ties_L1", rng.integers(0, 3, 2000).astype(np.float64), 1, 0.0),
           ("ties_delta", rng.integers(0, 6, 3000).astype(np.float64), 5, 1.0),
           ("noise_delta", rng.standard_normal(3000), 11, 0.3),
           ("flat", np.zeros(2000), 11, 0.0),
           ("up", np.arange(2000, dtype=np.float64), 11, 0.0),
           ("down", -np.arange(2000, dtype=np.float64), 3, 0.0),
           ("alternating", np.tile([0.0, 1.0], 1000), 1, 0.0),
           ("alternating_L2", np.tile([0.0, 1.0, 1.0], 700), 2, 0.0),
           ("short_eq_L", rng.standard_normal(11), 11, 0.0),
           ("short_lt_L", rng.standard_normal(5), 11, 0.0),
           ("one_past_L", rng.standard_normal(12), 11, 0.0),
           ("big_L", rng.standard_normal(3000), 300, 0.0),
           ("quantised", np.abs(np.round(rng.standard_normal(4000) * 4) / SPB), 11, 0.0)]
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_peakdetect_exact_vs_host_machine(dd, case):
    _, afsk, _, _, _ = dd
    _, y, L, delta = case
    assert _pd(afsk, y, L, delta) == _ax25.peakdetect_host(y, L, delta)


def test_peakdetect_long_flat_and_monotone(dd):
    """no quadratic work on plateaus and ramps: 2 M samples each, no confirmations"""
    _, afsk, _, _, _ = dd
    for y in (np.zeros(2000000), np.arange(2000000, dtype=np.float64)):
        assert _pd(afsk, y, 11) == ([], [])


def test_peakdetect_rejects_bad_arguments(dd):
    pkg, afsk, _, peakdetect, _ = dd
    with pytest.raises(ValueError):
        peakdetect.peakdetect([1.0, 2.0, 1.0], lookahead=0)
    with pytest.raises(ValueError):
        peakdetect.peakdetect([1.0, 2.0, 1.0], lookahead=1, delta=-1)
    with pytest.raises(ValueError):
        peakdetect.peakdetect([1.0, 2.0, 1.0], [0, 1], lookahead=1)
    with pytest.raises(ValueError, match="non-finite"):         # DD_ERR_INVALID
        afsk.peak_lists(np.array([0.0, 1.0, np.nan, 0.0, 2.0, 0.0]), 1)


@pytest.mark.parametrize("bw", [22050, 48000, 11025])
def test_bits_exact_vs_numpy(dd, bw):
    _, afsk, _, _, _ = dd
    rng = np.random.default_rng(bw)
    n = 60000
    bf = rng.standard_normal(n) * 1e3
    bf[rng.integers(0, n, 200)] = 0.0
    q = bw / 1200
    gaps = np.maximum(1, np.round(rng.uniform(0.3, 6.0, 4000) * q)).astype(np.int64)
    px = np.cumsum(gaps)
    px = px[px < n - 5]
    bs = afsk.bit_stream(bf, px, bw)
    means, bits, marks, flags = _ax25.bits_host(bf, px, bw)
    got = bs.mean.to_host()
    assert got.shape == means.shape and np.array_equal(got.view(np.int64), means.view(np.int64))
    assert np.array_equal(bs.sgn.to_host(), np.sign(means).astype(np.int8))
    assert np.array_equal(bs.bits.to_host(), bits) and np.array_equal(bs.marks.to_host(), marks)
    assert np.array_equal(bs.flags.to_host(), flags)


def test_bits_stuffing_and_flags_on_a_known_stream(dd):
    """means of +-1 slices give prescribed NRZI levels: the device's bits, marks and flags equal the host's"""
    _, afsk, _, _, _ = dd
    fb = _ax25.frame_bytes(("APRS", 0), ("N0CALL", 1), "\xff\xfe~~" * 10)
    bits = [0, 1, 1, 1, 1, 1, 1, 0] * 3 + _ax25.hdlc_bits(fb)
    lv = np.array(_ax25.nrzi(bits), dtype=np.float64) * 2 - 1
    bf = np.repeat(np.concatenate([[1.0], lv]), SPB)
    px = np.arange(0, len(bf) - SPB + 1, SPB)
    bs = afsk.bit_stream(bf, px, 22050)
    _, hb, hm, hf = _ax25.bits_host(bf, px, 22050)
    assert np.array_equal(bs.bits.to_host(), hb) and np.array_equal(bs.marks.to_host(), hm)
    assert np.array_equal(bs.flags.to_host(), hf) and (hm == 2).any() and (hm == 1).any()


def test_bit_signs_from_the_device_front_end(dd):
    """the reference's peaks over the device's own binary_filter of fixture (a): the signs equal the reference's wherever the mean
    is a decision (|mean| > 1e-3 of the largest)"""
    pkg, afsk, dmod, _, source = dd
    g = _load("afsk_frames_a.npz")
    raw, fs, offset, _ = _ax25.fixture_a()
    obj = dmod.decode_afsk1200(source.IQarray(raw, fs), offset, 22050)
    from directdemod_amd import comm, constants, filters
    sig = obj._audio()
    sig.filter(filters.butter(sig.sampRate, 700, 2700, typeFlt=constants.FLT_BP))
    bf = afsk.binary_filter(comm._convert(sig.device_signal, np.float64), 22050)
    bs = afsk.bit_stream(bf, g["pd_max_x"].astype(np.int64), 22050)
    m = bs.mean.to_host()
    ref = g["nrzi_sign"]
    assert m.shape == ref.shape
    strong = np.abs(m) > 1e-3 * np.max(np.abs(m))
    assert strong.mean() > 0.95 and np.array_equal(np.sign(m[strong]).astype(np.int8), ref[strong])


def _stream(parts):
    bits = []
    for p in parts:
        bits += list(p)
    return bits


def test_frames_vs_host(dd):
    """back-to-back flags, len % 8 != 0, 128- and 136-bit messages, a bad CRC, a marked 2, a pair spanning 20 000 noise bits"""
    _, afsk, _, _, _ = dd
    from directdemod_amd._hip import DevArray
    rng = np.random.default_rng(9)
    F = [0, 1, 1, 1, 1, 1, 1, 0]

    def body(nbytes, bad=False):
        b = bytes(rng.integers(0, 256, nbytes - 2).tolist())
        fcs = _ax25._crc16(b) ^ (1 if bad else 0)
        return _ax25.hdlc_bits(b + bytes([fcs & 0xFF, fcs >> 8]), 0)
    noise = rng.integers(0, 2, 20000)
    noise[::5] = 0                                                  # no run of six ones: no flag inside the long pair
    parts = [F, F, F, body(30), F, body(18), F, body(19), F, body(20, bad=True), F, body(25)[:-3], F,
             [1, 1, 1, 1, 1, 1, 1, 1], F, body(40), F, noise.tolist(), F, body(35), F, F]
    bits = np.array(_stream(parts), dtype=np.int8)
    from directdemod_amd.decode_afsk1200 import decode_afsk1200 as D
    marks = D.find_bit_stuffing(bits).astype(np.int8)
    flags = np.array([k for k in range(len(bits) - 8) if tuple(bits[k:k + 8]) == tuple(F)], dtype=np.int64)
    info, raws = _ax25.frames_host(bits, marks, flags)
    bs = afsk.BitStream(None, None, DevArray.from_host(bits), DevArray.from_host(marks), DevArray.from_host(flags))
    ginfo, graws = afsk.frames(bs)
    assert np.array_equal(ginfo, info) and graws == raws
    assert info[:, 1].sum() >= 4 and (info[:, 1] == 0).sum() >= 4 and info[:, 0].max() > 19000


def _check_frames(frames, g, fb):
    assert [f["flag"] for f in frames] == g["frame_flag"].tolist()
    # start bits: the same peaks give the same bits; a different f32 front end could shift them, bounded by one flag's length
    d = np.abs(np.array([f["start"] for f in frames]) - g["frame_start"])
    assert d.max(initial=0) <= 8
    offs = np.concatenate([[0], np.cumsum(g["frame_bits_len"])])
    for k, f in enumerate(frames):
        ref = g["frame_bits"][offs[k]:offs[k + 1]]
        want = bytes(int(sum(int(ref[i + j]) << j for j in range(8))) for i in range(0, len(ref), 8))
        assert f["raw"] == want
        out = str(g["stdout"])
        assert ("information:\t " + f["info"] + "\n") in out and ("destination:\t " + f["destination"] + "\n") in out
        assert ("source:\t\t " + f["source"] + "\n") in out and ("path:\t\t " + f["path"] + "\n") in out
        assert f["control"] == "0x3" and f["pid"] == "0xf0"
    sent = [b[:-2] for b in fb]
    assert all(f["raw"] in sent for f in frames)


def test_end_to_end_fixture_a(dd):
    pkg, afsk, dmod, _, source = dd
    g = _load("afsk_frames_a.npz")
    raw, fs, offset, fb = _ax25.fixture_a()
    obj = dmod.decode_afsk1200(source.IQarray(raw, fs), offset, None)
    assert obj.getMsg == str(g["msg"]) and obj.useful == int(g["useful"]) == 1
    fr = obj.getFrames
    _check_frames(fr, g, fb)
    assert len(fr) == 3 and fb[2][:-2] not in [f["raw"] for f in fr]             # the corrupted frame is rejected
    assert fr[0]["destination"] == "APRS  0" and fr[0]["source"] == "N0CALL7" and fr[0]["info"] == _ax25.INFO
    assert set(obj.timings) == {"front_end", "bandpass", "correlators", "peaks", "bits", "frames"}


class _HostOnly:
    """a source without read_device_raw"""

    def __init__(self, src):
        self._s = src
        self.sampFreq, self.length, self.sourceType = src.sampFreq, src.length, src.sourceType

    def read(self, a, b=None):
        return self._s.read(a, b)


@pytest.mark.parametrize("device_raw", [True, False])
def test_end_to_end_config1_wav(dd, tmp_path, device_raw):
    pkg, afsk, dmod, _, source = dd
    g = _load("afsk_frames_b.npz")
    raw, fs, offset, fb = _ax25.fixture_b()
    path = tmp_path / _ax25.C1_NAME
    _ax25.write_wav(str(path), raw, fs)
    src = source.IQwav(str(path))
    obj = dmod.decode_afsk1200(src if device_raw else _HostOnly(src), offset, 22050, use_device_raw=device_raw)
    assert obj.getMsg == str(g["msg"]) and obj.useful == 1
    _check_frames(obj.getFrames, g, fb)


def test_noise_only_recording(dd):
    pkg, afsk, dmod, _, source = dd
    rng = np.random.default_rng(4)
    raw = rng.integers(100, 156, (882000, 2)).astype(np.uint8)
    obj = dmod.decode_afsk1200(source.IQarray(raw, 882000), 0, 22050)
    assert obj.getMsg is None and obj.useful == 0 and obj.getFrames == []
