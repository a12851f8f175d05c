"""The AIS kernels on the device (dd_ais.h through dd_ais_candidates and dd_ais_demod, the wrappers of directdemod_amd/ais.py and
decode_ais) against the NumPy restatement in ais.py.

Everything behind the quantiser is integer, so every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import _ais as A
from directdemod_amd import ais, decode_ais, source

pytestmark = pytest.mark.gpu

SENT = np.int64(-0x5A5A5A5A5A5A5A5B)
SPARE = 16
SPS = [4.0, 5.0, 2048000 / 42 / 9600.0, 16.0]


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def w_of(sps):
    return ais.params(sps * ais.BAUD)[1]


def dev_candidates(hip, audio, sps, w, slack, cap):
    """dd_ais_candidates with `cap` places and SPARE sentinels behind them -> (rc, count, the places, the sentinels still whole)"""
    x = hip.DevArray.from_host(np.ascontiguousarray(audio, dtype=np.float64))
    lst = hip.DevArray.from_host(np.full(cap + SPARE, SENT))
    count = C.c_int64(-1)
    rc = hip.lib().dd_ais_candidates(x.ptr, len(audio), float(sps), int(w), int(slack), lst.ptr, cap, C.byref(count), None)
    hip.sync()
    got = lst.to_host()
    return rc, count.value, got[:cap], bool(np.all(got[cap:] == SENT))


def check_candidates(hip, audio, sps, w=None, slack=0):
    w = w_of(sps) if w is None else w
    want = ais.candidates_host(audio, sps, w, slack)
    rc, count, got, whole = dev_candidates(hip, audio, sps, w, slack, len(want) + 3)
    assert rc == 0 and count == len(want) and whole
    assert np.array_equal(got[:count], want) and np.all(got[count:] == SENT)
    return want


def dev_demod(hip, audio, sps, w, ts):
    """dd_ais_demod with sentinels behind every output -> the dict of ais.demod_host"""
    m = len(ts)
    x = hip.DevArray.from_host(np.ascontiguousarray(audio, dtype=np.float64))
    lst = hip.DevArray.from_host(np.ascontiguousarray(ts, dtype=np.int64))
    frames = hip.DevArray.from_host(np.full(ais.FRAME_BYTES * m + SPARE, 0xA5, np.uint8))
    meta = hip.DevArray.from_host(np.full(4 * m + SPARE, -0x5A5A5A5B, np.int32))
    score = hip.DevArray.from_host(np.full(m + SPARE, SENT))
    rc = hip.lib().dd_ais_demod(x.ptr, len(audio), float(sps), int(w), lst.ptr, m, frames.ptr, meta.ptr, score.ptr, None)
    hip.sync()
    assert rc == 0
    f, mt, sc = frames.to_host(), meta.to_host(), score.to_host()
    assert np.all(f[ais.FRAME_BYTES * m:] == 0xA5) and np.all(mt[4 * m:] == -0x5A5A5A5B) and np.all(sc[m:] == SENT)
    mt = mt[:4 * m].reshape(m, 4)
    return {"t": np.asarray(ts, dtype=np.int64), "frames": f[:ais.FRAME_BYTES * m].reshape(m, ais.FRAME_BYTES), "status": mt[:, 0],
            "nbits": mt[:, 1], "rem": mt[:, 2], "polarity": mt[:, 3], "score": sc[:m]}


def check_demod(hip, audio, sps, ts, w=None):
    w = w_of(sps) if w is None else w
    got = dev_demod(hip, audio, sps, w, ts)
    want = ais.demod_host(audio, sps, w, ts)
    for key in ("t", "frames", "status", "nbits", "rem", "polarity", "score"):
        assert np.array_equal(got[key], want[key]), key
    return got


# ---------------------------------------------------------------------------------------------------------------- candidates
@pytest.mark.parametrize("sps", SPS)
@pytest.mark.parametrize("slack", [0, 2, 11])
def test_candidates_on_noise(hip, sps, slack):
    """seeded noise of 3000 samples; at the largest slack only a distance of exactly 12 from the template fails, so most starts are
    listed, across twelve tiles"""
    audio = np.random.default_rng(int(sps * 1000) + slack).uniform(-np.pi, np.pi, 3000)
    want = check_candidates(hip, audio, sps, slack=slack)
    if slack == 11:
        assert len(want) > 2000


@pytest.mark.parametrize("sps", SPS)
def test_zero_and_full_scale_audio(hip, sps):
    for fill in (0.0, np.pi, -np.pi):
        audio = np.full(3000, fill)
        assert len(check_candidates(hip, audio, sps)) == 0           # every comparison an equality: all -, nine places off
        want = check_candidates(hip, audio, sps, slack=9)
        assert len(want) == ais.n_starts(3000, sps, w_of(sps))       # and with nine allowed every start passes


@pytest.mark.parametrize("sps", [4, 5, 16])
def test_shortest_audio_and_a_template_on_the_last_sample(hip, sps):
    w = w_of(sps)
    full = ais.reach(float(sps), w)
    x = A.as_audio(A.rect(A.frame_raw(A.payloads()[0]), sps, t=0))
    assert ais.n_starts(full - 1, float(sps), w) == 0 and ais.n_starts(full, float(sps), w) == 1
    rc, count, got, whole = dev_candidates(hip, x[:full - 1], float(sps), w, 0, 4)
    assert (rc, count, whole) == (0, 0, True) and np.all(got == SENT)
    assert check_candidates(hip, x[:full], float(sps)).tolist() == [0]           # the burst at the very start is found
    for t in (1, 300, 1021):                                         # the template ends on the last sample
        y = A.as_audio(A.rect(A.frame_raw(A.payloads()[0]), sps, t=t, n=t + full))
        want = check_candidates(hip, y, float(sps))
        assert want[-1] == t == ais.n_starts(len(y), float(sps), w) - 1


@pytest.mark.parametrize("edge", [256, 1024])
def test_passes_around_tile_edges(hip, edge):
    for sps in (4, 5):
        msg = A.frame_raw(A.payloads()[6])
        for t in (edge - 1, edge, edge + 1):
            want = check_candidates(hip, A.as_audio(A.rect(msg, sps, t=t)), float(sps))
            assert t in want
    x = ais.encode_audio(A.payloads()[:1] * 3, 48000.0, [edge - 80 - 2.5, 3000.0, 6000.0], sigma=0.01, seed=edge)
    want = check_candidates(hip, x, 5.0)
    assert np.any(want < edge) and np.any((want >= edge) & (want < edge + 4))    # one burst's passes on both sides of the edge


def test_capacities(hip):
    x = ais.encode_audio(A.payloads()[:4] + A.payloads()[5:], 48000.0, 200.5 + 1500.0 * np.arange(7), sigma=0.02, seed=7)
    want = ais.candidates_host(x, 5.0, 3)
    m = len(want)
    assert m >= 14
    for cap in (0, 1, m - 1, m, m + 1, m + 5):
        rc, count, got, whole = dev_candidates(hip, x, 5.0, 3, 0, cap)
        assert count == m and whole
        assert rc == (0 if cap >= m else hip.DD_ERR_INVALID)
        kept = min(cap, m)
        assert np.array_equal(got[:kept], want[:kept]) and np.all(got[kept:] == SENT)
    lst, count = ais.candidates(hip.DevArray.from_host(x), 5.0, 3, cap=3)        # the wrapper asks again at the true count
    assert count == m and np.array_equal(lst.view(0, m).to_host(), want)


@pytest.mark.parametrize("level", [1, -1])
@pytest.mark.parametrize("slack", [0, 1, 2])
def test_polarities_and_slack(hip, level, slack):
    """bursts in noise that flips a template bit now and then: with every place allowed more starts pass"""
    x = ais.encode_audio(A.payloads()[:3], 48000.0, [100.25, 1400.5, 2700.75], sigma=0.1, seed=9, levels=level)
    want = check_candidates(hip, x, 5.0, slack=slack)
    tighter = ais.candidates_host(x, 5.0, 3, max(slack - 1, 0))
    assert set(tighter) <= set(want) and (slack == 0 or len(want) > len(tighter))
    det = check_demod(hip, x, 5.0, want)
    near = np.abs(det["t"] - (100.25 + 16 * 5.0)) < 4                # the first burst's template
    assert np.count_nonzero(near) >= 3 and np.any(det["status"][near] == ais.OK)
    assert np.all(det["polarity"][near] == (0 if level == 1 else 1))


@pytest.mark.parametrize("k", range(ais.TEMPLATE))
def test_each_comparison_is_strict(hip, k):
    tie, up, plus = A.tie_cases()[k]
    assert (0 in check_candidates(hip, A.as_audio(tie), 4.0, 3)) == (not plus)   # 16 v = S reads -
    assert (0 in check_candidates(hip, A.as_audio(up), 4.0, 3)) == plus


# ---------------------------------------------------------------------------------------------------------------- demodulation
@pytest.mark.parametrize("i", range(8))
def test_each_payload(hip, i):
    msg = A.payloads()[i]
    for rate in (48000.0, 2048000 / 42.0):
        sps = rate / ais.BAUD
        x = ais.encode_audio([msg], rate, [50.4], sigma=0.02, seed=i)
        ts = check_candidates(hip, x, sps)
        det = check_demod(hip, x, sps, ts)
        ok = np.flatnonzero(det["status"] == ais.OK)
        assert len(ok) >= 1 and all(bytes(det["frames"][j][:len(msg)]) == msg and det["nbits"][j] == 8 * len(msg) + 16 for j in ok)


@pytest.mark.parametrize("at", [63, 64, 65])
def test_a_stuffed_bit_at_a_word_edge(hip, at):
    m = np.zeros(21, dtype=np.uint8)
    stream = np.zeros(168, dtype=np.uint8)
    stream[at - 5:at] = 1
    m[:] = np.packbits(stream, bitorder="little")
    raw = A.frame_raw(m.tobytes())
    assert raw[at] == 0 and raw[at - 5:at].all() and not raw[:at - 5].any()      # the stuffed 0 is raw bit `at`
    det = check_demod(hip, A.as_audio(A.rect(raw, 5, t=9)), 5.0, [9])
    assert det["status"][0] == ais.OK and bytes(det["frames"][0][:21]) == m.tobytes()


def test_the_last_raw_bits(hip):
    stream = np.zeros(1280, dtype=np.uint8)
    stream[1274:1279] = 1                                            # the stuffed 0 would be raw bit 1279: no end flag follows
    det = check_demod(hip, A.as_audio(A.rect(ais.stuff(stream), 4, t=5)), 4.0, [5])
    assert det["status"][0] == ais.NO_END
    last = A.frame_raw(A.message_with_stuffed_length(1272))          # the end flag's closing 0 is raw bit 1279
    assert len(last) == 1280
    det = check_demod(hip, A.as_audio(A.rect(last, 4, t=5)), 4.0, [5])
    assert det["status"][0] == ais.OK and det["nbits"][0] % 8 == 0 and det["nbits"][0] >= 1200
    past = A.frame_raw(A.message_with_stuffed_length(1273))          # one further: it lies outside
    det = check_demod(hip, A.as_audio(A.rect(past, 4, t=5)), 4.0, [5])
    assert det["status"][0] == ais.NO_END
    det = check_demod(hip, A.as_audio(A.rect(np.zeros(1400, np.uint8), 4, t=5)), 4.0, [5])
    assert det["status"][0] == ais.NO_END and not det["frames"].any()


def test_statuses(hip):
    msg = A.payloads()[1]
    raw = A.frame_raw(msg)
    flipped = raw.copy()
    flipped[33] ^= 1
    cases = [(ais.ABORT, np.concatenate((raw[:50], [0], [1] * 7, [0]))), (ais.LENGTH, A.frame_raw(msg, extra=[0])),
             (ais.LENGTH, np.concatenate((raw[:30], [0], ais.FLAG))), (ais.STUFFING, np.concatenate((raw[:40], [0, 1, 1, 1, 1, 1], ais.FLAG))),
             (ais.CRC, flipped), (ais.OK, raw), (ais.LENGTH, np.array(ais.FLAG)), (ais.ABORT, np.ones(20, np.uint8))]
    for status, bits in cases:
        for sps in (5, 16):
            det = check_demod(hip, A.as_audio(A.rect(bits, sps, t=21)), float(sps), [21])
            assert det["status"][0] == status, (ais.STATUS[status], sps)
    det = check_demod(hip, A.as_audio(A.rect(A.frame_raw(msg, extra=[0]), 5, t=21)), 5.0, [21])
    assert det["nbits"][0] == 8 * len(msg) + 17


def test_a_burst_cut_off_and_starts_outside(hip):
    msg = A.payloads()[4]
    x = ais.encode_audio([msg], 48000.0, [40.5], sigma=0.01, seed=2)
    ts = ais.candidates_host(x, 5.0, 3)
    whole = check_demod(hip, x, 5.0, ts)
    assert np.any(whole["status"] == ais.OK)
    for n in (len(x) // 2, int(ts[0]) + ais.reach(5.0, 3) + 40, int(ts[0]) + 1):
        cut = check_demod(hip, x[:n], 5.0, ts)
        assert not np.any(cut["status"] == ais.OK)
    det = check_demod(hip, x, 5.0, np.array([-1, len(x), int(ts[0]), 1 << 40, -(1 << 62)]))
    assert det["status"].tolist()[:2] == [ais.NO_END, ais.NO_END] and det["status"][3] == ais.NO_END and not det["frames"][[0, 1, 3, 4]].any()


@pytest.mark.parametrize("m", [1, 65, 300])
def test_list_lengths(hip, m):
    x = ais.encode_audio(A.payloads()[:2], 48000.0, [50.0, 1500.0], sigma=0.05, seed=m)
    ts = np.random.default_rng(m).integers(0, len(x), m)
    ts[0] = ais.candidates_host(x, 5.0, 3)[0]
    det = check_demod(hip, x, 5.0, ts)
    assert det["status"][0] == ais.OK


# ---------------------------------------------------------------------------------------------------------------- end to end
def same_messages(got, want):
    assert len(got) == len(want)
    for g, v in zip(got, want):
        assert g == v


def test_end_to_end(hip):
    """decode_ais over the host test's recording.  Its front end is float32 on the device, which float64 NumPy does not repeat bit
    for bit; so the device decoder is held exactly (messages, sentences, frameInfo, candidates) to the restatement run over the
    device's own audio, and to decode_host of the recording in what does not hang on a rounding: the messages' bytes, channels,
    fields and sentences, and their starts within a sample."""
    raw, starts = A.recording()
    offsets = (A.OFFSETS["A"], A.OFFSETS["B"])
    dec = decode_ais.decode_ais(source.IQarray(np.array(raw), A.FS), offsets)
    assert dec.audioRate == 48000.0
    audios = [a.to_host() for a in dec.audio()]
    msgs, info, cands = ais.decode(audios, dec.audioRate, ["A", "B"], ops=ais.HostOps())
    same_messages(dec.getMsgs, msgs)
    assert dec.frameInfo == info and dec.getNMEA == [s for m in msgs for s in m["nmea"]]
    assert dec.getVessels == ais.vessels(msgs) and dec.useful == 1
    got = dec.candidateInfo
    for ch in ("A", "B"):
        for key in ("t", "status", "nbits", "rem", "polarity", "score"):
            assert np.array_equal(got[ch][key], cands[ch][key]), (ch, key)
    frames, lengths = dec.getFrames
    assert [bytes(f[:n]) for f, n in zip(frames, lengths)] == A.payloads()       # all eight, in the order sent
    assert set(dec.timings) == {"front_end", "candidates", "demod", "host"}
    hmsgs, hinfo, hvessels = decode_ais.decode_host(np.array(raw), A.FS, offsets)
    assert len(hmsgs) == 8 and hinfo["accepted"] == info["accepted"] == 8
    skip = ("t", "start", "score")
    for g, v in zip(dec.getMsgs, hmsgs):
        assert {k: x for k, x in g.items() if k not in skip} == {k: x for k, x in v.items() if k not in skip}
        assert abs(g["start"] - v["start"]) <= 1
    assert [m["channel"] for m in msgs] == [A.channel_of(i) for i in range(8)]
    assert dec.getVessels.keys() == hvessels.keys()
    same = decode_ais.decode_ais(source.IQarray(np.array(raw), A.FS), offsets, use_device_raw=False)
    same_messages(same.getMsgs, msgs)


def test_from_audio(hip):
    rate = 48000.0
    want = A.payloads()
    x = ais.encode_audio(want, rate, 300.25 + np.arange(8) * 3000.0, sigma=0.03, seed=4, carrier_offsets=np.linspace(-1500, 1500, 8))
    msgs, info, vessels = decode_ais.decode_audio_host(x, rate, "B")
    for audio in (x, hip.DevArray.from_host(x)):
        dec = decode_ais.decode_ais.fromAudio(audio, rate, channel="B")
        same_messages(dec.getMsgs, msgs)
        assert dec.frameInfo == info and dec.getVessels == vessels
        assert [m["raw"] for m in dec.getMsgs] == want
    empty = decode_ais.decode_ais.fromAudio(np.zeros(10), rate)
    assert empty.getMsgs == [] and empty.useful == 0 and empty.frameInfo["candidates"] == 0


def test_rate_limits(hip):
    raw = np.zeros((1000, 2), np.uint8)
    with pytest.raises(ValueError, match="9600"):
        decode_ais.decode_ais(source.IQarray(raw, 240000), bw=30000)             # 30 kS/s: 3.125 samples per bit
    with pytest.raises(ValueError):
        decode_ais.decode_ais.fromAudio(np.zeros(10), 200000.0)
