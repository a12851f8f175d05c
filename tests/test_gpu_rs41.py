"""The RS41 kernels on the device (dd_rs41.h through dd_rs41_candidates, dd_rs41_frames and the diagnostics dd_debug_rs41_masks and
dd_debug_rs41_rs, the wrappers of directdemod_amd/rs41.py and decode_rs41) against the NumPy restatement in rs41.py.

Everything behind the quantiser is integer, so every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import _rs41 as T
from directdemod_amd import decode_rs41, rs41, source

pytestmark = pytest.mark.gpu

SENT = np.int64(-0x5A5A5A5A5A5A5A5B)
SPARE = 16
SPS = [4.0, 10.0, 10.16, 64.0]


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def w_of(sps):
    return rs41.params(sps * 4800.0)[1]


def dev_candidates(hip, audio, sps, w, slack, cap):
    """dd_rs41_candidates with `cap` places and SPARE sentinels behind them -> (rc, count, the places, the sentinels still whole)"""
    x = hip.DevArray.from_host(np.ascontiguousarray(audio if len(audio) else np.zeros(1), dtype=np.float64))
    lst = hip.DevArray.from_host(np.full(cap + SPARE, SENT))
    count = C.c_int64(-1)
    rc = hip.lib().dd_rs41_candidates(x.ptr, len(audio), float(sps), int(w), int(slack), lst.ptr, cap, C.byref(count), None)
    hip.sync()
    got = lst.to_host()
    return rc, count.value, got[:cap], bool(np.all(got[cap:] == SENT))


def check_candidates(hip, audio, sps, w=None, slack=4):
    """the device's list and, through the diagnostic entry, its mask bytes against the restatement's"""
    w = w_of(sps) if w is None else w
    masks = rs41.masks_host(audio, sps, w, slack)
    want = np.flatnonzero(masks & 1).astype(np.int64)
    rc, count, got, whole = dev_candidates(hip, audio, sps, w, slack, len(want) + 3)
    assert rc == 0 and count == len(want) and whole
    assert np.array_equal(got[:count], want) and np.all(got[count:] == SENT)
    if len(audio):
        dev = rs41.masks_device(hip.DevArray.from_host(np.ascontiguousarray(audio, dtype=np.float64)), sps, w, slack)
        assert np.array_equal(dev[:len(masks)], masks) and not dev[len(masks):].any()
    return want


def dev_frames(hip, audio, sps, w, ts):
    """dd_rs41_frames with sentinels behind every output -> the dict of rs41.frames_host"""
    m = len(ts)
    x = hip.DevArray.from_host(np.ascontiguousarray(audio, dtype=np.float64)) if len(audio) else None
    lst = hip.DevArray.from_host(np.ascontiguousarray(ts, dtype=np.int64))
    fixed = hip.DevArray.from_host(np.full(rs41.EXT * m + SPARE, 0xA5, np.uint8))
    recv = hip.DevArray.from_host(np.full(rs41.EXT * m + SPARE, 0xA5, np.uint8))
    meta = hip.DevArray.from_host(np.full(6 * m + SPARE, -0x5A5A5A5B, np.int32))
    rc = hip.lib().dd_rs41_frames(x.ptr if x else None, len(audio), float(sps), int(w), lst.ptr, m, fixed.ptr, recv.ptr, meta.ptr, None)
    hip.sync()
    assert rc == 0
    fx, rx, mt = fixed.to_host(), recv.to_host(), meta.to_host()
    k = rs41.EXT * m
    assert np.all(fx[k:] == 0xA5) and np.all(rx[k:] == 0xA5) and np.all(mt[6 * m:] == -0x5A5A5A5B)
    mt = mt[:6 * m].reshape(m, 6)
    return {"t": np.asarray(ts, dtype=np.int64), "fixed": fx[:k].reshape(m, rs41.EXT), "recv": rx[:k].reshape(m, rs41.EXT),
            "status": mt[:, 0], "polarity": mt[:, 1], "length": mt[:, 2], "mis": mt[:, 3], "errs": mt[:, 4:6]}


KEYS = ("t", "fixed", "recv", "status", "polarity", "length", "mis", "errs")


def check_frames(hip, audio, sps, ts, w=None):
    w = w_of(sps) if w is None else w
    got = dev_frames(hip, audio, sps, w, ts)
    want = rs41.frames_host(audio, sps, w, ts)
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    return got


# ---------------------------------------------------------------------------------------------------------------- the Reed-Solomon wave
@pytest.fixture(scope="module")
def rs_reference():
    words = T.rs_words()
    return {fv: rs41.rs_decode_np(words, fv) for fv in (0, 99)}


@pytest.mark.parametrize("first_valid", [0, 99])
@pytest.mark.parametrize("m", [1, 65, 300])
def test_reed_solomon_wave(hip, rs_reference, m, first_valid):
    """dd_rs_wave<12, 1, 0> over the 0x11D table against the restatement, word for word"""
    words = T.rs_words()
    pick = np.arange(300)[::-1][:m] if m < 300 else np.arange(300)       # m = 1: the last word; 65: the edge positions' rows among them
    fixed, errors = rs41.rs_device(words[pick], first_valid)
    want_fixed, want_errors = rs_reference[first_valid]
    assert np.array_equal(errors, want_errors[pick]) and np.array_equal(fixed, want_fixed[pick])
    if m == 300:
        assert errors[0] == 0 and not fixed[0].any()                     # the all-zero word
        assert errors[10:30].tolist() == ([1] * 20 if first_valid == 0 else want_errors[10:30].tolist())
        assert (errors[160:180] == 1).all() and (errors[180:200] == 6).all() and (errors[200:220] == 12).all()
        full = errors[[90, 91, 92, 93, 94, 95, 96, 97]].tolist()
        short = errors[[240, 241, 242, 243, 244, 245, 246, 247]].tolist()
        assert short == ([1, 1, 1, 1, 2, 2, 4, 4] if first_valid == 0 else [-1, -1, 1, 1, -1, -1, -1, 4])
        assert full == ([1, 1, 1, 1, 2, 2, 4, 5] if first_valid == 0 else [-1, -1, 1, 1, -1, -1, -1, -1])
        assert errors[250:257].tolist() == [1, 2, 3, 6, 11, 12, 12]      # the parity only
        for e, f, w in zip(errors[220:240], fixed[220:240], words[220:240]):     # thirteen: none, or another word within twelve
            assert (e == -1 and np.array_equal(f, w)) or (not rs41.rs_syndromes(f).any() and e == (f != w).sum() <= 12)


# ---------------------------------------------------------------------------------------------------------------- candidates
@pytest.mark.parametrize("sps", SPS)
@pytest.mark.parametrize("slack", [0, 4, rs41.SLACK_MAX])
def test_candidates_on_noise(hip, sps, slack):
    """Gaussian noise of 2^15 samples, 128 tiles, with three headers in it, the last with five places wrong"""
    rng = np.random.default_rng(int(sps * 1000) + slack)
    audio = rng.normal(0.0, 0.25, 1 << 15)
    for t, wrong, polarity in ((700, 0, 0), (9000, 3, 1), (20000, 5, 0)):
        h = T.as_audio(T.fractional(T.header_bits(wrong), sps, t + 0.3, amp=300000, polarity=polarity))[t:]
        audio[t:t + len(h)] += h
    want = check_candidates(hip, audio, sps, slack=slack)
    assert np.any(np.abs(want - 700) <= sps) and (slack < 5 or np.any(np.abs(want - 20000) <= sps))


@pytest.mark.parametrize("sps", SPS)
def test_zero_and_full_scale_audio(hip, sps):
    for fill in (0.0, np.pi, -np.pi):
        audio = np.full(9000, fill)
        assert len(check_candidates(hip, audio, sps, slack=rs41.SLACK_MAX)) == 0     # every comparison an equality: 25 places off


@pytest.mark.parametrize("sps", [4, 10, 64])
def test_shortest_audio_and_a_header_on_the_last_sample(hip, sps):
    w = w_of(float(sps))
    full = rs41.reach(float(sps), w)
    x = T.as_audio(T.header_rect(sps, t=0, n=full + 2000))
    assert rs41.n_starts(full - 1, float(sps), w) == 0 and rs41.n_starts(full, float(sps), w) == 1
    rc, count, got, whole = dev_candidates(hip, x[:full - 1], float(sps), w, 0, 4)
    assert (rc, count, whole) == (0, 0, True) and np.all(got == SENT)
    assert check_candidates(hip, x[:full], float(sps), slack=0).tolist() == [0]      # the one start there is
    rc, count, got, whole = dev_candidates(hip, x[:0], float(sps), w, 0, 4)         # n = 0
    assert (rc, count, whole) == (0, 0, True) and np.all(got == SENT)
    for t in (1, 300, 1021):                                         # the header ends on the last sample
        y = T.as_audio(T.header_rect(sps, t=t, n=t + full))
        want = check_candidates(hip, y, float(sps), slack=0)
        assert want[-1] == t == rs41.n_starts(len(y), float(sps), w) - 1


@pytest.mark.parametrize("edge", [256, 1024])
def test_passes_around_tile_edges(hip, edge):
    for sps in (4, 7):
        for t in (edge - 1, edge):
            want = check_candidates(hip, T.as_audio(T.header_rect(sps, t=t)), float(sps), slack=0)
            assert t in want
    x = T.as_audio(T.header_rect(40, t=edge - 12))                   # a run of adjacent passes that lies across the edge
    want = check_candidates(hip, x, 40.0, slack=0)
    assert np.any(want < edge) and np.any(want >= edge) and len(want) >= 16


@pytest.mark.parametrize("polarity", [0, 1])
@pytest.mark.parametrize("wrong", range(6))
def test_polarities_and_slack(hip, polarity, wrong):
    frame = T.frame_bits(rs41.build_frame(T.NORTH))
    for sps in (4, 10):
        x = T.as_audio(T.rect(np.concatenate((T.header_bits(wrong), frame[64:])), sps, t=77, polarity=polarity))
        w = w_of(float(sps))
        masks = rs41.masks_host(x, float(sps), w, 4)
        assert masks[77] == (0 if wrong > 4 else (3 if polarity else 1))
        want = check_candidates(hip, x, float(sps), slack=4)
        assert (77 in want) == (wrong <= 4)                          # the list holds both polarities' passes
        det = check_frames(hip, x, float(sps), [77])
        assert det["polarity"][0] == polarity and det["mis"][0] == wrong and det["errs"][0].tolist() == [0, 0]


@pytest.mark.parametrize("k", range(64))
def test_each_comparison_is_strict(hip, k):
    """on the threshold a place reads 0: a one-place then fails the header, a zero-place holds; one unit towards a 1 turns both"""
    for polarity in (0, 1):
        tie, nudged, one = T.tie_cases(polarity)[k]
        assert (0 in check_candidates(hip, T.as_audio(tie), 4.0, 3, slack=0)) == (not one)
        assert (0 in check_candidates(hip, T.as_audio(nudged), 4.0, 3, slack=0)) == one


def test_capacities(hip):
    x = rs41.encode([T.NORTH], 4800.0 * 8, start=50.5, sigma=0.02, seed=7, preamble=64)
    want = rs41.candidates_host(x, 8.0, 5)
    m = len(want)
    assert m >= 3
    for cap in (0, 1, m - 1, m, m + 5):
        rc, count, got, whole = dev_candidates(hip, x, 8.0, 5, 4, cap)
        assert count == m and whole
        assert rc == (0 if cap >= m else hip.DD_ERR_INVALID)
        kept = min(cap, m)
        assert np.array_equal(got[:kept], want[:kept]) and np.all(got[kept:] == SENT)
    lst, count = rs41.candidates(hip.DevArray.from_host(x), 8.0, 5, cap=1)          # the wrapper asks again at the true count
    assert count == m and np.array_equal(lst.view(0, m).to_host(), want)


# ---------------------------------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("polarity", [0, 1])
@pytest.mark.parametrize("sps", [7.5, 10.16])
def test_standard_and_extended_frames_at_fractional_samples_per_bit(hip, sps, polarity):
    for fields in (T.SOUTH, T.extended(T.SOUTH)):
        frame = rs41.build_frame(fields)
        bad = T.damage(T.damage(frame, 0, 5, 1), 1, 12, 2)
        x = T.as_audio(T.fractional(T.frame_bits(bad), sps, t=301.3, polarity=polarity))
        ts = check_candidates(hip, x, sps, slack=0)
        assert len(ts) >= int(sps) // 2 and np.all(np.abs(ts - 301.3) < sps)
        det = check_frames(hip, x, sps, [301, 302, 304, 299])
        assert det["length"][0] == len(frame) and det["polarity"][0] == polarity and det["errs"][0].tolist() == [5, 12]
        assert np.array_equal(det["fixed"][0, :len(frame)], frame) and np.array_equal(det["recv"][0, :len(frame)], bad)
        assert not det["fixed"][0, len(frame):].any() and not det["recv"][0, len(frame):].any()


def test_a_frame_cut_off_and_starts_outside(hip):
    std, ext = rs41.build_frame(T.NORTH), rs41.build_frame(T.extended(T.NORTH))
    x = T.as_audio(T.rect(T.frame_bits(ext), 4, t=9))
    w = w_of(4.0)
    last = lambda nbytes: 9 + 4 * 8 * nbytes - 2 + w // 2            # noqa: E731  the last sample the frame's last bit reads
    for n, status, length in ((last(320), rs41.OUTSIDE, 0), (last(320) + 1, rs41.OK, 320), (9 + 32 * 400, rs41.OK, 320),
                              (last(518), rs41.OK, 320), (last(518) + 1, rs41.OK, 518), (len(x), rs41.OK, 518)):
        det = check_frames(hip, x[:n], 4.0, [9])
        assert det["status"][0] == status and det["length"][0] == length
        if length == 518:
            assert det["errs"][0].tolist() == [0, 0] and np.array_equal(det["fixed"][0], ext)
        elif length == 320:                                          # an extended frame read as a standard one: not decodable
            assert det["errs"][0].tolist() == [-1, -1] and np.array_equal(det["fixed"][0, :320], ext[:320])
    y = T.as_audio(T.rect(T.frame_bits(std), 4, t=9))
    n = len(y)
    det = check_frames(hip, y, 4.0, np.array([-1, n, n - 1, 9, 1 << 40, -(1 << 62), n - 4 * 2560]))
    assert det["status"].tolist() == [rs41.OUTSIDE, rs41.OUTSIDE, rs41.OUTSIDE, rs41.OK, rs41.OUTSIDE, rs41.OUTSIDE, rs41.OK]
    assert not det["fixed"][[0, 1, 2, 4, 5]].any() and not det["recv"][[0, 1, 2, 4, 5]].any() and det["errs"][3].tolist() == [0, 0]
    det = check_frames(hip, y[:0], 4.0, np.array([0, 9, -1, 1 << 40]))     # no audio, and a list: every start is outside
    assert det["status"].tolist() == [rs41.OUTSIDE] * 4 and not det["fixed"].any() and not det["recv"].any() and not det["errs"].any()


@pytest.mark.parametrize("m", [1, 65, 300])
def test_list_lengths(hip, m):
    x = rs41.encode([T.NORTH, T.extended(T.SOUTH)], 4800.0 * 8, gap=0.7, start=50.0, sigma=0.05, seed=m, preamble=64)
    ts = np.random.default_rng(m).integers(0, len(x), m)
    ts[0] = rs41.candidates_host(x, 8.0, 5)[0]
    det = check_frames(hip, x, 8.0, ts)
    assert det["errs"][0].tolist() == [0, 0]


@pytest.mark.parametrize("flips", [0x01, 0x03, 0x07, 0x0F, 0x10, 0x30, 0x70, 0xF0, 0x81, 0xC3])
def test_the_type_byte_with_bits_flipped(hip, flips):
    """one to four bits of byte 56 flipped either way: the nearer of 0F and F0 gives the length, a tie the standard one"""
    for fields in (T.NORTH, T.extended(T.NORTH)):
        frame = rs41.build_frame(fields)
        bad = frame.copy()
        bad[rs41.TYPE_AT] ^= flips
        det = check_frames(hip, T.as_audio(T.rect(T.frame_bits(bad), 4, t=5)), 4.0, [5])
        ty = int(bad[rs41.TYPE_AT])
        want = 518 if bin(ty ^ 0xF0).count("1") < bin(ty ^ 0x0F).count("1") else 320
        assert det["length"][0] == want
        if want == len(frame):
            assert det["errs"][0].tolist() == [1, 0] and np.array_equal(det["fixed"][0, :want], frame)


@pytest.mark.parametrize("codeword", [0, 1])
def test_twelve_and_thirteen_errors_in_one_codeword(hip, codeword):
    for fields in (T.NORTH, T.extended(T.NORTH)):
        frame = rs41.build_frame(fields)
        for ne in (12, 13):
            bad = T.damage(frame, codeword, ne, 10 * ne + codeword)
            det = check_frames(hip, T.as_audio(T.rect(T.frame_bits(bad), 4, t=5)), 4.0, [5])
            errs = det["errs"][0].tolist()
            assert errs[1 - codeword] == 0
            if ne == 12:
                assert errs[codeword] == 12 and np.array_equal(det["fixed"][0, :len(frame)], frame)
            else:                                                    # none, or another codeword within twelve
                assert errs[codeword] == -1 or 0 < errs[codeword] <= 12


# ---------------------------------------------------------------------------------------------------------------- end to end
def same_frames(got, want):
    assert len(got) == len(want)
    for g, v in zip(got, want):
        assert g == v


def test_end_to_end(hip):
    """decode_rs41 over the shared recording.  Its front end is float32 on the device, which float64 NumPy does not repeat bit for
    bit; so the device decoder is held exactly (frames, frameInfo, candidates) to the restatement run over the device's own audio,
    and to decode_host of the recording in what does not hang on a rounding: every field of every frame."""
    raw = T.recording()
    dec = decode_rs41.decode_rs41(source.IQarray(np.array(raw), T.FS), T.OFFSET)
    assert abs(dec.audioRate - T.FS / 42.0) < 1e-9
    audio = dec.audio().to_host()
    found, info, cands = rs41.decode(audio, dec.audioRate, ops=rs41.HostOps())
    same_frames(dec.getFrames, [decode_rs41._public(f) for f in found])
    assert dec.frameInfo == info and dec.useful == 1 and info["ok"] == 3
    got = dec.candidateInfo
    for key in KEYS:
        assert np.array_equal(got[key], cands[key]), key
    frames, lengths = dec.getRaw
    assert lengths.tolist() == [320, 518, 320] and frames.shape == (3, 518)
    for k, (f, fields) in enumerate(zip(dec.getFrames, T.RECORDING_FIELDS)):
        T.same_fields(f, fields)
        assert f["status"] == "ok" and np.array_equal(frames[k, :lengths[k]], rs41.build_frame(fields))
    assert [len(v) for v in dec.getTrack.values()] == [3] and dec.getTrack["S1234567"][0][0] == rs41.gps_time(2337, 302400123)
    sonde = dec.getSondes["S1234567"]
    assert (sonde["first"], sonde["last"], sonde["frames"]) == (4321, 4323, 3) and np.flatnonzero(sonde["seen"]).tolist() == [5, 6, 7]
    assert set(dec.timings) == {"front_end", "candidates", "frames", "host"}
    hfound, hinfo = decode_rs41.decode_host(np.array(raw), T.FS, T.OFFSET)
    assert len(hfound) == 3 and hinfo["ok"] == 3
    for g, v in zip(dec.getFrames, hfound):
        for key in g:
            if key not in ("t", "start", "corrected", "header_errors"):
                assert g[key] == v[key], key
        assert abs(g["start"] - v["start"]) <= dec.audioRate / rs41.BAUD         # the merge picks one start of a bit time of them


def test_from_audio_inside_a_frame_and_follow(hip):
    rate = 48000.0
    fields = [dict(T.SOUTH, frame_number=20 + k) for k in range(4)]
    fields[2] = T.extended(fields[2])
    x = rs41.encode(fields, rate, polarity=1, start=100.0, sigma=0.05, seed=4)
    found, info = decode_rs41.decode_audio_host(x, rate)
    assert [f["frame_number"] for f in found] == [20, 21, 22, 23]
    for audio in (x, hip.DevArray.from_host(x)):
        dec = decode_rs41.decode_rs41.fromAudio(audio, rate)
        same_frames(dec.getFrames, found)
        assert dec.frameInfo == info
    cut = int(rs41.frame_start(rate, 0, 100.0)) + 5000               # a recording that starts inside the first frame
    dec = decode_rs41.decode_rs41.fromAudio(hip.DevArray.from_host(x[cut:]), rate)
    assert [f["frame_number"] for f in dec.getFrames] == [21, 22, 23]
    same_frames(dec.getFrames, decode_rs41.decode_audio_host(x[cut:], rate)[0])
    at = int(rs41.frame_start(rate, 2, 100.0))                       # the third frame's header: twenty places set to the other level
    for k in np.flatnonzero(T.header_bits(20) != T.header_bits(0)):
        x[at + 10 * k:at + 10 * (k + 1)] *= -1.0
    for follow, numbers in ((2, [20, 21, 22, 23]), (0, [20, 21, 23])):
        dec = decode_rs41.decode_rs41.fromAudio(hip.DevArray.from_host(x), rate, follow=follow)
        assert [f["frame_number"] for f in dec.getFrames] == numbers and dec.frameInfo["followed"] == (1 if follow else 0)
        same_frames(dec.getFrames, decode_rs41.decode_audio_host(x, rate, follow=follow)[0])
    empty = decode_rs41.decode_rs41.fromAudio(np.zeros(10), rate)
    assert empty.getFrames == [] and empty.useful == 0 and empty.frameInfo["frames"] == 0 and empty.getRaw[0].shape == (0, 518)
