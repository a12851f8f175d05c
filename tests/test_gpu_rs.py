"""Reed-Solomon correction on the device (dd_lrpt_rs, lrpt.reed_solomon) against lrpt.py's NumPy restatement of DESIGN.md section
4.15, and decode_meteorm2.getVCDUs / rsInfo / getPackets / packetInfo end to end.  All arithmetic is integer and every comparison is
exact.  A frame is one workgroup and a codeword one wave, so the shapes are frames whose four codewords take different ways through
the kernel: clean (the early exit), damaged at and past the radius, at the word's ends, in the parity only, and undecodable."""
import ctypes as C

import numpy as np
import pytest

import _lrpt
import _rs
from directdemod_amd import lrpt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _words(seed, nframes):
    return lrpt.rs_encode(_rng(seed).integers(0, 256, size=(nframes, 4, 223), dtype=np.uint8))


def _hit(word, positions, rng, value=None):
    positions = np.asarray(positions)
    word[positions] ^= rng.integers(1, 256, len(positions), dtype=np.uint8) if value is None else np.uint8(value)


def _both(bodies):
    """the device's answer, held to the restatement's"""
    fixed, errors = lrpt.reed_solomon(bodies)
    want_fixed, want_errors = lrpt.rs_frames_np(bodies)
    assert fixed.dtype == np.uint8 and fixed.shape == (len(bodies), 1020) and errors.shape == (len(bodies), 4)
    assert np.array_equal(errors, want_errors), (errors.tolist(), want_errors.tolist())
    assert np.array_equal(fixed, want_fixed)
    return fixed, errors


@pytest.mark.parametrize("n", [0, 1, 3, 5])
def test_frame_counts(hip, n):
    rng = _rng(40 + n)
    sent = _words(50 + n, n)
    got = sent.copy()
    count = rng.integers(0, 17, size=(n, 4))
    for f in range(n):
        for w in range(4):
            _hit(got[f, w], rng.choice(255, count[f, w], replace=False), rng)
    fixed, errors = _both(lrpt.interleave(got).reshape(n, 1020))
    assert np.array_equal(errors, count) and np.array_equal(fixed, lrpt.interleave(sent).reshape(n, 1020))


def test_clean_one_sixteen_and_seventeen_in_one_frame(hip):
    # the early exit, both edges and the failure in one workgroup: no wave waits for another
    rng = _rng(60)
    sent = _words(61, 1)
    got = sent.copy()
    for w, e in enumerate((0, 1, 16, 17)):
        _hit(got[0, w], rng.choice(255, e, replace=False), rng)
    fixed, errors = _both(lrpt.interleave(got))
    assert errors.tolist() == [[0, 1, 16, -1]]
    back = lrpt.deinterleave(fixed)
    assert np.array_equal(back[0, :3], sent[0, :3]) and np.array_equal(back[0, 3], got[0, 3])


def test_errors_at_the_ends_in_parity_and_in_data(hip):
    rng = _rng(62)
    sent = _words(63, 1)
    got = sent.copy()
    _hit(got[0, 0], [0], rng)
    _hit(got[0, 1], [254], rng)
    _hit(got[0, 2], 223 + rng.choice(32, 16, replace=False), rng)
    _hit(got[0, 3], rng.choice(223, 16, replace=False), rng)
    fixed, errors = _both(lrpt.interleave(got))
    assert errors.tolist() == [[1, 1, 16, 16]] and np.array_equal(fixed, lrpt.interleave(sent))


def test_sixteen_adjacent_and_sixteen_of_value_one(hip):
    rng = _rng(64)
    sent = _words(65, 1)
    got = sent.copy()
    _hit(got[0, 0], np.arange(100, 116), rng)
    _hit(got[0, 1], rng.choice(255, 16, replace=False), rng, value=0x01)
    _hit(got[0, 2], np.arange(239, 255), rng)
    _hit(got[0, 3], np.arange(0, 16), rng, value=0x01)
    fixed, errors = _both(lrpt.interleave(got))
    assert errors.tolist() == [[16] * 4] and np.array_equal(fixed, lrpt.interleave(sent))


@pytest.mark.parametrize("value", [0x00, 0xFF])
def test_constant_frames_are_codewords(hip, value):
    body = np.full((1, 1020), value, dtype=np.uint8)
    assert not lrpt.rs_syndromes(lrpt.deinterleave(body)).any()              # x^254 + ... + 1 vanishes at every root but 1
    fixed, errors = _both(body)
    assert errors.tolist() == [[0] * 4] and np.array_equal(fixed, body)


def test_random_frame_is_left_alone(hip):
    body = _rng(66).integers(0, 256, size=(1, 1020), dtype=np.uint8)
    fixed, errors = _both(body)
    assert errors.tolist() == [[-1] * 4] and np.array_equal(fixed, body)


def test_seventeen_to_twenty_four_errors(hip):
    rng = _rng(67)
    sent = _words(68, 6)
    got = sent.copy()
    for k, word in enumerate(got.reshape(24, 255)):
        _hit(word, rng.choice(255, 17 + k % 8, replace=False), rng)
    bodies = lrpt.interleave(got)
    assert np.all(lrpt.rs_frames_np(bodies)[1] == -1)                        # the restatement's answer for these seeds: none is in reach
    fixed, errors = _both(bodies)
    assert np.all(errors == -1) and np.array_equal(fixed, bodies)


def test_device_input_and_poisoned_tails(hip):
    rng = _rng(69)
    got = _words(70, 3)
    for word in got.reshape(12, 255):
        _hit(word, rng.choice(255, 9, replace=False), rng)
    bodies = lrpt.interleave(got)
    want_fixed, want_errors = lrpt.rs_frames_np(bodies)
    dev = hip.DevArray.from_host(bodies.ravel())
    fixed, errors = lrpt.reed_solomon(dev)
    assert np.array_equal(fixed, want_fixed) and np.array_equal(errors, want_errors)
    out = hip.DevArray.from_host(np.full(3 * 1020 + 16, 0xA5, dtype=np.uint8))
    err = hip.DevArray.from_host(np.full(3 * 4 + 4, -77, dtype=np.int32))
    hip.check(hip.lib().dd_lrpt_rs(dev.ptr, 3, out.ptr, err.ptr, None))
    o, e = out.to_host(), err.to_host()
    assert np.array_equal(o[:3 * 1020].reshape(3, 1020), want_fixed) and np.all(o[3 * 1020:] == 0xA5)
    assert np.array_equal(e[:12].reshape(3, 4), want_errors) and np.all(e[12:] == -77)
    hip.check(hip.lib().dd_lrpt_rs(None, 0, None, None, None))               # no frames: nothing is touched


def test_bad_arguments(hip):
    dev = hip.DevArray.from_host(np.zeros(1020, dtype=np.uint8))
    out = hip.DevArray(1020, np.uint8)
    err = hip.DevArray(4, np.int32)
    for args in ((dev.ptr, -1, out.ptr, err.ptr), (None, 1, out.ptr, err.ptr), (dev.ptr, 1, None, err.ptr), (dev.ptr, 1, out.ptr, None)):
        with pytest.raises(ValueError):
            hip.check(hip.lib().dd_lrpt_rs(*args, None))
    for bad in (np.zeros((2, 1019), dtype=np.uint8), np.zeros(1020, dtype=np.uint8), hip.DevArray(1021, np.uint8),
                hip.DevArray(1020, np.int8)):
        with pytest.raises(ValueError):
            lrpt.reed_solomon(bad)


# ------------------------------------------------------------------ decode_meteorm2.getVCDUs / rsInfo / getPackets / packetInfo
def test_packets_end_to_end_case_b(hip):
    from directdemod_amd import decode_meteorm2, source
    raw, built, _ = _rs.case("b")
    obj = decode_meteorm2.decode_meteorm2(source.IQarray(raw, _rs.FS), 0)
    frames, finfo = obj.getFrames, obj.frameInfo
    vcdus, rs, pkts, pinfo = obj.getVCDUs, obj.rsInfo, obj.getPackets, obj.packetInfo
    assert vcdus.dtype == np.uint8 and vcdus.shape == (len(frames), 892) and rs.dtype == lrpt.RS_INFO and len(rs) == len(frames)
    assert pinfo.dtype == lrpt.PACKET_INFO and len(pinfo) == len(pkts)
    want_fixed, want_errors = lrpt.rs_frames_np(frames)
    assert np.array_equal(rs["errors"], want_errors) and np.array_equal(vcdus, want_fixed[:, :892])
    assert np.array_equal(rs["ok"], np.all(want_errors >= 0, axis=1))
    # against what was sent, frame by frame through (vcid, counter) of the corrected headers
    rows, state = _rs.match(built, rs["vcid"], rs["counter"], rs["ok"])
    assert _rs.SHORT in rows and _rs.LONG in rows and rows == sorted(set(rows))
    for i, r in enumerate(rows):
        if rs["ok"][i]:
            assert np.array_equal(vcdus[i], built["vcdus"][r]), r
            assert (int(rs["vcid"][i]), int(rs["counter"][i])) == (int(built["vcid"][r]), int(built["counter"][r]))
        else:
            assert np.array_equal(vcdus[i], frames[i, :892])
    short = rs["errors"][rows.index(_rs.SHORT)]
    assert rs["ok"][rows.index(_rs.SHORT)] and np.all((short >= 1) & (short <= 16))
    assert not rs["ok"][rows.index(_rs.LONG)]
    assert state[_rs.LONG + 1] == "ok" and not rs["errors"][rows.index(_rs.LONG + 1)].any()
    want = _rs.expected(built, state)
    assert pkts == [p["data"] for p in want] and len(pkts) >= 8
    assert pinfo["vcid"].tolist() == [p["vcid"] for p in want] and pinfo["frame"].tolist() == [rows.index(p["first"]) for p in want]
    assert pinfo["length"].tolist() == [len(p) for p in pkts]
    assert [(int(r["apid"]), int(r["flags"]), int(r["count"])) for r in pinfo] == \
           [tuple(lrpt.packet_header(p)[k] for k in ("apid", "flags", "count")) for p in pkts]
    assert next(p for p in built["packets"] if p["first"] == _rs.LONG + 1)["data"] in pkts
    # getFrames and frameInfo are what the frame decoder's stages return, with or without the new properties
    w = obj.walker()
    soft = lrpt.soft_symbols(w.view("sym"))
    starts = lrpt.frame_starts(lrpt.asm_candidates(soft, w.nsym), w.nsym)
    bodies, fin = lrpt.finish(lrpt.viterbi(soft, w.nsym, starts[:, :2]), soft, w.nsym, starts[:, :2])
    assert np.array_equal(frames, bodies) and obj.getFrames is frames and obj.frameInfo is finfo
    assert finfo.dtype == lrpt.INFO and np.array_equal(finfo["symbol"], starts[:, 0]) and np.array_equal(finfo["hypothesis"], starts[:, 1])
    assert np.array_equal(finfo["asm_errors"], fin[:, 0]) and np.array_equal(finfo["corrected"], fin[:, 1])
    assert np.array_equal(finfo["vcid"], fin[:, 2])
    assert obj.getVCDUs is vcdus and obj.getPackets is pkts
    for k in ("lrpt_rs", "lrpt_packets", "lrpt_finish"):
        assert obj.timings[k] >= 0.0


def test_random_bodies_give_no_packets_case_a(hip):
    from directdemod_amd import decode_meteorm2, source
    raw, _, _ = _lrpt.case("a")
    obj = decode_meteorm2.decode_meteorm2(source.IQarray(raw, _lrpt.FS), 0)
    frames = obj.getFrames
    assert len(frames) >= 10
    assert not obj.rsInfo["ok"].any() and np.all(obj.rsInfo["errors"] == -1)
    assert np.array_equal(obj.getVCDUs, frames[:, :892])
    assert obj.getPackets == [] and obj.packetInfo.shape == (0,)
