"""RS41 radiosonde decoding on the CPU: the format's constants, the Reed-Solomon restatement, the
synthesiser through the NumPy restatement of both kernels and the host logic (rs41.decode, decode_rs41.decode_audio_host), and the
slack bound."""
import numpy as np
import pytest

import _rs41 as T
from directdemod_amd import decode_rs41, rs41

RATES = (48000.0, 48768.0)            # 10 and 10.16 samples per bit


# ---------------------------------------------------------------------------------------------------------------- the format
def test_mask_and_header():
    on_air = np.frombuffer(rs41.HEADER, dtype=np.uint8)
    assert bytes(on_air ^ rs41.MASK[:8]) == bytes.fromhex("8635F44093DF1A60") == rs41.HEADER_CLEAR
    sent = "0000100001101101" "0101001110001000" "0100010001101001" "0100100000011111"
    assert "".join("01"[int(b)] for b in rs41.HEADER_BITS) == sent
    assert "".join("01"[(v >> k) & 1] for v in on_air for k in range(8)) == sent         # each byte's lowest bit first
    assert rs41.HEADER_BITS.sum() == rs41.ONES == 25 and (~rs41.HEADER_BITS).sum() == rs41.ZEROS == 39
    assert len(rs41.MASK) == 64 and rs41.MASK[0] == 0x96 and rs41.MASK[63] == 0xC1


def test_crc():
    assert rs41.crc16(b"123456789") == 0x29B1


def test_block_offsets_of_an_encoded_frame():
    f = rs41.build_frame(T.NORTH)
    assert len(f) == rs41.STD == 0x140 and bytes(f[:8]) == rs41.HEADER_CLEAR and f[rs41.TYPE_AT] == 0x0F
    blocks = rs41.blocks_of(f, len(f), True)
    assert [(b["at"], b["id"], len(b["bytes"])) for b in blocks] == list(rs41.LAYOUT)
    assert all(b["crc_ok"] for b in blocks) and not any(blocks[-1]["bytes"])
    assert blocks[-1]["at"] + 2 + 0x11 + 2 == 0x140
    e = rs41.build_frame(T.extended(T.NORTH))
    assert len(e) == rs41.EXT and e[rs41.TYPE_AT] == 0xF0
    eb = rs41.blocks_of(e, len(e), True)
    assert [(b["at"], b["id"]) for b in eb[:6]] == [(o, i) for o, i, _ in rs41.LAYOUT[:5]] + [(0x12B, 0x7E)]
    assert eb[5]["bytes"] == T.XDATA and eb[6]["id"] == 0x76 and eb[6]["at"] + 4 + len(eb[6]["bytes"]) == rs41.EXT


def test_quantiser_unit():
    assert rs41.quantise(T.as_audio(np.arange(-5000, 5000))).tolist() == list(range(-5000, 5000))


# ---------------------------------------------------------------------------------------------------------------- Reed-Solomon
def _random_words(count, seed):
    return np.array(rs41.rs_encode(np.random.default_rng(seed).integers(0, 256, (count, 231)).astype(np.uint8)))


def test_an_encoded_word_has_zero_syndromes():
    words = _random_words(8, 1)
    assert rs41.rs_syndromes(words).shape == (8, 24) and not rs41.rs_syndromes(words).any()
    ex, lg = rs41.gf_tables()
    p = 254 - np.arange(255)                                         # byte i is the coefficient of x^(254 - i)
    for j in (0, 1, 23):                                             # and directly: c(alpha^j) = 0
        terms = np.where(words[0] == 0, 0, ex[(lg[words[0]].astype(np.int64) + j * p) % 255])
        assert np.bitwise_xor.reduce(terms) == 0
    frame = rs41.build_frame(T.NORTH)
    assert not rs41.rs_syndromes(rs41.codewords(frame, rs41.STD)).any()
    assert not rs41.codewords(frame, rs41.STD)[:, :99].any() and rs41.first_valid(rs41.STD) == 99 and rs41.first_valid(rs41.EXT) == 0
    c0 = rs41.codewords(frame, rs41.STD)[0]                          # c_p = frame[8 + p] below 24, frame[56 + 2 (p - 24)] from there on
    assert c0[254 - 0] == frame[8] and c0[254 - 23] == frame[31] and c0[254 - 24] == frame[56] and c0[254 - 155] == frame[56 + 262]


@pytest.mark.parametrize("ne", [0, 1, 12])
def test_errors_within_reach_are_corrected(ne):
    words = _random_words(6, 2 + ne)
    bad = words.copy()
    T.spoil(bad, range(6), [np.random.default_rng(r).choice(255, ne, replace=False) for r in range(6)], np.random.default_rng(5))
    fixed, errors = rs41.rs_decode_np(bad)
    assert np.array_equal(fixed, words) and errors.tolist() == [ne] * 6


def test_thirteen_errors():
    words = _random_words(12, 7)
    bad = words.copy()
    T.spoil(bad, range(12), [np.random.default_rng(r).choice(255, 13, replace=False) for r in range(12)], np.random.default_rng(6))
    fixed, errors = rs41.rs_decode_np(bad)
    for f, b, e in zip(fixed, bad, errors):                           # -1 with the word untouched, or another valid word within 12
        assert (e == -1 and np.array_equal(f, b)) or (not rs41.rs_syndromes(f).any() and e == (f != b).sum() <= 12)


def test_an_error_in_the_shortened_part_is_rejected():
    frame = rs41.build_frame(T.SOUTH)
    word = rs41.codewords(frame, rs41.STD)[1]
    for at in (0, 50, 98):
        bad = word.copy()
        bad[[at, 200]] ^= 0x5A
        fixed, errors = rs41.rs_decode_np(bad, 99)
        assert errors == -1 and np.array_equal(fixed, bad)
        fixed, errors = rs41.rs_decode_np(bad, 0)                    # the full code corrects it
        assert errors == 2 and np.array_equal(fixed, word)
    bad = word.copy()
    bad[[99, 254]] ^= 0xA5                                           # the first byte of the frame's own part, and the last
    fixed, errors = rs41.rs_decode_np(bad, 99)
    assert errors == 2 and np.array_equal(fixed, word)


def test_errors_in_the_parity_are_corrected():
    words = _random_words(4, 9)
    bad = words.copy()
    bad[:, 231:243] ^= 0xFF
    fixed, errors = rs41.rs_decode_np(bad)
    assert np.array_equal(fixed, words) and errors.tolist() == [12] * 4


# ---------------------------------------------------------------------------------------------------------------- encode -> decode
@pytest.mark.parametrize("polarity", [0, 1])
@pytest.mark.parametrize("rate", RATES)
def test_round_trip(rate, polarity):
    """a standard frame in each hemisphere, an extended one, and one within a degree of the pole, a second apart"""
    fields = [T.NORTH, T.extended(T.SOUTH), T.POLAR, T.extended(T.POLAR, b"")]
    x = rs41.encode(fields, rate, polarity=polarity, start=77.3)
    found, info = decode_rs41.decode_audio_host(x, rate)
    assert len(found) == 4 and info["ok"] == 4 and info["followed"] == 0 and info["partial"] == 0
    for k, (f, want) in enumerate(zip(found, fields)):
        T.same_fields(f, want)
        assert f["status"] == "ok" and f["polarity"] == polarity and f["corrected"] == (0, 0) and f["header_errors"] == 0
        assert abs(f["start"] - rs41.frame_start(rate, k, 77.3)) <= rate / rs41.BAUD and abs(f["t"] * rate - f["start"]) < 1e-6
        assert all(b["crc_ok"] for b in f["blocks"]) and not f["followed"]
    assert [b["id"] for b in found[0]["blocks"]] == [0x79, 0x7A, 0x7C, 0x7D, 0x7B, 0x76]
    assert T.position_error(found[0], T.NORTH)[2] <= 2e-7 and T.position_error(found[1], T.SOUTH)[2] <= 2e-7    # the longitude itself


def test_twelve_byte_errors_per_codeword_are_ok():
    frame = T.damage(T.damage(rs41.build_frame(T.NORTH), 0, 12, 1), 1, 12, 2)
    found, info = decode_rs41.decode_audio_host(rs41.encode([frame], 48000.0, start=30.0), 48000.0)
    assert len(found) == 1 and found[0]["status"] == "ok" and found[0]["corrected"] == (12, 12)
    T.same_fields(found[0], T.NORTH)


def test_a_destroyed_codeword_leaves_a_partial_frame_with_its_position():
    frame = T.damage(rs41.build_frame(T.SOUTH), 1, 30, 3, inside=(0x39, 0x112))     # codeword 1, all of it in front of GPSPOS
    found, info = decode_rs41.decode_audio_host(rs41.encode([frame], 48000.0, start=30.0), 48000.0)
    assert len(found) == 1 and info["partial"] == 1
    f = found[0]
    assert f["status"] == "partial" and f["corrected"] == (0, -1) and all(b["crc_ok"] for b in f["blocks"])
    assert 0x7B in [b["id"] for b in f["blocks"]] and len(f["blocks"]) < 6
    assert T.within_bounds(f, T.SOUTH) and f["sats"] == T.SOUTH["sats"]
    for key in [k for k, b in (("frame_number", 0x79), ("gps_week", 0x7C), ("meas_raw", 0x7A)) if b not in [x["id"] for x in f["blocks"]]]:
        assert f[key] is None
    ruined = T.damage(T.damage(rs41.build_frame(T.SOUTH), 1, 100, 3), 0, 100, 4)  # nothing left: dropped
    found, info = decode_rs41.decode_audio_host(rs41.encode([ruined], 48000.0, start=30.0), 48000.0)
    assert found == [] and info["dropped"] == 1


@pytest.mark.parametrize("flip", [0x01, 0x0A, 0x0E, 0x10, 0xC0, 0xE0])
def test_a_damaged_type_byte_decodes(flip):
    for fields in (T.NORTH, T.extended(T.NORTH)):
        frame = rs41.build_frame(fields)
        frame[rs41.TYPE_AT] ^= flip
        found, _ = decode_rs41.decode_audio_host(rs41.encode([frame], 48000.0, start=12.5), 48000.0)
        assert len(found) == 1 and found[0]["status"] == "ok" and found[0]["corrected"] == (1, 0)
        T.same_fields(found[0], fields)


@pytest.mark.parametrize("polarity", [0, 1])
@pytest.mark.parametrize("slack", [0, 4, rs41.SLACK_MAX])
def test_header_slack(slack, polarity):
    for wrong, passes in ((slack, True), (slack + 1, False)):
        bits = np.concatenate((T.header_bits(wrong), T.frame_bits(rs41.build_frame(T.NORTH))[64:]))
        x = T.as_audio(T.rect(bits, 10, t=40, polarity=polarity))
        masks = rs41.masks_host(x, 10.0, 5, slack)
        assert masks[40] == ((3 if polarity else 1) if passes else 0)
        found, info = decode_rs41.decode_audio_host(x, 48000.0, slack=slack, follow=0)
        assert len(found) == (1 if passes else 0)
        if passes:
            assert found[0]["header_errors"] == wrong and found[0]["polarity"] == polarity and found[0]["status"] == "ok"
    with pytest.raises(ValueError):
        rs41.params(48000.0, None, rs41.SLACK_MAX + 1)
    for rate in (4800.0 * 3.9, 4800.0 * 64.1, 0.0, float("nan")):
        with pytest.raises(ValueError):
            rs41.params(rate)
    assert rs41.params(4800.0 * 4)[:2] == (4.0, 3) and rs41.params(4800.0 * 64)[:2] == (64.0, 39)


def test_follow_recovers_a_frame_whose_header_was_overwritten():
    rate = 48000.0
    fields = [dict(T.NORTH, frame_number=10 + k) for k in range(4)]
    x = rs41.encode(fields, rate, start=100.0)
    lost = [int(rs41.frame_start(rate, k, 100.0)) for k in (1, 2)]
    for at in lost:                                                  # twenty places of the header set to the other level
        for k in np.flatnonzero(T.header_bits(20) != T.header_bits(0)):
            x[at + 10 * k:at + 10 * (k + 1)] *= -1.0
    found, info = decode_rs41.decode_audio_host(x, rate, follow=2)
    assert [f["frame_number"] for f in found] == [10, 11, 12, 13] and info["followed"] == 2
    assert [f["followed"] for f in found] == [False, True, True, False] and found[1]["header_errors"] == 20
    assert 0 <= found[1]["start"] - found[0]["start"] - 48000 <= 10 and all(f["status"] == "ok" for f in found)   # from the centre
    found, info = decode_rs41.decode_audio_host(x, rate, follow=1)
    assert [f["frame_number"] for f in found] == [10, 11, 13] and info["followed"] == 1
    found, info = decode_rs41.decode_audio_host(x, rate, follow=0)
    assert [f["frame_number"] for f in found] == [10, 13] and info["followed"] == 0


@pytest.mark.parametrize("gap", [0.99994, 1.00006, 0.9999, 1.0001])
def test_a_second_that_is_not_round_rate_samples_gives_each_frame_once(gap):
    """the sonde's clock 60 and 100 ppm off the recorder's: the next header lies 3 or 5 samples off the prediction, inside the bit
    time the merge calls one frame, so nothing is asked for and nothing kept twice; and a lost header is still followed"""
    rate = 48000.0
    fields = [dict(T.NORTH, frame_number=10 + k) for k in range(4)]
    x = rs41.encode(fields, rate, gap=gap, start=100.0)
    found, info = decode_rs41.decode_audio_host(x, rate, follow=2)
    assert [f["frame_number"] for f in found] == [10, 11, 12, 13] and info["followed"] == 0 and info["frames"] == 4
    at = int(round(rs41.frame_start(rate, 2, 100.0, gap)))
    for k in np.flatnonzero(T.header_bits(20) != T.header_bits(0)):
        x[at + 10 * k:at + 10 * (k + 1)] *= -1.0
    found, info = decode_rs41.decode_audio_host(x, rate, follow=2)
    assert [f["frame_number"] for f in found] == [10, 11, 12, 13] and info["followed"] == 1
    assert [f["followed"] for f in found] == [False, False, True, False]


def test_calibration_is_assembled_over_51_frames():
    rate = 4800.0 * 4
    rng = np.random.default_rng(8)
    cal = rng.integers(0, 256, (51, 16)).astype(np.uint8)
    order = [(7 + k) % 51 for k in range(51)]
    fields = [dict(T.NORTH, frame_number=500 + k, subframe=s, calibration=bytes(cal[s])) for k, s in enumerate(order)]
    x = rs41.encode(fields, rate, gap=0.62, start=9.0)
    found, info = rs41.decode(x, rate, follow=0)[:2]
    assert info["ok"] == 51
    sondes = rs41.assemble(found)
    assert list(sondes) == ["S1234567"]
    s = sondes["S1234567"]
    assert s["seen"].all() and np.array_equal(s["calibration"], cal) and (s["first"], s["last"], s["frames"]) == (500, 550, 51)
    assert T.within_bounds(dict(zip(("lat", "lon", "alt"), s["position"])), T.NORTH)
    half = rs41.assemble(found[:20])["S1234567"]
    assert half["seen"].sum() == 20 and half["seen"][order[:20]].all() and not half["calibration"][~half["seen"]].any()
    pub = decode_rs41.sondes_host(decode_rs41.decode_audio_host(x[:int(0.6 * rate * 5)], rate, follow=0)[0])
    assert pub["S1234567"]["frames"] == 4 and pub["S1234567"]["seen"].sum() == 4


# ---------------------------------------------------------------------------------------------------------------- the slack bound
def test_slack_bound():
    """the header slid over alternating bits + header, by brute force, both phases and both polarities"""
    best = 64
    hdr = [int(c) for c in "0000100001101101010100111000100001000100011010010100100000011111"]
    for first in (0, 1):
        seq = [(first + i) & 1 for i in range(320)] + hdr
        for s in range(1, 321):
            d = sum(a != b for a, b in zip(seq[320 - s:384 - s], hdr))
            best = min(best, d, 64 - d)
    assert best == rs41.slide_distance() == rs41.HEADER_DISTANCE == 24
    assert rs41.SLACK_MAX == (best - 1) // 2 == 11                   # slack wrong places of its own still leave a slid header outside
