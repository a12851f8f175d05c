"""RDS on the host (directdemod_amd/rds.py): the code's facts, the burst repair, the parser, the clock, and the
NumPy restatement of the kernels decoding what the synthesiser sends.  No GPU."""
import numpy as np
import pytest

import _rds as T
import directdemod_amd
from directdemod_amd import decode_rds, rds

RATE = 171000.0


def as_group(words, k=0, third=None):
    """a parsed group as rds.decode makes it, from four words (None: not decoded)"""
    third = (1 if words[1] is not None and words[1] >> 11 & 1 else 0) if third is None else third
    pi, kind, tp, pty = rds.fields(words, third)
    return {"t": 0.0, "start": k, "pi": pi, "group": kind, "tp": tp, "pty": pty, "words": list(words), "repaired": 0, "followed": False,
            "third": third}


def without(words, *blocks):
    return [None if i in blocks else w for i, w in enumerate(words)]


# ---------------------------------------------------------------------------------------------------------------- the code
def test_exports():
    assert "rds" in directdemod_amd.__all__ and "decode_rds" in directdemod_amd.__all__


def test_the_generator_has_order_341():
    assert rds.x_power(341) == 1 and all(rds.x_power(e) != 1 for e in range(1, 341))
    assert [rds.x_power(e) for e in range(11)][-1] == rds.GEN ^ 0x400


def test_the_367_bursts_have_distinct_remainders():
    b = rds.bursts()
    assert len(b) == 367 and len({r for _, r, _, _ in b}) == 367 and all(r != 0 for _, r, _, _ in b)
    assert sorted({ln for _, _, ln, _ in b}) == [1, 2, 3, 4, 5] and all(e < 1 << 26 for e, _, _, _ in b)
    # the XOR of two offset words is itself a burst's remainder for every pair but A and C: blocks are typed by position
    rems = {r for _, r, _, _ in b}
    pairs = {(i, j): (rds.OFFSETS[i] ^ rds.OFFSETS[j]) in rems for i in range(5) for j in range(i + 1, 5)}
    assert [p for p, hit in pairs.items() if not hit] == [(rds.A, rds.CC)]


def test_checkword_of_zero_is_the_offset_word():
    for o in range(5):
        assert rds.checkword(0, o) == rds.OFFSETS[o] and rds.block(0, o) == rds.OFFSETS[o]
        assert int(rds.remainder(rds.block(0xD318, o))) == rds.OFFSETS[o]


def test_every_burst_is_repaired_for_every_offset():
    rng = np.random.default_rng(3)
    for o in range(5):
        info = int(rng.integers(0, 1 << 16))
        good = rds.block(info, o)
        assert rds.repair_np(good, o, 0) == (good, 0)
        for e, _, ln, ones in rds.bursts():
            assert rds.repair_np(good ^ e, o, ln) == (good, ones) and rds.repair_np(good ^ e, o, 5) == (good, ones)
            assert rds.repair_np(good ^ e, o, ln - 1) == (good ^ e, -1)


# ---------------------------------------------------------------------------------------------------------------- the parser
def test_parser_0a_and_0b():
    gs = [as_group(rds.group_0a(T.PI, T.PS, s, tp=1, pty=10, ta=1, ms=0, di=0b0110, af=T.AF[s]), s) for s in range(4)]
    st = rds.stations(gs)[T.PI]
    assert st["ps"] == T.PS and st["ps_complete"] and (st["tp"], st["pty"], st["ta"], st["ms"], st["di"]) == (1, 10, 1, 0, 0b0110)
    assert st["af"] == [88.5, 89.5, 90.5] and st["af_count"] == 3 and st["groups"] == {"0A": 4}
    assert [g["group"] for g in gs] == ["0A"] * 4
    gb = [as_group(rds.group_0a(0x1234, "ABCDEFGH", s, version="B"), s) for s in (0, 2)]
    assert gb[0]["group"] == "0B" and gb[0]["third"] == 1
    st = rds.stations(gb)[0x1234]
    assert st["ps"] == "AB  EF  " and not st["ps_complete"] and st["af"] == [] and st["di"] is None
    # a version B group whose first block is lost still has its PI, in the third
    lost = as_group(without(rds.group_0a(0x1234, "ABCDEFGH", 1, version="B"), 0), 9)
    assert lost["pi"] == 0x1234 and as_group(without(rds.group_0a(0x1234, "ABCDEFGH", 1), 0), 9)["pi"] is None


def test_parser_2a_and_2b():
    text = "A text of forty characters, just so.....\r"
    gs = [as_group(rds.group_2a(T.PI, text, s), s) for s in range(11)]
    assert rds.stations(gs)[T.PI]["radiotext"] == text[:-1] and gs[0]["group"] == "2A"
    gb = [as_group(rds.group_2a(T.PI, "Short one\r", s, version="B"), s) for s in range(5)]
    assert rds.stations(gb)[T.PI]["radiotext"] == "Short one" and gb[0]["group"] == "2B"
    assert rds.char(0x41) == "A" and rds.char(0x7F) == "�" and rds.char(0x19) == "�" and rds.char(0xE9) == "�"


def test_radiotext_with_a_toggle_and_missing_segments():
    first = [as_group(rds.group_2a(T.PI, "OLD TEXT HERE...", s, flag=0), s) for s in range(4)]
    second = [as_group(rds.group_2a(T.PI, "NEW!", 0, flag=1), 4)]
    assert rds.stations(first)[T.PI]["radiotext"] == "OLD TEXT HERE..."
    assert rds.stations(first + second)[T.PI]["radiotext"] == "NEW!"         # the flag cleared the old text
    gaps = [as_group(rds.group_2a(T.PI, "0123456789ABCDEF\r", s), s) for s in (0, 2, 3, 4)]
    gaps[1] = as_group(without(gaps[1]["words"], 3), 2)                      # segment 2 without its second half
    assert rds.stations(gaps)[T.PI]["radiotext"] == "0123    89  CDEF"
    ps = [as_group(without(rds.group_0a(T.PI, T.PS, 0), 3), 0), as_group(rds.group_0a(T.PI, T.PS, 3), 1)]
    st = rds.stations(ps)[T.PI]
    assert st["ps"] == "      1 " and not st["ps_complete"] and st["groups"] == {"0A": 2}


def test_clock():
    assert rds.mjd_date(51544) == (2000, 1, 1) and rds.mjd_date(58849) == (2020, 1, 1) and rds.mjd_date(60000) == (2023, 2, 25)
    assert rds.mjd_date(59274) == (2021, 3, 1) and rds.mjd_date(59273) == (2021, 2, 28) and rds.mjd_date(58908) == (2020, 2, 29)
    for hour, offset in ((13, 2), (17, -3), (0, 0), (23, -24), (16, 31), (15, -31)):
        w = rds.group_4a(T.PI, 60000, hour, 59, offset)
        assert (w[2] & 1, w[3] >> 12) == (hour >> 4, hour & 15)              # the hour's top bit ends block 3, the rest begins block 4
        st = rds.stations([as_group(w)])[T.PI]
        assert st["clock"] == ("2023-02-25T%02d:59:00Z" % hour, offset) and st["groups"] == {"4A": 1}
    assert rds.clock_of(*rds.group_4a(T.PI, 131071, 23, 0)[1:])["mjd"] == 131071     # the day's 17 bits across blocks 2 and 3
    assert rds.stations([as_group(without(rds.group_4a(T.PI, 60000, 1, 2), 2))])[T.PI]["clock"] is None


def test_af_codes():
    assert rds.af_of(1) == ("freq", 87.6) and rds.af_of(204) == ("freq", 107.9) and rds.af_of(125) == ("freq", 100.0)
    assert rds.af_of(225) == ("count", 1) and rds.af_of(249) == ("count", 25)
    assert rds.af_of(0) is None and rds.af_of(rds.FILLER) is None and rds.af_of(224) is None and rds.af_of(250) is None


def test_rates_and_options():
    assert rds.params(171000.0)[:2] == (9, 16.0) and rds.params(240000.0)[0] == 12 and rds.params(384000.0)[0] == 20
    assert abs(rds.params(240000.0)[1] - 16.8421) < 1e-4 and rds.params(240000.0)[2] == int(round(57000 * 2.0 ** 32 / 240000))
    for bad in (0, -1, 124999.0, 500001.0, float("nan")):
        with pytest.raises(ValueError):
            rds.params(bad)
    for kw in (dict(clean=1), dict(clean=5), dict(fix=-1), dict(fix=6), dict(follow=-1), dict(follow=1.5)):
        with pytest.raises(ValueError):
            decode_rds.decode_rds.fromAudio(np.zeros(10), RATE, **kw)
    assert [rds.window_taps(fs) for fs in (2400000, 1200000, 2048000, 240000)] == [37, 19, 31, 5]


# ---------------------------------------------------------------------------------------------------------------- the restatement
def sent(found):
    return [tuple(g["words"]) for g in found]


@pytest.mark.parametrize("clock_ppm", [0.0, 100.0, -100.0])
@pytest.mark.parametrize("phase", [0.0, np.pi / 2.0])
def test_every_group_is_decoded(clock_ppm, phase):
    found, info = decode_rds.decode_audio_host(T.multiplex(RATE, clock_ppm, phase), RATE)
    assert sent(found) == T.station_groups() and info["groups"] == 7 and info["followed"] == 0 and info["dropped"] == 0
    assert all(g["repaired"] == 0 and not g["followed"] and g["pi"] == T.PI for g in found)
    T.same_station(decode_rds.stations_host(found)[T.PI])
    assert rds.text_lines(rds.decode(T.multiplex(RATE, clock_ppm, phase), RATE)[0]) == [
        "RDS D318 PS: 'RADIO 1 ' RT: 'Hi RDS' CT: 2023-02-25T13:37:00Z +1.0 h"]
    d, sps, _ = rds.params(RATE)
    starts = np.array([g["start"] for g in found], dtype=np.float64)
    period = rds.BITS * sps * (1.0 - clock_ppm * 1e-6)
    assert np.all(np.abs(np.diff(starts) - period) <= 2.0)


def test_other_rates():
    for rate in (240000.0, 250000.0, 384000.0):
        found, _ = decode_rds.decode_audio_host(T.multiplex(rate, 60.0, 1.0), rate)
        assert sent(found) == T.station_groups()


def test_a_stream_that_starts_inside_a_group():
    x = T.multiplex(RATE)
    cut = int((0.01 + 0.4 * rds.BITS / rds.BITRATE) * RATE)
    found, _ = decode_rds.decode_audio_host(x[cut:], RATE)
    assert sent(found) == T.station_groups()[1:]
    assert decode_rds.decode_audio_host(x[:cut], RATE)[0] == [] and decode_rds.decode_audio_host(np.zeros(0), RATE)[0] == []


def test_follow_across_a_group_with_two_blocks_destroyed():
    bits = rds.air_bits(T.station_groups())
    rng = np.random.default_rng(11)
    for blk in (0, 3):                                                   # group 3 (the 4A): blocks 1 and 4 replaced by noise
        at = 3 * rds.BITS + 26 * blk
        bits[at:at + 26] = rng.integers(0, 2, 26)
    x = rds.encode_mpx(bits, RATE, start=0.01)
    for follow, count in ((2, 7), (0, 6)):
        found, info = decode_rds.decode_audio_host(x, RATE, follow=follow)
        assert len(found) == count and info["followed"] == (1 if follow else 0)
    found, _ = decode_rds.decode_audio_host(x, RATE)
    want = T.station_groups()
    assert [g["followed"] for g in found] == [k == 3 for k in range(7)]
    assert found[3]["words"] == [None, want[3][1], want[3][2], None] and found[3]["pi"] is None and found[3]["group"] == "4A"
    assert sent(found[:3] + found[4:]) == want[:3] + want[4:]
    st = decode_rds.stations_host(found)                                 # the group without a PI goes to the station before it
    assert list(st) == [T.PI] and st[T.PI]["groups"] == {"0A": 4, "2A": 2, "4A": 1} and st[T.PI]["clock"] is None
    assert st[T.PI]["ps"] == T.PS and st[T.PI]["radiotext"] == "Hi RDS"


def test_noise_gives_candidates_and_no_group():
    """A minute of Gaussian noise at the decimated rate: at clean = 2 a start passes by chance with probability 9 * 2^-20 (six
    pairs of blocks at 2^-10 each, those with the third block twice), some ten of 1 140 000; none is chained or clean in all four
    blocks, so none is accepted (DESIGN.md section 4.27 has the arithmetic).  A condition on the rule, checked here once: seed 1."""
    d, sps, _ = rds.params(RATE)
    m = int(60 * RATE / d)
    b = np.rint(np.random.default_rng(1).normal(0.0, 20000.0, (m, 2))).astype(np.int32)
    found, info, det = rds.decode_baseband(b, m, RATE, clean=2)
    print("candidates on noise:", info["candidates"])
    assert 1 <= info["candidates"] <= 30 and info["dropped"] == info["candidates"] - info["duplicates"]
    assert found == [] and info["groups"] == 0 and info["followed"] == 0
    assert (det["status"] == 0).sum(axis=1).max() < 4
