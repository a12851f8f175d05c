"""The host side of the ACARS decoder (directdemod_amd/acars.py, decode_acars.decode_host): the block check sequence, the framing
characters, the parity-guided repair over every small error pattern of a short block, the template against a block's own pre-key,
and the NumPy restatement of the whole decoder over synthesised recordings.  No GPU."""
import itertools

import numpy as np
import pytest

import _acars as T
from directdemod_amd import acars, decode_acars, source


# ---------------------------------------------------------------------------------------------------------------- the block check
def test_crc_known_answer():
    assert acars.crc_bitwise(b"123456789") == 0x2189 == acars.residual(b"123456789")                # CRC-16/KERMIT
    for blk in (T.SHORT, T.text_block(220)):
        assert acars.crc_bitwise(blk[:-1]) == 0 == acars.residual(blk[:-1]) and blk[-1] == acars.DEL


def test_ztable_is_the_bitwise_register():
    rng = np.random.default_rng(3)
    for size in (1, 2, 15, 16, 17, 239, 240):
        data = bytes(rng.integers(0, 256, size).tolist())
        assert acars.residual(data) == acars.crc_bitwise(data)
    for m in (0, 1, 15, 16, 1000, acars.BLOCK_BITS - 1):                                             # a lone bit, m zero bits behind it
        n = m + 1
        lone = np.zeros(-(-n // 8) * 8, dtype=np.uint8)
        lone[len(lone) - n] = 1
        assert acars.ZTABLE[m] == acars.crc_bitwise(np.packbits(lone, bitorder="little").tobytes())
    assert len(set(acars.ZTABLE.tolist())) == acars.BLOCK_BITS                                       # distinct: one hit at most
    with pytest.raises(ValueError):
        acars.residual(bytes(241))


def test_framing_characters_and_template():
    assert acars.odd([0x2B, 0x2A, 0x16, 0x01, 0x03, 0x17, 0x7F]).tolist() == [0xAB, 0x2A, 0x16, 0x01, 0x83, 0x97, 0x7F]
    assert (acars.PLUS, acars.STAR, acars.SYN, acars.SOH, acars.ETX, acars.ETB, acars.DEL) == (0xAB, 0x2A, 0x16, 0x01, 0x83, 0x97, 0x7F)
    bits = acars.block_bits(T.SHORT, prekey=3)
    assert bits[:24].all() and np.packbits(bits[24:32], bitorder="little")[0] == 0xAB
    assert int("".join(map(str, bits[32:64])), 2) == acars.TEMPLATE == 0x54686880
    assert np.packbits(bits[64:], bitorder="little").tobytes() == T.SHORT
    assert not acars.flagged(np.frombuffer(T.SHORT[:13], dtype=np.uint8)).any()                      # odd parity through ETX
    assert T.SHORT[12] == acars.ETX and T.text_block(0, more=True)[13] == acars.ETB and len(T.text_block(220)) == 237


def test_quantiser():
    x = np.array([0.0, T.UNIT, -3 * T.UNIT, 0.5 * T.UNIT, 1.5 * T.UNIT, 512.0, -512.0, 512.0 + T.UNIT, np.nan, np.inf, -np.inf, 1e300])
    assert acars.quantise(x).tolist() == [0, 1, -3, 0, 2, 1 << 21, -(1 << 21), 0, 0, 0, 0, 0]
    assert 181 * 4096 < 1 << 20                                      # a u8 recording's envelope: |(127.5, 127.5)| < 181


# ---------------------------------------------------------------------------------------------------------------- repair, exhaustively
BODY = list(range(96))                                               # the bits of bytes 0 .. 11 of the short block
BCS = list(range(104, 120))                                          # bytes 13 and 14; bits 96 .. 103 are ETX


def test_every_single_error_is_restored():
    whole = T.received()
    assert acars.judge(whole, 0)[1:] == (acars.OK, 12, 0, 0, 1, 0)
    for p in BODY + BCS:
        fixed, status, e, c, nfix, closed, s = acars.judge(T.received(flips=[p]), 1)
        assert (status, e, c, nfix, closed) == (acars.OK, 12, int(p < 96), 1, 1) and s != 0 and np.array_equal(fixed, whole)
        assert acars.judge(T.received(flips=[p]), 0)[1] == acars.BAD_BCS                             # fix below the need
    for p in range(96, 104):                                         # an error in the ETX byte: the end is not found
        assert acars.judge(T.received(flips=[p]), 2)[1:3] == (acars.NO_END, -1)


def test_every_pair_in_two_characters_is_restored():
    whole = T.received()
    for a, b in itertools.combinations(range(12), 2):
        for i in range(8):
            for j in range(8):
                got = T.received(flips=[8 * a + i, 8 * b + j])
                fixed, status, e, c, nfix, _, _ = acars.judge(got, 2)
                assert (status, c, nfix) == (acars.OK, 2, 2) and np.array_equal(fixed, whole)
    assert acars.judge(T.received(flips=[5, 77]), 1)[1] == acars.BAD_BCS                             # fix below the need


def test_parity_invisible_and_triple_errors_are_refused():
    """None of these passes, and none can at this length.  A wrong block passes when its errors and the bits the repair flips
    together make a codeword of the block check.  The generator x^16 + x^12 + x^5 + 1 has the factor x + 1, so every codeword has
    an even number of ones: two errors in one character (no parity flag) plus one block check bit are three; three errors in three
    characters are refused for their three flags; three errors in two characters (two flags) plus a pair are five; two errors in
    one character and one in another (one flag) plus one bit are four -- and the block check has no codeword of four ones within
    the short block's 120 bits (the pairs test above relies on the same fact: no second pair fits).  In a long block it has some
    (T.twin_pairs finds one), which is what the miscorrection note of INTEGRATION.md is about."""
    passed = 0
    for a in range(12):
        for i, j in itertools.combinations(range(8), 2):
            two = [8 * a + i, 8 * a + j]
            fixed, status, e, c, nfix, _, _ = acars.judge(T.received(flips=two), 2)
            assert c == 0
            passed += status == acars.OK
            for p in BODY[:8 * a] + BODY[8 * a + 8:] + BCS:                                          # and a third somewhere else
                passed += acars.judge(T.received(flips=two + [p]), 2)[1] == acars.OK
    for p, r in itertools.product(BODY, BCS):                        # one in the body, one in the block check: one flag, no one bit fits
        passed += acars.judge(T.received(flips=[p, r]), 2)[1] == acars.OK
    for k, three in enumerate(itertools.combinations(BODY + BCS, 3)):
        if k % 23 == 0:                                              # a sample of all triples
            passed += acars.judge(T.received(flips=three), 2)[1] == acars.OK
    assert passed == 0


def test_two_hits_in_the_pair_search_are_refused():
    f1, i, f2, j, i2, j2 = T.twin_pairs()
    assert f1 != f2 and (i, j) != (i2, j2)
    blk = T.block_ending_at(236)
    assert acars.find_end(T.received(blk)) == 236
    got = T.received(blk, flips=[8 * f1 + i, 8 * f2 + j])
    fixed, status, e, c, nfix, _, _ = acars.judge(got, 2)
    assert (status, e, c, nfix) == (acars.BAD_BCS, 236, 2, 0) and np.array_equal(fixed, got)
    other = T.received(blk, flips=[8 * f1 + i, 8 * f2 + (j + 1) % 8])                                # a pair without a twin is repaired
    if acars.judge(other, 2)[1] == acars.OK:
        assert np.array_equal(acars.judge(other, 2)[0], T.received(blk))


def test_ends():
    for chars, e in ((None, 12), (0, 13), (1, 14), (220, 233)):
        for more in (False, True):
            blk = T.text_block(chars, more)
            fixed, status, end, c, nfix, closed, s = acars.judge(T.received(blk), 2)
            assert (status, end, c, nfix, closed, s) == (acars.OK, e, 0, 0, 1, 0) and blk[e] == (acars.ETB if more else acars.ETX)
    for e in (236, 237, 238):                                        # the end pushed back by filler characters: 238 has no room
        d = T.received(T.block_ending_at(e))
        status, end, closed = acars.judge(d, 2)[1], acars.judge(d, 2)[2], acars.judge(d, 2)[5]
        assert (status, end, closed) == {236: (acars.OK, 236, 1), 237: (acars.OK, 237, 0), 238: (acars.NO_END, -1, 0)}[e]
    early = T.received(T.text_block(5))
    early[3] = acars.ETX                                             # before byte 12 an ETX is no end
    assert acars.judge(early, 0)[2] == 18


# ---------------------------------------------------------------------------------------------------------------- the template
@pytest.mark.parametrize("sps", [8.0, 10.5, 20.0])
def test_template_against_its_own_prekey(sps):
    """On clean synthesised audio, at every start from the carrier's rise to one bit time before the template's true start, at
    ten fractional offsets and every window the samples per bit allow, the 32 decisions stay 6 or more places from the template and
    from its inverse (8 or more up to w = 0.7 sps: the windows of w near sps reach across the neighbouring bits): slack is capped
    at 5.  At whole-bit steps it is 10 or more."""
    k = np.arange(32)
    bits = acars.block_bits(T.SHORT)
    slid = [int((bits[a:a + 32] != acars.TEMPLATE_BITS).sum()) for a in range(8 * (acars.PREKEY + 1))]
    assert min(min(d, 32 - d) for d in slid) >= 10
    least = {}
    for w in range(1, min(acars.W_MAX, int(sps)) + 1):
        for frac in np.arange(10) / 10.0:
            x = acars.encode_audio([T.SHORT], sps * 2400.0, [40.0 + frac])
            true = acars.block_start(sps * 2400.0, 40.0 + frac)
            ts = np.arange(0, int(np.floor(true - sps)) + 1)
            mis = ((acars.values(acars.quantise(x), ts, k, sps, w) > 0) != acars.TEMPLATE_BITS).sum(axis=1)
            least[w] = min(least.get(w, 32), int(np.minimum(mis, 32 - mis).min()))
            hit = int(np.floor(true + 0.25 * sps))                   # a quarter bit late still reads the template
            assert w > sps / 2 or ((acars.values(acars.quantise(x), [hit], k, sps, w)[0] > 0) == acars.TEMPLATE_BITS).all()
    assert min(least.values()) == 6 == acars.SLACK_MAX + 1
    assert all(v >= 8 for w, v in least.items() if w <= 0.7 * sps)
    with pytest.raises(ValueError):
        acars.params(48000.0, None, acars.SLACK_MAX + 1)


# ---------------------------------------------------------------------------------------------------------------- round trips
@pytest.fixture(scope="module")
def host_decode():
    return decode_acars.decode_host(np.array(T.recording()), T.FS, T.OFFSETS)


def test_round_trip_two_channels_both_polarities(host_decode):
    found, info, msgs = host_decode
    assert [(b["channel"], b["bytes"]) for b in found] == T.expected()
    assert all(b["corrected"] == 0 and b["parity_errors"] == 0 and b["closed"] for b in found)
    assert [b["polarity"] for b in found] == [0 if b["channel"] == "A" else 1 for b in found]
    blks, _, starts, _ = T.blocks()
    for b, s in zip(found, sorted(starts)):                          # the template starts 17 characters behind the block's start
        assert abs(b["t"] - (s + 8 * 17 / 2400.0)) < 1.5 / 2400.0
    a = [b for b in found if b["channel"] == "A"]
    assert [(b["mode"], b["address"], b["ack"], b["label"], b["block_id"], b["downlink"], b["text"], b["more"]) for b in a] == [
        ("2", "G-ABCD", None, "Q0", "1", True, "", False), ("2", "N123AB", "A", "_.", "S", False, "x", False),
        ("E", "OH-LVA", None, "H1", "7", True, T.LONG_TEXT, False)]
    assert a[0]["msgno"] is None and a[2]["msgno"] == T.LONG_TEXT[:4] and a[2]["flight"] == T.LONG_TEXT[4:10]
    assert a[1]["bytes"][10] == 0x7F                                 # the raw bytes keep what the text shows as a dot
    per = info["channels"]
    assert info["blocks"] == 6 and per["A"]["accepted"] == 3 == per["B"]["accepted"]
    assert all(p["clean"] == p["accepted"] + p["duplicates"] and p["duplicates"] > 0 and p["outside"] == 0 for p in per.values())
    assert all(acars.line(b).startswith("ACARS %s: Mode: " % b["channel"]) for b in found)


def test_reassembly(host_decode):
    found, _, msgs = host_decode
    chain = [m for m in msgs if m["channel"] == "B"]
    assert len(msgs) == 4 and len(chain) == 1
    assert chain[0]["text"] == "".join(T.CHAIN) + "".join(T.CHAIN_TEXT) and chain[0]["blocks"] == 3 and chain[0]["complete"]
    assert (chain[0]["address"], chain[0]["msgno"], chain[0]["flight"]) == ("G-EUPJ",) + T.CHAIN
    b = [dict(x) for x in found if x["channel"] == "B"]
    assert [x["more"] for x in b] == [True, True, False]
    assert len(acars.messages(b[:2])) == 1 and not acars.messages(b[:2])[0]["complete"]
    assert len(acars.messages([b[0], b[2]])) == 2                    # the block letters must be consecutive
    late = dict(b[1], t=b[0]["t"] + 30.5)
    assert len(acars.messages([b[0], late])) == 2                    # and each block within 30 s of the one before
    assert len(acars.messages([b[0], dict(b[1], address="G-EUPK")])) == 2
    assert len(acars.messages([b[0], dict(b[1], msgno="M08B")])) == 2
    assert len(acars.messages([dict(b[0], more=False), b[1]])) == 2  # ETX closes a message


def test_a_block_cut_by_the_end_of_the_recording():
    rate = 48000.0
    x = acars.encode_audio([T.text_block(40)], rate, [300.5], sigma=0.5, seed=2)
    t = int(acars.block_start(rate, 300.5))
    whole, _, _ = decode_acars.decode_audio_host(x, rate)
    assert len(whole) == 1 and abs(whole[0]["start"] - t) <= 10
    for n in (t + 20 * 8 * 20, t + 33 * 20, t + 31 * 20, t - 5):      # inside the text, behind the template, inside it, before it
        found, info, _ = decode_acars.decode_audio_host(x[:n], rate)
        assert found == [] and info["channels"]["A"]["accepted"] == 0
    det = acars.blocks_host(x[:t + 20 * 8 * 20], 20.0, 10, 2, [t, t + 20 * 8 * 20, -1])
    assert det["status"].tolist() == [acars.NO_END, acars.OUTSIDE, acars.OUTSIDE] and not det["bytes"][1:].any()


def test_repairs_through_the_audio():
    rate = 48000.0
    blks = [T.text_block(30)] * 4
    flips = [None, {5: 0x10}, {15: 0x01, 40: 0x80}, {44: 0x04}]      # clean, one character, two characters, the block check
    x = acars.encode_audio(blks, rate, [200.0, 12200.3, 24200.6, 36200.9], sigma=0.5, seed=5, flips=flips)
    for fix, want in ((2, 4), (1, 3), (0, 1)):
        found, info, _ = decode_acars.decode_audio_host(x, rate, fix=fix)
        assert len(found) == want and all(b["bytes"] == blks[0][:-1] for b in found)
        per = info["channels"]["A"]
        assert (per["one_character"] > 0) == (fix >= 1) and (per["bcs"] > 0) == (fix >= 1) and (per["two_characters"] > 0) == (fix >= 2)
    found, _, _ = decode_acars.decode_audio_host(x, rate)
    assert [(b["corrected"], b["parity_errors"]) for b in found] == [(0, 0), (1, 1), (2, 2), (1, 0)]


def test_noise_only():
    """2^20 samples of a Gaussian envelope at 20 samples per bit and the widest slack: some hundred starts pass the sync test (a
    share of 2 x 242 825 / 2^32 of random words lies within five places of the template or its inverse), none is a block"""
    x = np.random.default_rng(20).normal(40.0, 10.0, 1 << 20)
    found, info, _ = decode_acars.decode_audio_host(x, 48000.0, slack=acars.SLACK_MAX)
    per = info["channels"]["A"]
    assert found == [] and per["accepted"] == 0 and per["candidates"] > 20
    assert per["candidates"] == per["no_end"] + per["bad_bcs"]


# ---------------------------------------------------------------------------------------------------------------- the errors
def test_value_errors():
    for rate in (19199.0, 153601.0, float("nan"), 0.0):
        with pytest.raises(ValueError):
            acars.params(rate)
    assert acars.params(19200.0)[:2] == (8.0, 4) and acars.params(153600.0)[:2] == (64.0, 32) and acars.params(25200.0)[1] == 5
    for kw in ({"w": 0}, {"w": 33}, {"w": 2.5}, {"slack": -1}, {"slack": 6}, {"fix": 3}, {"fix": -1}):
        with pytest.raises(ValueError):
            acars.params(48000.0, **kw)
    for kw in ({"slack": 6}, {"fix": 3}):
        with pytest.raises(ValueError):
            decode_acars.decode_acars.fromAudio(np.zeros(10), 48000.0, **kw)
        with pytest.raises(ValueError):
            decode_acars.decode_acars(source.IQarray(np.zeros((1000, 2), np.uint8), 240000), (0.0,), **kw)
    raw = source.IQarray(np.zeros((1000, 2), np.uint8), 2400000)
    with pytest.raises(ValueError, match="16000.*2400000|2400000.*16000"):
        decode_acars.decode_acars(raw, (0.0,), bw=16000)             # 16 kS/s: 6.67 samples per bit
    with pytest.raises(ValueError):
        decode_acars.decode_acars(raw, (0.0,), bw=200000)            # 200 kS/s: 83 samples per bit
    with pytest.raises(ValueError):
        decode_acars.decode_acars(raw, (0.0,), cut=30000.0)
    with pytest.raises(ValueError):
        decode_acars.decode_acars.fromAudio(np.zeros(10), 8000.0)
    assert decode_acars.decode_acars(raw, (1000.0, 26000.0)).audioRate == 48000.0
    for bad in (("22", "N1", None, "H1", "1"), ("2", "TOOLONG8", None, "H1", "1"), ("2", "N1", None, "H", "1"), ("2", "N1", "AB", "H1", "1")):
        with pytest.raises(ValueError):
            acars.block_bytes(*bad)
    with pytest.raises(ValueError):
        acars.block_bytes("2", "N1", None, "H1", "1", "x" * 221)
    with pytest.raises(ValueError):
        acars.encode_audio([T.SHORT], 48000.0, [1.0, 2.0])


def test_registered():
    import directdemod_amd
    assert "acars" in directdemod_amd.__all__ and "decode_acars" in directdemod_amd.__all__
