"""ADS-B on the CPU: the published frames against their published decodes, the CRC table, one-bit repair, the acceptance and
duplicate rules, the synthesiser, the restatement's decode rate on synthesised recordings, and the C entries' argument checks
(the library is needed, a GPU is not)."""
import ctypes as C
import math

import numpy as np
import pytest

import _adsb as A
from directdemod_amd import adsb, decode_adsb


# ---------------------------------------------------------------------------------------------------------------- known answers
def test_every_published_frame_has_remainder_zero():
    for f in A.FRAMES:
        assert adsb.crc(f) == 0
    assert adsb.crc(A.flip(A.F_CALLSIGN, 17)) != 0


def test_callsign():
    f = adsb.parse(A.F_CALLSIGN)
    assert (f["df"], f["icao"], f["tc"], f["callsign"]) == (17, 0x4840D6, 4, "KLM1023_")


def test_altitude_and_both_cpr_results():
    even, odd = adsb.parse(A.F_EVEN), adsb.parse(A.F_ODD)
    assert (even["tc"], even["cpr_f"], odd["cpr_f"], even["alt"], even["alt_q"], odd["alt"]) == (11, 0, 1, 38000, 1, 38000)
    assert (even["cpr_lat"], even["cpr_lon"], odd["cpr_lat"], odd["cpr_lon"]) == (93000, 51372, 74158, 50194)
    assert adsb.cpr_global(even, odd, 0) == (52.2572021484375, 3.91937255859375)
    lat_e, lat_o = adsb.cpr_latitudes(even, odd)
    assert (lat_e, lat_o) == (52.2572021484375, 52.26578017412606) and adsb.NL(lat_e) == adsb.NL(lat_o) == 36
    assert adsb.cpr_global(even, odd, 1)[0] == 52.26578017412606
    assert adsb.cpr_local((52.25, 3.9), even) == (52.2572021484375, 3.91937255859375)
    assert adsb.cpr_local((52.3, 4.0), odd)[0] == 52.26578017412606


def test_velocity():
    f = adsb.parse(A.F_VELOCITY)
    assert (f["tc"], f["subtype"], f["vr"]) == (19, 1, -832)
    assert abs(f["gs"] - 159.20) < 0.005 and abs(f["track"] - 182.88) < 0.005
    g = adsb.parse(A.F_AIRSPEED)
    assert (g["tc"], g["subtype"], g["airspeed"], g["airspeed_type"], g["vr"]) == (19, 3, 375, "TAS", -2304)
    assert g["heading"] == 243.984375


def test_second_pair_and_short_frame():
    even, odd = adsb.parse(A.F_EVEN2), adsb.parse(A.F_ODD2)
    assert (even["cpr_f"], odd["cpr_f"], even["alt"]) == (0, 1, 39000)
    lat, lon = adsb.cpr_global(even, odd, 1)
    assert abs(lat - 49.81755) < 1e-5 and abs(lon - 6.08442) < 1e-5
    f = adsb.parse(A.F_DF11)
    assert (f["df"], f["icao"], f["tc"]) == (11, 0x4840D6, None)
    assert adsb.parse("02E197B00179C3") == {"df": 0, "icao": None, "tc": None}          # everything else is left raw


def test_altitude_without_the_q_bit_is_left_out():
    b = adsb.bits_of(A.F_EVEN).copy()
    b[32 + 15] = 0                                                   # the Q bit: ME bit 15
    assert adsb.parse(np.packbits(b).tobytes())["alt"] is None


def test_NL():
    assert adsb.NL(0) == 59 and adsb.NL(87) == adsb.NL(-87) == 2 and adsb.NL(87.0001) == adsb.NL(-89.9) == adsb.NL(90) == 1
    assert adsb.NL(86.9) == 2 and adsb.NL(-86.9) == 2 and adsb.NL(86.5) == 3          # (86.53536998: 3 -> 2)
    # two transitions of the published table: 10.47047130 (59 -> 58) and 59.95459277 (30 -> 29)
    assert (adsb.NL(10.4704), adsb.NL(10.4705), adsb.NL(-10.4704), adsb.NL(-10.4705)) == (59, 58, 59, 58)
    assert (adsb.NL(59.9545), adsb.NL(59.9547)) == (30, 29)
    assert [adsb.NL(v) for v in (52.2572021484375, 52.26578017412606)] == [36, 36]


# ---------------------------------------------------------------------------------------------------------------- CRC and repair
def _long_division(bits):
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
        if v & (1 << 24):
            v ^= adsb.GENERATOR
    return v


def test_table_against_long_division():
    for i in range(112):
        lone = np.zeros(112, dtype=np.uint8)
        lone[i] = 1
        assert adsb.TABLE[i] == _long_division(lone)
        if i >= 56:
            assert adsb.TABLE[i] == _long_division(lone[56:])
    assert len(set(adsb.TABLE.tolist())) == 112 and 0 not in adsb.TABLE
    for f in A.FRAMES + [A.flip(A.F_ODD, 3, 77)]:
        assert adsb.crc(f) == _long_division(adsb.bits_of(f))


@pytest.fixture(scope="module")
def bit_errors():
    """the restatement over a recording of the 112 one-bit errors of one DF 17 frame, and over twenty seeded two-bit errors"""
    rate, Q = 2400000, 4
    raw, ks = A.slots([A.flip(A.F_CALLSIGN, p) for p in range(112)], rate, Q)
    one = adsb.demod_host(adsb.power(raw), rate, Q, ks)
    pairs = A.double_errors()
    raw, ks = A.slots([A.flip(A.F_CALLSIGN, *p) for p in pairs], rate, Q)
    return one, pairs, adsb.demod_host(adsb.power(raw), rate, Q, ks)


def test_every_single_bit_error_is_repaired_from_position_5(bit_errors):
    one, _, _ = bit_errors
    assert np.array_equal(one["fixed"][5:], np.arange(5, 112)) and np.all(one["fixed"][:5] == -1)
    assert np.array_equal(one["rem"][1:], adsb.TABLE[1:]) and one["L"][0] == 56     # (without bit 0 the format is 1: a short word)
    assert all(bytes(f).hex().upper() == A.F_CALLSIGN for f in one["frames"][5:])
    for p in range(5):                                               # the format bits are not repaired: the word stays as received
        assert bytes(one["frames"][p][:one["L"][p] // 8]) == A.flip(A.F_CALLSIGN, p)[:one["L"][p] // 8]


def test_double_errors_are_not_repaired(bit_errors):
    _, pairs, two = bit_errors
    assert np.all(two["fixed"] == -1) and np.all(two["rem"] != 0)
    for i, p in enumerate(pairs):
        if min(p) >= 5:
            assert bytes(two["frames"][i]) == A.flip(A.F_CALLSIGN, *p)
    # no two lone bits' remainders add up to a third's: a two-bit error never looks like a one-bit error
    t = adsb.TABLE
    assert not np.isin((t.reshape(-1, 1) ^ t.reshape(1, -1))[np.triu_indices(112, 1)], t).any()


# ---------------------------------------------------------------------------------------------------------------- acceptance
def _det(rows):
    """detections from (k, frame bytes, score): the fields demod_host would give, `fixed` from an optional fourth entry"""
    det = adsb._empty_det(len(rows))
    for i, row in enumerate(rows):
        raw = adsb.as_bytes(row[1])
        det["k"][i], det["score"][i] = row[0], row[2]
        det["frames"][i, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        det["L"][i], det["df"][i] = 8 * len(raw), raw[0] >> 3
        det["fixed"][i] = row[3] if len(row) > 3 else -1
        word = A.flip(raw, row[3]) if len(row) > 3 else raw          # (rem belongs to the word as received)
        det["rem"][i] = adsb.crc(word)
    return det


RATE, Q = 2400000, 4


def _overlaid(head, address):
    """a 56-bit frame of the four bytes `head` whose parity field is the remainder overlaid with the address"""
    parity = adsb.crc(head + bytes(3)) ^ address
    return head + parity.to_bytes(3, "big")


AP_FRAME = _overlaid(bytes([0x20, 0x00, 0x05, 0x10]), 0x4840D6)     # DF 4


def test_a_repaired_frame_needs_a_known_address():
    lone = _det([(100, A.F_VELOCITY, 50, 40)])
    assert adsb.accept(lone, RATE, Q)[0] == []
    both = _det([(100, A.F_VELOCITY, 50, 40), (90000, A.F_VELOCITY, 60)])
    msgs, counts = adsb.accept(both, RATE, Q)
    assert [(m["k"], m["fixed"], m["icao"]) for m in msgs] == [(100, 40, 0x485020), (90000, -1, 0x485020)]
    assert counts == {"clean": 1, "repaired": 1, "address_parity": 0, "duplicates": 0}
    assert [m["k"] for m in adsb.accept(both, RATE, Q, fix=0)[0]] == [90000]
    other = _det([(100, A.F_VELOCITY, 50, 40), (90000, A.F_CALLSIGN, 60)])
    assert [m["k"] for m in adsb.accept(other, RATE, Q)[0]] == [90000]


def test_address_parity_needs_a_known_address():
    assert adsb.crc(AP_FRAME) == 0x4840D6 and AP_FRAME[0] >> 3 == 4
    assert adsb.accept(_det([(100, AP_FRAME, 50)]), RATE, Q)[0] == []
    msgs, counts = adsb.accept(_det([(100, AP_FRAME, 50), (5000, A.F_DF11, 60)]), RATE, Q)
    assert [(m["k"], m["df"], m["icao"], m["raw"]) for m in msgs] == [(100, 4, 0x4840D6, AP_FRAME), (5000, 11, 0x4840D6, adsb.as_bytes(A.F_DF11))]
    assert counts["address_parity"] == 1 and counts["clean"] == 1
    assert [m["k"] for m in adsb.accept(_det([(100, AP_FRAME, 50), (5000, A.F_VELOCITY, 60)]), RATE, Q)[0]] == [5000]
    # formats that are neither: dropped whatever their remainder
    df24 = bytes([24 << 3]) + bytes(13)
    assert adsb.accept(_det([(100, df24, 50), (5000, A.F_DF11, 60)]), RATE, Q)[1]["clean"] == 1


def test_duplicates():
    two_chips = 2 * RATE * Q // adsb.U                               # candidates in two chips: 9.6 -> those less than 10 on are one group
    assert two_chips == 9
    rows = [(1000, A.F_VELOCITY, 50), (1001, A.F_VELOCITY, 70), (1009, A.F_VELOCITY, 70), (1010, A.F_VELOCITY, 10)]
    msgs, counts = adsb.accept(_det(rows + [(90000, A.F_VELOCITY, 60)]), RATE, Q)
    assert [(m["k"], m["score"]) for m in msgs] == [(1001, 70), (1010, 10), (90000, 60)]       # greatest score, then the lowest k
    assert counts["duplicates"] == 2
    # fewer repaired bits come first, whatever the score
    msgs, _ = adsb.accept(_det([(1000, A.F_VELOCITY, 90, 40), (1002, A.F_VELOCITY, 20)]), RATE, Q)
    assert [(m["k"], m["fixed"]) for m in msgs] == [(1002, -1)]
    # a different frame that starts inside another one is kept
    msgs, counts = adsb.accept(_det([(1000, A.F_DF11, 50), (1000 + 640, A.F_CALLSIGN, 70)]), RATE, Q)
    assert [m["k"] for m in msgs] == [1000, 1640] and counts["duplicates"] == 0


# ---------------------------------------------------------------------------------------------------------------- the synthesiser
def test_encode_durations():
    for rate in (2000000, 2400000, 10000000):
        spc = rate / 2e6
        for frame, bits in ((A.F_CALLSIGN, 112), (A.F_DF11, 56)):
            c = adsb.cover(frame, rate, 10.3, 4000)
            assert abs(c.sum() - (4 + bits) * spc) < 1e-9            # four preamble pulses and one pulse per bit, half a microsecond each
            on = np.flatnonzero(c > 0)
            assert on[0] == 10 and on[-1] in (math.ceil(10.3 + (16 + 2 * bits) * spc) - 1, math.ceil(10.3 + (15 + 2 * bits) * spc) - 1)
            assert c.max() <= 1.0 + 1e-12
    raw = adsb.encode([A.F_CALLSIGN], 2400000, [5.0])
    assert raw.shape == (5 + 288 + 1, 2) and raw.dtype == np.uint8
    assert adsb.n_candidates(len(raw), 2400000, 4) > 5 * 4           # the frame's own start is a candidate
    quiet = adsb.encode([], 2400000, [], n=50)
    assert np.all((quiet == 127) | (quiet == 128))
    assert np.array_equal(adsb.encode([A.F_ODD], 2400000, [3.3], 50.0, 2.0, 7), adsb.encode([A.F_ODD], 2400000, [3.3], 50.0, 2.0, 7))


def _all_found(rate, phases, seed, keep_off_half=False):
    rng = np.random.default_rng(seed)
    Qd = adsb.check_rate(rate)[1]
    step = adsb.reach(rate) + 40
    lost = []
    for ph in range(phases):
        frac = rng.uniform(-0.25, 0.25) % 1.0 if keep_off_half else rng.uniform(0.0, 1.0)
        starts = 20 + step * np.arange(8) + frac
        raw = adsb.encode(A.FRAMES, rate, starts, 40.0, 3.0, seed=1000 * seed + ph, n=int(starts[-1]) + step)
        msgs, info, _ = decode_adsb.decode_host(raw, rate, Qd)
        got = {m["raw"] for m in msgs}
        lost += [(frac, f) for f in A.FRAMES if adsb.as_bytes(f) not in got]
        assert len(msgs) == 8 and info["clean"] == 8 and info["passed"] >= 8
    return lost


def test_every_frame_is_found_at_2400000():
    assert _all_found(2400000, 100, 1) == []


def test_every_frame_is_found_at_10000000():
    assert _all_found(10000000, 40, 2) == []


def test_every_frame_is_found_at_2000000_off_the_half_sample():
    assert _all_found(2000000, 40, 3, keep_off_half=True) == []


def test_rate_and_phase_limits():
    assert adsb.check_rate(2000000) == (2000000, 4) and adsb.check_rate(2400000) == (2400000, 4)
    assert adsb.check_rate(4000000) == (4000000, 2) and adsb.check_rate(8000000) == (8000000, 1)
    assert adsb.check_rate(20000000) == (20000000, 1) and adsb.check_rate(3999999) == (3999999, 4)
    for rate, q in ((1999999, None), (20000001, None), (2400000.5, None), (2400000, 3), (2400000, 0), (2400000, 16)):
        with pytest.raises(ValueError):
            adsb.check_rate(rate, q)
    with pytest.raises(ValueError):
        decode_adsb.decode_adsb.fromIQ(np.zeros((10, 2), np.uint8), 1000000)
    assert adsb.n_candidates(287, 2400000, 4) == 0 and adsb.n_candidates(288, 2400000, 4) == 1 and adsb.n_candidates(289, 2400000, 4) == 5
    assert adsb.grid(2400000, 4) == (20, 5, 24) and adsb.grid(20000000, 1) == (1, 1, 10) and adsb.grid(3000001, 2) == (2000000, 1000000, 3000001)


def test_chip_energies_against_the_definition():
    """adsb.chips takes differences of a running integral; here the sum of overlap / g times power, term by term"""
    for rate, Qd in ((2400000, 4), (3000001, 2), (2000000, 8)):
        n = adsb.reach(rate) + 3
        p = adsb.power(np.random.default_rng(rate).integers(0, 256, (n, 2)).astype(np.uint8))
        g = math.gcd(adsb.U // Qd, rate)
        ks = [0, 1, adsb.n_candidates(n, rate, Qd) - 1]
        E = adsb.chips(p, rate, Qd, ks)
        for row, k in zip(E, ks):
            for c in (0, 1, 15, 16, 100, 239):
                a = k * (adsb.U // Qd) + c * rate
                want = sum((min(a + rate, (j + 1) * adsb.U) - max(a, j * adsb.U)) // g * int(p[j]) for j in range(a // adsb.U, (a + rate - 1) // adsb.U + 1))
                assert row[c] == want


def test_noise_alone_gives_no_message():
    raw = np.clip(np.rint(np.random.default_rng(5).normal(127.5, 3.0, (100000, 2))), 0, 255).astype(np.uint8)
    msgs, info, aircraft = decode_adsb.decode_host(raw, 2400000)
    assert msgs == [] and aircraft == {} and info["clean"] == 0
    assert 0.0005 < info["passed"] / info["candidates"] < 0.005     # about 0.2 % of the candidates pass the preamble test


# ---------------------------------------------------------------------------------------------------------------- the C entries
@pytest.fixture(scope="module")
def lib():
    from directdemod_amd import _hip
    return _hip.load()


def test_entries_classify_their_arguments_before_any_buffer(lib):
    from directdemod_amd import _hip
    count = C.c_int64(77)
    bad = _hip.DD_ERR_INVALID
    # n = 0 returns at once, whatever the buffers
    assert lib.dd_adsb_candidates(None, 0, 2400000, 4, None, 0, C.byref(count), None) == 0 and count.value == 0
    assert lib.dd_adsb_demod(None, 0, 2400000, 4, None, 5, None, None, None, None) == 0
    assert lib.dd_debug_adsb_chips(None, 0, 2400000, 4, None, 5, None, None) == 0
    assert lib.dd_adsb_demod(None, 500, 2400000, 4, None, 0, None, None, None, None) == 0
    # null buffers with n > 0
    assert lib.dd_adsb_candidates(None, 500, 2400000, 4, None, 0, C.byref(count), None) == bad
    assert lib.dd_adsb_candidates(None, 500, 2400000, 4, None, 0, None, None) == bad
    assert lib.dd_adsb_demod(None, 500, 2400000, 4, None, 5, None, None, None, None) == bad
    assert lib.dd_debug_adsb_chips(None, 500, 2400000, 4, None, 5, None, None) == bad
    assert b"null buffer" in lib.dd_last_error()
    # sizes, rates and phase counts, with buffers that must not be touched
    wild = C.c_void_p(16)
    for n, rate, q, cap in ((-1, 2400000, 4, 8), (500, 1999999, 4, 8), (500, 20000001, 1, 8), (500, 2400000, 3, 8), (500, 2400000, 0, 8),
                            (500, 2400000, 16, 8), (500, 2400000, 4, -1), (1 << 28, 2400000, 4, 8)):
        assert lib.dd_adsb_candidates(wild, n, rate, q, wild, cap, C.byref(count), None) == bad
        assert lib.dd_adsb_demod(wild, n, rate, q, wild, cap, wild, wild, wild, None) == bad
        assert lib.dd_debug_adsb_chips(wild, n, rate, q, wild, cap, wild, None) == bad
