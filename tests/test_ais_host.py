"""The host side of the AIS decoder (directdemod_amd/ais.py, decode_ais.decode_host): the parser, the sentences, the CRC, bit stuffing,
the quantiser, and the NumPy restatement of the kernels on synthesised bursts.  No GPU."""
import numpy as np
import pytest

import _ais as A
from directdemod_amd import ais, decode_ais
from directdemod_amd.decode_afsk1200 import decode_afsk1200, fcs_crc16


@pytest.mark.parametrize("i", range(len(A.VECTORS)))
def test_parse_published_sentences(i):
    sentences, ty, mmsi, want = A.VECTORS[i]
    bits, channel = ais.from_nmea(sentences)
    assert len(bits) == A.NBITS[i] and channel == A.channel_of(i)
    got = ais.parse(bits)
    assert got["type"] == ty and got["mmsi"] == mmsi
    for key, v in want.items():
        if key in ("lon", "lat"):
            assert abs(got[key] - v) <= 1e-6, (key, got[key], v)
        else:
            assert got[key] == v, (key, got[key], v)
    assert ais.parse(np.packbits(bits).tobytes()) == got             # bytes or bits


def test_parse_not_given_values_and_other_types():
    bits = A.payload_bits(0).copy()
    bits[50:60] = 1                                                  # sog 1023
    bits[116:128] = [1, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0]            # cog 3600
    bits[61:89] = ((181 * 600000) >> np.arange(27, -1, -1)) & 1
    bits[89:116] = ((91 * 600000) >> np.arange(26, -1, -1)) & 1
    got = ais.parse(bits)
    assert got["sog"] is None and got["cog"] is None and got["lon"] is None and got["lat"] is None
    bits[:6] = [0, 0, 1, 0, 0, 1]                                    # type 9: no table
    assert ais.parse(bits) == {"type": 9, "repeat": 0, "mmsi": 477553000}
    assert set(ais.parse(A.payload_bits(0)[:100])) == {"type", "repeat", "mmsi"}       # shorter than its table


@pytest.mark.parametrize("i", range(len(A.VECTORS)))
def test_sentences_round_trip(i):
    """dearmor -> nmea gives every sentence back byte for byte.  The published two-sentence message is cut at 56 characters, as
    many receivers do; nmea cuts at 60 unless told otherwise."""
    sentences = A.VECTORS[i][0]
    bits, channel = ais.from_nmea(sentences)
    first = sentences[0].split(",")
    seq = int(first[3]) if first[3] else None
    width = len(first[5]) if len(sentences) > 1 else 60
    assert ais.nmea(bits, channel, seq, width) == sentences
    payload, fill = ais.armor(bits)
    assert payload == "".join(s.split(",")[5] for s in sentences) and fill == int(sentences[-1].split(",")[6][0])
    assert np.array_equal(ais.dearmor(payload, fill), bits)
    if len(sentences) > 1:
        cut = ais.nmea(bits, channel, seq)
        assert [len(s.split(",")[5]) for s in cut] == [60, 11] and np.array_equal(ais.from_nmea(cut)[0], bits)


def test_armor_table_and_bad_input():
    for v in range(64):
        ch = ais.armor([(v >> j) & 1 for j in range(5, -1, -1)])[0]
        assert ch == (chr(v + 48) if v < 40 else chr(v + 56))
        assert ais.dearmor(ch).tolist() == [(v >> j) & 1 for j in range(5, -1, -1)]
    for bad in ("X", "_", "x", "/", " "):
        with pytest.raises(ValueError):
            ais.dearmor(bad)
    with pytest.raises(ValueError):
        ais.from_nmea(["!AIVDM,1,1,,B,177KQJ5000G?tO`K>RA1wUbN0TKH,0*5D"])


def test_crc_agrees_with_the_afsk_one():
    rng = np.random.default_rng(1)
    for L in (1, 2, 3, 5, 21, 53, 158):
        d = rng.integers(0, 256, L).astype(np.uint8).tobytes()
        stream = np.unpackbits(np.frombuffer(d, dtype=np.uint8), bitorder="little")
        f = ais.crc(d)
        assert "".join(str((f >> j) & 1) for j in range(16)) == fcs_crc16("".join(str(b) for b in stream)), L
        full = np.unpackbits(np.frombuffer(d + bytes((f & 0xFF, f >> 8)), dtype=np.uint8), bitorder="little")
        assert ais.crc_register(full) == ais.GOOD
        reg = 0xFFFF                                                 # the register bit by bit, against the table route
        for b in full:
            reg = (reg >> 1) ^ (0x8408 if (reg ^ int(b)) & 1 else 0)
        assert reg == ais.GOOD


def test_stuffing_round_trips_on_runs_of_ones():
    rng = np.random.default_rng(2)
    words = [np.ones(64, np.uint8), np.zeros(64, np.uint8), np.array(([1] * 5 + [0]) * 12, np.uint8), np.array(([1] * 6 + [0]) * 10, np.uint8),
             np.array([0] + [1] * 11 + [0, 1, 1, 1, 1, 1], np.uint8)]
    words += [(rng.random(200) < 0.85).astype(np.uint8) for _ in range(20)]
    for w in words:
        s = ais.stuff(w)
        run = 0
        for b in s:                                                  # no six ones in a row
            run = run + 1 if b else 0
            assert run <= 5
        assert np.array_equal(ais.destuff(s), w)
        marks = decode_afsk1200.find_bit_stuffing(s)                 # the serial walk the AFSK decoder describes
        assert np.array_equal(np.array(decode_afsk1200.reduce_stuffed_bit(s, marks), dtype=np.uint8), w)


def test_quantiser_returns_chosen_integers():
    k = np.concatenate((np.arange(-5000, 5001), [1 << 20, -(1 << 20), (1 << 21), -(1 << 21), 1048575, 333772, -777777]))
    assert np.array_equal(ais.quantise(A.as_audio(k)), k)
    rng = np.random.default_rng(3)
    k = rng.integers(-(1 << 21), (1 << 21) + 1, 200000)
    assert np.array_equal(ais.quantise(A.as_audio(k)), k)
    assert ais.quantise([np.nan, np.inf, -np.inf, 7.0, -7.0]).tolist() == [0, 0, 0, 0, 0]


def test_params_and_rates():
    assert ais.params(48000)[:2] == (5.0, 3) and ais.params(38400)[1] == 3 and ais.params(153600)[1] == 9
    for rate in (38399.0, 153601.0, 22050, float("nan")):
        with pytest.raises(ValueError, match="9600"):
            ais.params(rate)
    for w in (0, 2, 17):
        with pytest.raises(ValueError):
            ais.params(48000, w)
    with pytest.raises(ValueError):
        ais.params(48000, None, 12)
    assert ais.window_taps(2400000) == 151 and ais.window_taps(2048000) == 129 and ais.window_taps(240000) == 15


def test_each_comparison_is_strict_in_the_restatement():
    for k, (tie, up, plus) in enumerate(A.tie_cases()):
        q = ais.quantise(A.as_audio(tie))
        v = ais.values(q, [0], np.arange(24), 4.0, 3)[0]
        S = v[:16].sum()
        assert 16 * v[k] == S and np.count_nonzero(16 * v == S) == 1, k
        assert (0 in ais.candidates_host(A.as_audio(tie), 4.0, 3)) == (not plus), k      # equality reads -
        assert (0 in ais.candidates_host(A.as_audio(up), 4.0, 3)) == plus, k


def test_crafted_frames_and_statuses():
    msg = A.payloads()[0]
    for sps, w in ((4, 3), (5, 3), (16, 9)):
        x = A.as_audio(A.rect(A.frame_raw(msg), sps, t=37))
        ts = ais.candidates_host(x, float(sps), w)
        assert 37 in ts
        det = ais.demod_host(x, float(sps), w, [37])
        assert det["status"][0] == ais.OK and det["nbits"][0] == 184 and bytes(det["frames"][0][:21]) == msg
        assert det["rem"][0] == ais.GOOD and not det["frames"][0][23:].any()
    raw = A.frame_raw(msg)
    cases = {ais.ABORT: np.concatenate((raw[:50], [0], [1] * 7, [0])), ais.LENGTH: A.frame_raw(msg, extra=[0]),
             ais.STUFFING: np.concatenate((raw[:40], [0, 1, 1, 1, 1, 1], ais.FLAG)), ais.NO_END: np.zeros(1300, np.uint8)}
    flipped = raw.copy()
    flipped[20] ^= 1
    cases[ais.CRC] = flipped
    for status, bits in cases.items():
        det = ais.demod_host(A.as_audio(A.rect(bits, 5, t=11)), 5.0, 3, [11])
        assert det["status"][0] == status, ais.STATUS[status]


@pytest.fixture(scope="module")
def decoded():
    raw, starts = A.recording()
    return decode_ais.decode_host(raw, A.FS, (A.OFFSETS["A"], A.OFFSETS["B"]))


def test_decode_host_finds_all_eight_on_their_channels(decoded):
    msgs, info, vessels = decoded
    assert A.ebn0_db(A.AMPLITUDE, A.SIGMA, A.FS) >= 24.0
    raw, starts = A.recording()
    want = A.payloads()
    assert len(msgs) == 8 and info["accepted"] == 8
    for i, (m, s) in enumerate(zip(msgs, starts)):                   # time order is the order sent
        assert m["raw"] == want[i] and m["channel"] == A.channel_of(i), i
        assert m["type"] == A.VECTORS[i][1] and m["mmsi"] == A.VECTORS[i][2] and m["nbits"] == A.NBITS[i]
        at = ais.flag_start(A.FS, s) / 5.0                           # (240 kS/s -> 48 kS/s)
        delay = 7 / 5.0 + 20 - 0.5                                   # the 15-tap window at 240 kS/s, the 41-tap low-pass, the discriminator
        assert abs(m["start"] - at - delay) <= 2, (m["start"], at)
        assert ais.from_nmea(m["nmea"])[1] == m["channel"] and np.array_equal(np.packbits(ais.from_nmea(m["nmea"])[0]).tobytes(), want[i])
    assert [m["nmea"] for m in msgs if m["type"] != 5] == [A.VECTORS[i][0] for i in range(8) if i != 4]
    assert info["duplicates"] >= 8 and info["candidates"] >= info["accepted"] + info["duplicates"]
    assert vessels[369190000]["shipname"] == "MT.MITCHELL" and vessels[369190000]["destination"] == "SEATTLE"
    assert vessels[271041815]["shipname"] == "PROGUY" and vessels[271041815]["callsign"] == "TC6163"
    assert len(vessels[477553000]["track"]) == 1 and abs(vessels[477553000]["track"][0][1] - 47.582833) < 1e-6


def test_audio_level_decode_and_polarity():
    rate = 2048000 / 42.0
    want = A.payloads()
    starts = 300.25 + np.arange(8) * 3000.0
    for level in (1, -1):
        x = ais.encode_audio(want, rate, starts, sigma=0.03, seed=4, carrier_offsets=np.linspace(-1500, 1500, 8), levels=level)
        msgs, info, _ = decode_ais.decode_audio_host(x, rate, "B")
        assert [m["raw"] for m in msgs] == want and all(m["channel"] == "B" for m in msgs)
        for m, s in zip(msgs, starts):
            assert abs(m["start"] - ais.flag_start(rate, s)) <= 2


@pytest.fixture(scope="module")
def lib():
    from directdemod_amd import _hip
    return _hip.load()


def test_entries_classify_their_arguments_before_any_buffer(lib):
    import ctypes as C
    from directdemod_amd import _hip
    count = C.c_int64(77)
    bad = _hip.DD_ERR_INVALID
    # n = 0 returns at once, whatever the buffers
    assert lib.dd_ais_candidates(None, 0, 5.0, 3, 0, None, 0, C.byref(count), None) == 0 and count.value == 0
    assert lib.dd_ais_demod(None, 0, 5.0, 3, None, 5, None, None, None, None) == 0
    assert lib.dd_ais_demod(None, 500, 5.0, 3, None, 0, None, None, None, None) == 0
    # null buffers with n > 0
    assert lib.dd_ais_candidates(None, 500, 5.0, 3, 0, None, 0, C.byref(count), None) == bad
    assert lib.dd_ais_candidates(None, 500, 5.0, 3, 0, None, 0, None, None) == bad
    assert lib.dd_ais_demod(None, 500, 5.0, 3, None, 5, None, None, None, None) == bad
    assert b"null buffer" in lib.dd_last_error()
    # sizes, samples per bit, windows and slack, with buffers that must not be touched
    wild = C.c_void_p(16)
    for n, sps, w, slack, cap in ((-1, 5.0, 3, 0, 8), (500, 3.99, 3, 0, 8), (500, 16.01, 9, 0, 8), (500, float("nan"), 3, 0, 8),
                                  (500, 5.0, 2, 0, 8), (500, 5.0, 0, 0, 8), (500, 5.0, 17, 0, 8), (500, 5.0, 3, 0, -1), (1 << 31, 5.0, 3, 0, 8)):
        assert lib.dd_ais_candidates(wild, n, sps, w, slack, wild, cap, C.byref(count), None) == bad
        assert lib.dd_ais_demod(wild, n, sps, w, wild, cap, wild, wild, wild, None) == bad
    for slack in (-1, 12):
        assert lib.dd_ais_candidates(wild, 500, 5.0, 3, slack, wild, 8, C.byref(count), None) == bad
