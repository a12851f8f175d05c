"""Reed-Solomon (255,223) and the packet layer of the LRPT decoder as lrpt.py states them, on the CPU: the
known answers of the field and the code, the bounded-distance decoder at and past its radius, the interleave, packet reassembly on
hand-made VCDUs, and the whole restatement over the soft symbols of the reference's own walk of tests/_rs.py's case (b)
(tests/golden/lrpt_rs_b.npz, tools/gen_golden.py --lrpt-rs)."""
import os

import numpy as np
import pytest

import _rs
from directdemod_amd import lrpt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _damaged(seed, nerr, nwords=20):
    """(sent codewords, the same with nerr bytes changed in each at random positions by random non-zero values)"""
    rng = _rng(seed)
    sent = lrpt.rs_encode(rng.integers(0, 256, size=(nwords, 223), dtype=np.uint8))
    got = sent.copy()
    for row in got:
        row[rng.choice(255, nerr, replace=False)] ^= rng.integers(1, 256, nerr, dtype=np.uint8)
    return sent, got


# ------------------------------------------------------------------ field and code
def test_known_answers():
    g = lrpt.rs_generator()
    assert bytes(g).hex() == "015b7f56101e0deb61a5082a3656ab207120ab56362a08a561eb0d1e10567f5b01"
    assert len(g) == 33 and g[0] == 1 and g[32] == 1 and np.array_equal(g, g[::-1])
    ex, lg = lrpt.gf_tables()
    published = [0, 249, 59, 66, 4, 43, 126, 251, 97, 30, 3, 213, 50, 66, 170, 5, 24]            # CCSDS 131.0-B, as powers of alpha
    assert [int(lg[v]) for v in g[:17]] == published and [int(lg[v]) for v in g[:15:-1]] == published
    assert sorted(ex[:255].tolist()) == list(range(1, 256)) and ex[8] == 0x87 and all(ex[lg[v]] == v for v in range(1, 256))
    word = lrpt.rs_encode(np.arange(223, dtype=np.uint8))
    assert np.array_equal(word[:223], np.arange(223))
    assert bytes(word[223:]).hex() == "2fbd4fb4748494b9acd554627212eeb3ebed41191de1d36320ea49290b25abcf"
    one = np.zeros(223, dtype=np.uint8)
    one[222] = 1
    assert bytes(lrpt.rs_encode(one)[223:]).hex() == "5b7f56101e0deb61a5082a3656ab207120ab56362a08a561eb0d1e10567f5b01"


def test_encoded_words_have_zero_syndromes():
    words = lrpt.rs_encode(_rng(1).integers(0, 256, size=(50, 223), dtype=np.uint8))
    syn = lrpt.rs_syndromes(words)
    assert syn.shape == (50, 32) and not syn.any()
    words[7, 100] ^= 1
    assert lrpt.rs_syndromes(words)[7].all() and not lrpt.rs_syndromes(words)[8].any()
    fixed, errors = lrpt.rs_decode_np(words[8])
    assert errors.shape == () and errors == 0 and np.array_equal(fixed, words[8])


@pytest.mark.parametrize("nerr", [1, 8, 15, 16])
def test_decodes_up_to_sixteen_errors(nerr):
    # with e <= 16 errors every other codeword is at distance >= 33 - e > 16: the answer is forced
    sent, got = _damaged(10 + nerr, nerr)
    fixed, errors = lrpt.rs_decode_np(got)
    assert errors.tolist() == [nerr] * 20
    assert np.array_equal(fixed, sent)


@pytest.mark.parametrize("nerr", [17, 20, 40])
def test_past_the_radius_is_left_alone(nerr):
    # the seeds are fixed and the -1 asserted, so that a seed that ever lands inside another codeword's sphere is seen
    _, got = _damaged(30 + nerr, nerr)
    fixed, errors = lrpt.rs_decode_np(got)
    assert errors.tolist() == [-1] * 20
    assert np.array_equal(fixed, got)


def test_random_words_are_left_alone():
    got = _rng(5).integers(0, 256, size=(20, 255), dtype=np.uint8)       # inside some sphere with probability about 1e-13 each
    fixed, errors = lrpt.rs_decode_np(got)
    assert errors.tolist() == [-1] * 20
    assert np.array_equal(fixed, got)


def test_interleave_round_trip():
    bodies = _rng(6).integers(0, 256, size=(3, 1020), dtype=np.uint8)
    words = lrpt.deinterleave(bodies)
    assert words.shape == (3, 4, 255)
    assert all(words[1, k % 4, k // 4] == bodies[1, k] for k in (0, 1, 5, 891, 892, 1019))
    assert np.array_equal(lrpt.interleave(words), bodies)
    sent = lrpt.rs_encode(_rng(7).integers(0, 256, size=(2, 4, 223), dtype=np.uint8))
    got = lrpt.interleave(sent)
    got[0, 40:104] ^= 0xFF                                                 # a burst of 64 bytes: 16 in each codeword
    got[1, 40:108] ^= 0xFF                                                 # 68: 17 in each
    fixed, errors = lrpt.rs_frames_np(got)
    assert errors.tolist() == [[16] * 4, [-1] * 4]
    assert np.array_equal(fixed[0], lrpt.interleave(sent)[0]) and np.array_equal(fixed[1], got[1])


# ------------------------------------------------------------------ headers and reassembly
def test_headers():
    v = _rs.vcdu(12, 0x123456, 0x2A5, bytes(882))
    assert len(v) == 892 and lrpt.vcdu_header(v)["vcid"] == 12 and lrpt.vcdu_header(v)["counter"] == 0x123456
    assert lrpt.mpdu_header(v)["fhp"] == 0x2A5
    assert lrpt.mpdu_header(_rs.vcdu(5, 0, 0x7FF, bytes(882)))["fhp"] == 0x7FF
    h = lrpt.packet_header(bytes([0x0D, 0x34, 0x9F, 0xFE, 0x01, 0x02]) + bytes(300))
    assert (h["apid"], h["flags"], h["count"], h["length"]) == (0x534, 2, 0x1FFE, 7 + 0x102)
    p = _rs.packet(70, 300, 40, _rng(8))
    assert len(p) == 40 and lrpt.packet_header(p) == dict(version=0, type=0, secondary=0, apid=70, flags=3, count=300, length=40)


A_LEN = [500, 382, 881, 100, 778, 1087, 300, 1000]
B_LEN = [400, 1364, 300, 2000]
A, B, FILL = 5, 12, 63
ORDER = [(A, 0), (B, 0), (A, 1), (FILL, 0), (B, 1), (A, 2), (A, 3), (B, 2), (A, 4)]       # (channel, which of its zones)


@pytest.fixture(scope="module")
def laid():
    """Channel A: a0 + a1 end exactly at zone 0's end; a2 leaves 1 byte of zone 1 for a3's header; a4 leaves 5 bytes of zone 2 for
    a5's; a5 fills zone 3 (no header in it) and ends in zone 4; a7 never ends.  A's counter wraps 2^24 between zones 1 and 2.
    Channel B: b1 runs from zone 0 to exactly the end of zone 1, so it is closed by zone 2, whose pointer is 0; b3 never ends.
    -> (packets per channel, frames as (vcid, counter, fhp, zone) in ORDER)"""
    rng = _rng(9)
    pk, zs = {}, {}
    for ch, lens in ((A, A_LEN), (B, B_LEN)):
        at = np.concatenate(([0], np.cumsum(lens)))[:-1]
        pk[ch] = [(int(a), _rs.packet(64 + i % 4, i, n, rng)) for i, (a, n) in enumerate(zip(at, lens))]
        zs[ch] = _rs.zones(pk[ch], 5 if ch == A else 3)
    zs[FILL] = [(0x7FE, rng.integers(0, 256, 882, dtype=np.uint8).tobytes())]
    assert [f for f, _ in zs[A]] == [0, 0, 99, 0x7FF, 200] and [f for f, _ in zs[B]] == [0, 0x7FF, 0]
    first = {A: (1 << 24) - 2, B: 10, FILL: 77}
    frames = [(ch, (first[ch] + k) & 0xFFFFFF, zs[ch][k][0], zs[ch][k][1]) for ch, k in ORDER]
    assert [c for ch, c, _, _ in frames if ch == A] == [(1 << 24) - 2, (1 << 24) - 1, 0, 1, 2]
    return {ch: [p for _, p in v] for ch, v in pk.items()}, frames


def _run(frames, ok=None):
    v = np.array([_rs.vcdu(*f) for f in frames])
    ok = np.ones(len(frames), dtype=bool) if ok is None else ok
    return lrpt.packets(v, ok, [f[0] for f in frames], [f[1] for f in frames])


def _want(pk, names):
    return [pk[A if n[0] == "a" else B][int(n[1:])] for n in names]


def test_packets_two_channels_every_special_length(laid):
    pk, frames = laid
    got, info = _run(frames)
    assert got == _want(pk, ["a0", "a1", "b0", "a2", "a3", "a4", "b1", "b2", "a5", "a6"])
    assert info.dtype == lrpt.PACKET_INFO
    assert info["vcid"].tolist() == [A, A, B, A, A, A, B, B, A, A]
    assert info["frame"].tolist() == [0, 0, 1, 2, 2, 5, 1, 7, 5, 8]          # the row in which the packet's first byte lies
    assert info["length"].tolist() == [500, 382, 400, 881, 100, 778, 1364, 300, 1087, 300]
    assert info["apid"].tolist() == [64, 65, 64, 66, 67, 64, 65, 66, 65, 66] and info["count"].tolist() == [0, 1, 0, 2, 3, 4, 1, 2, 5, 6]
    assert np.all(info["flags"] == 3)


def test_packets_counter_gap(laid):
    pk, frames = laid
    got, _ = _run(frames[:5] + frames[6:])                  # A's zone 2 never arrives: a3, a4 and a5 go, B is untouched
    assert got == _want(pk, ["a0", "a1", "b0", "a2", "b1", "b2", "a6"])


def test_packets_frame_not_ok(laid):
    pk, frames = laid
    ok = np.ones(len(frames), dtype=bool)
    ok[6] = False                                           # A's zone 3: a5 goes, and so does b1, which was under way
    got, _ = _run(frames, ok)
    assert got == _want(pk, ["a0", "a1", "b0", "a2", "a3", "a4", "b2", "a6"])


def test_packets_pointer_882(laid):
    pk, frames = laid
    bad = list(frames)
    bad[5] = bad[5][:2] + (882,) + bad[5][3:]               # nothing of A's zone 2 is used, and a3 goes with it
    got, _ = _run(bad)
    assert got == _want(pk, ["a0", "a1", "b0", "a2", "b1", "b2", "a6"])
    bad[5] = bad[5][:2] + (2046,) + bad[5][3:]
    assert _run(bad)[0] == got


def test_packets_continuation_disagrees_with_pointer(laid):
    pk, frames = laid
    bad = list(frames)
    bad[5] = bad[5][:2] + (877,) + bad[5][3:]               # the pointer names a5's header: a3's byte + 877 bytes are no packet
    got, _ = _run(bad)
    assert got == _want(pk, ["a0", "a1", "b0", "a2", "b1", "b2", "a5", "a6"])


def test_packets_nothing():
    got, info = lrpt.packets(np.zeros((0, 892), dtype=np.uint8), [], [], [])
    assert got == [] and info.shape == (0,) and info.dtype == lrpt.PACKET_INFO


# ------------------------------------------------------------------ the restatement chain over the reference's walk of case (b)
@pytest.fixture(scope="module")
def chain_b():
    g = np.load(os.path.join(GOLDEN, "lrpt_rs_b.npz"))
    soft, nsym = g["soft"], int(g["nsym"])
    raw, built, _ = _rs.case("b")
    assert raw.shape[0] == int(g["n"]) and _rs.sha256(raw) == str(g["sha256"])
    starts = lrpt.frame_starts(lrpt.asm_candidates_np(soft, nsym), nsym)
    bodies = np.array([lrpt.finish_np(lrpt.viterbi_blocks(soft, nsym, int(q), int(h), 8192), soft, nsym, int(q), int(h))[0]
                       for q, h, _ in starts])
    return built, bodies


def test_restatement_chain_case_b(chain_b):
    built, bodies = chain_b
    fixed, errors = lrpt.rs_frames_np(bodies)
    ok = np.all(errors >= 0, axis=1)
    vcid = fixed[:, 1] & 0x3F
    counter = np.array([lrpt.vcdu_header(b)["counter"] for b in fixed])
    rows, state = _rs.match(built, vcid, counter, ok)
    assert rows == list(range(2, 12))
    # case (b)'s two conditions: the short fade's frame is corrected with something to correct in every codeword, the long fade's is lost
    e = errors[rows.index(_rs.SHORT)]
    assert np.all((e >= 1) & (e <= 16)) and e.max() >= 4
    assert np.any(errors[rows.index(_rs.LONG)] == -1)
    assert [r for r, good in zip(rows, ok) if not good] == [_rs.LONG]
    quiet = [i for i, r in enumerate(rows) if r not in (_rs.SHORT, _rs.LONG)]
    assert not errors[quiet].any()                                                      # the loops stay locked through both fades
    good = np.nonzero(ok)[0]
    assert np.array_equal(fixed[good], built["bodies"][np.array(rows)[good]])
    bad = rows.index(_rs.LONG)
    assert np.array_equal(fixed[bad], bodies[bad])
    got, info = lrpt.packets(fixed[:, :892], ok, vcid, counter)
    want = _rs.expected(built, state)
    assert got == [p["data"] for p in want] and len(got) >= 8
    assert info["frame"].tolist() == [rows.index(p["first"]) for p in want] and info["vcid"].tolist() == [p["vcid"] for p in want]
    # the first packet after the long fade that starts at a first-header pointer, and the one that needs the corrected frame
    after = next(p for p in built["packets"] if p["first"] == _rs.LONG + 1 and p["vcid"] == built["vcid"][_rs.LONG + 1])
    assert after["data"] in got
    assert any(p["first"] < _rs.SHORT < p["last"] and p["vcid"] == built["vcid"][_rs.SHORT] for p in want)
