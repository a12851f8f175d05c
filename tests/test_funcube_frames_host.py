"""funcube_fec.py's NumPy restatement of DESIGN.md section 4.17 on the CPU: the format constants, the encoder against the decoder,
each stage's edges, two frames in a stream, the inverted polarity and noise.  All arithmetic is integer and every comparison is
exact.  The symbol-level inputs come from tests/_funcube_frames.py."""
import numpy as np
import pytest

import _funcube_frames as F
from directdemod_amd import funcube_fec as fec
from directdemod_amd import lrpt

SYNC = "1111111000011101111001011001001000000100010011000101110101101100" "0"
LEAD = 137


@pytest.fixture(scope="module")
def clean():
    """one frame from bit 3 of a 5210-bit stream behind 137 symbols: (data, soft symbols, D, p)"""
    data = F.payload(1)
    r = F.symbols(2, fec.CHANNEL_BITS + 10, [(3, data, False)], lead=LEAD)
    return data, r, fec.diff_np(r), F.position(LEAD, 3)


def test_constants():
    assert (fec.FRAME_BYTES, fec.CHANNEL_BITS, fec.SYMBOLS_PER_BIT, fec.MIN_SCORE, fec.GUARD) == (256, 5200, 10, 54, 10)
    assert fec.INFO.names == ("symbol", "sample", "inverted", "sync_score", "sync_corr", "corrected", "rs_errors", "ok", "sat_id",
                              "frame_type") and fec.INFO["rs_errors"].shape == (2,)
    assert "".join(str(int(b)) for b in fec.sync_vector()) == SYNC and len(SYNC) == 65


def test_scrambler_is_the_ccsds_sequence():
    sr, out = 0xFF, []                                            # the AO-40 way: output bit 7, feedback parity(sr & 0x95)
    for _ in range(8 * 320):
        out.append((sr >> 7) & 1)
        sr = ((sr << 1) | (bin(sr & 0x95).count("1") & 1)) & 0xFF
    assert np.array_equal(np.packbits(np.array(out, dtype=np.uint8)), lrpt.pn_sequence(320))


def test_encoder_polynomials_are_lrpts():
    bits = F.rng(3).integers(0, 2, 400).astype(np.uint8)
    sr, out = 0, []                                               # 0x4F / 0x6D with the newest bit at the LSB
    for b in bits:
        sr = ((sr << 1) | int(b)) & 0x7F
        out += [bin(sr & 0x4F).count("1") & 1, bin(sr & 0x6D).count("1") & 1]
    assert np.array_equal(np.array(out, dtype=np.uint8), lrpt.encode(bits))


def test_interleaver_is_a_permutation_with_three_unused_slots():
    q = np.concatenate((80 * np.arange(65), fec.code_positions()))
    assert len(np.unique(q)) == 65 + 5132 and q.min() == 0
    assert np.setdiff1d(np.arange(5200), q).tolist() == [5039, 5119, 5199]      # slots 5197..5199: row 79 of columns 62..64
    bits = fec.encode_frame(F.payload(4))
    assert bits.shape == (5200,) and bits.dtype == np.uint8
    assert np.array_equal(bits[80 * np.arange(65)], fec.sync_vector())
    assert not bits[np.setdiff1d(np.arange(5200), q)].any()


def test_differential():
    assert fec.differential([1, 0, 1, 1, 0]).tolist() == [1, 1, 0, 1, 1]
    assert fec.differential([1, 0, 1, 1, 0], start=1).tolist() == [0, 0, 1, 0, 0]


def test_diff_edges():
    for n in (0, 19):
        assert fec.diff_np(np.ones(n, dtype=np.int8)).shape == (0,)
    assert fec.diff_np(np.full(20, -128, dtype=np.int8)).tolist() == [-127]          # |10 * -128| / 10 = 128, limited
    assert fec.diff_np(np.full(21, 127, dtype=np.int8)).tolist() == [-127, -127]
    r = np.concatenate((np.full(10, 90), np.full(10, -90))).astype(np.int8)
    assert fec.diff_np(r).tolist() == [90]                                          # a phase flip: channel bit 1
    r = np.concatenate((np.tile([5, -5], 5), np.full(10, 90))).astype(np.int8)
    assert fec.diff_np(r).tolist() == [0]                                           # S = 0 on one side
    r = np.concatenate((np.full(10, 7), np.full(10, -100))).astype(np.int8)
    assert fec.diff_np(r).tolist() == [7]                                           # the smaller of the two, 70 // 10


def test_encode_then_decode_returns_the_data(clean):
    data, r, D, p = clean
    frames, starts, corrected, errors = fec.frames_np(D)
    assert starts.tolist() == [[p, starts[0, 1], 65]] and starts[0, 1] == 65 * 90
    assert np.array_equal(frames, data[None]) and corrected.tolist() == [0] and errors.tolist() == [[0, 0]]
    assert fec.frame_header(frames[0]) == dict(sat_id=int(data[0]) >> 6, frame_type=int(data[0]) & 0x3F)


def test_viterbi_on_a_clean_frame_returns_the_sent_bits(clean):
    data, r, D, p = clean
    block, corrected = fec.viterbi_np(D, p, 0)
    assert np.array_equal(block, fec.rs_block(data)) and corrected == 0
    for bad in ((-1, 0), (len(D) - fec.SPAN + 1, 0), (p, 2)):
        with pytest.raises(ValueError):
            fec.viterbi_np(D, *bad)


def test_two_frames_sixty_thousand_symbols_apart():
    a, b = F.payload(5), F.payload(6)
    r = F.symbols(7, 6000 + fec.CHANNEL_BITS + 2, [(1, a, False), (6001, b, False)], lead=LEAD)
    frames, starts, corrected, errors = fec.frames_np(fec.diff_np(r))
    assert starts[:, 0].tolist() == [F.position(LEAD, 1), F.position(LEAD, 1) + 60000] and starts[:, 2].tolist() == [65, 65]
    assert np.array_equal(frames, np.stack((a, b))) and not corrected.any() and not errors.any()


def test_inverted_polarity_returns_the_same_bytes():
    data = F.payload(8)
    r = F.symbols(9, fec.CHANNEL_BITS + 4, [(2, data, True)], lead=3)
    frames, starts, corrected, errors = fec.frames_np(fec.diff_np(r))
    assert starts.tolist() == [[F.position(3, 2), -65 * 90, 65]]
    assert np.array_equal(frames, data[None]) and corrected.tolist() == [0] and errors.tolist() == [[0, 0]]


def test_noisy_frame_decodes():
    data = F.payload(10)
    r = F.symbols(11, fec.CHANNEL_BITS + 4, [(2, data, False)], lead=LEAD, sigma=90.0)
    frames, starts, corrected, errors = fec.frames_np(fec.diff_np(r))
    print("sigma 90: score %s, corrected %s, rs errors %s" % (starts[:, 2].tolist(), corrected.tolist(), errors.tolist()))
    assert starts[:, 0].tolist() == [F.position(LEAD, 2)]
    assert np.array_equal(frames, data[None]) and np.all(errors >= 0)
    # Q(900 / (90 sqrt 10)) = 8e-4 per bit sum, two sums per channel bit: 8 of 5132 expected; none is impossible, 100 too
    assert 0 < corrected[0] < 100


def test_random_symbols_give_nothing():
    r = F.rng(12).integers(-128, 128, 60000).astype(np.int8)
    frames, starts, corrected, errors = fec.frames_np(fec.diff_np(r))
    assert frames.shape == (0, 256) and starts.shape == (0, 3) and corrected.shape == (0,) and errors.shape == (0, 2)


def test_frame_starts_guard_and_ties():
    c = np.array([[100, 500, 60], [105, -700, 58], [110, 700, 58], [121, 10, 54], [300, -5, 54], [301, 5, 54]])
    assert fec.frame_starts(c[::-1])[:, 0].tolist() == [105, 121, 300]   # 110 ties with 105; 121 is 11 from 110; 300 before 301
    assert fec.frame_starts(np.zeros((0, 3))).shape == (0, 3)


def test_reed_solomon_shortening():
    g = F.rng(13)
    data = F.payload(14)
    blk = fec.rs_block(data)
    for c in range(2):                                            # each codeword is one of the (255,223) code behind 95 zeros
        word = np.concatenate((np.zeros(95, dtype=np.uint8), blk[c::2]))
        assert not lrpt.rs_syndromes(word).any() and np.array_equal(blk[c::2][:128], data[c::2])
    got = np.stack((blk, blk, blk))
    got[0, 2 * g.choice(160, 16, replace=False)] ^= 0x41          # codeword 0: sixteen errors
    got[1, 1 + 2 * g.choice(160, 17, replace=False)] ^= 0x41      # codeword 1: seventeen
    unit = np.zeros(223, dtype=np.uint8)
    unit[40] = 1
    got[2, 0::2] ^= lrpt.rs_encode(unit)[95:]                     # one byte, at the padded position 40, from a full-length codeword
    frames, errors = fec.reed_solomon_np(got)
    assert errors.tolist() == [[16, 0], [0, -1], [-1, 0]]
    assert np.array_equal(frames[0], data) and np.array_equal(frames[1, 0::2], data[0::2])
    assert np.array_equal(frames[1, 1::2], got[1, 1::2][:128]) and np.array_equal(frames[2, 0::2], got[2, 0::2][:128])
