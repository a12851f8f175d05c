"""The LRPT channel decoder's definitions as lrpt.py restates them in NumPy, and its host stages: the check
values, frame_starts on a hand-made candidate list, the block-wise Viterbi decode against a whole-span decode and the sent bits, and
the whole restatement over the soft symbols of the reference's own symbol walk (tests/golden/lrpt_a.npz, tools/gen_golden.py --lrpt).

Where the frames of lrpt_a lie is not taken from the decoder: the received hard bits are aligned with the sent code bits (one lag and
one hypothesis agree over a 512-symbol window, all others sit near one half), and the sent frames' starts follow from the lag.  For
the recording of tests/_lrpt.py that is symbol 9159 + 8192 i under hypothesis 3."""
import os

import numpy as np
import pytest

import _lrpt
from directdemod_amd import lrpt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIRST, HYP = _lrpt.FIRST, _lrpt.HYP


def test_check_values():
    e = lrpt.encode(np.unpackbits(lrpt.ASM))
    assert int("".join(str(int(b)) for b in e), 2) == 0x035D49C24FF2686B == lrpt.ASM_ENCODED
    assert (~lrpt.ASM_ENCODED) & (2 ** 64 - 1) == 0xFCA2B63DB00D9794
    assert lrpt.pn_sequence(8).tobytes() == bytes.fromhex("FF480EC09A0D70BC")
    bits = np.unpackbits(lrpt.pn_sequence(1020))
    assert np.array_equal(bits[255:], bits[:-255])
    assert all(np.any(bits[d:510] != bits[:510 - d]) for d in range(1, 255))
    assert len(lrpt.pn_sequence()) == 1020


def test_encoder_state():
    rng = np.random.Generator(np.random.PCG64(1))
    bits = rng.integers(0, 2, 200, dtype=np.uint8)
    whole = lrpt.encode(bits)
    s = 0
    for k in range(100):
        s = ((int(bits[k]) << 6) | s) >> 1
    assert np.array_equal(lrpt.encode(bits[100:], s), whole[200:])


def test_hypotheses_have_inverses():
    a = np.array([-128, -5, 0, 7, 127])
    b = np.array([3, -128, 127, 0, -9])
    for h in range(8):
        x, y = lrpt.hypothesis(a, b, h)
        assert x.dtype == np.int32 and y.dtype == np.int32
        inv = [g for g in range(8) if all(np.array_equal(u, v) for u, v in zip(lrpt.hypothesis(x, y, g), (a, b)))]
        assert len(inv) == 1, (h, inv)
    assert lrpt.hypothesis(np.int8(-128), np.int8(1), 2)[0] == 128


def test_soft_np():
    v = np.array([0.0, -0.0, 0.5, -0.5, 1.9, -1.9, 2.0, -2.0, 3.9, -3.9, 253.9, -253.9, 254, -254, 256, -256, 300, -300, 1e9, -1e9])
    want = [0, 0, 1, -1, 1, -1, 1, -1, 1, -1, 126, -126, 127, -127, 127, -128, 127, -128, 127, -128]
    got = lrpt.soft_np(v + 1j * v[::-1])
    assert got.dtype == np.int8
    assert got[0::2].tolist() == want and got[1::2].tolist() == want[::-1]
    from directdemod_amd.symbolsync import lim
    assert got[0::2].tolist() == [lim(x / 2) for x in v]


def test_frame_starts():
    nsym = 30000
    c = np.array([
        (100, 2, 50), (100, 5, 50),           # a tie at one position: the lower h
        (1000, 1, 48), (1031, 1, 49),         # a neighbour 31 symbols on scores higher
        (2000, 0, 49), (2032, 0, 48),         # 32 symbols apart: both stay
        (3000, 4, 47), (3010, 4, 47),         # equal scores: the lower p
        (nsym - 8192, 3, 52),                 # fits exactly
        (nsym - 8191, 6, 52),                 # one symbol too close to the end, and it still suppresses nothing better
    ], dtype=np.int64)
    rng = np.random.Generator(np.random.PCG64(2))
    got = lrpt.frame_starts(c[rng.permutation(len(c))], nsym)
    assert got.tolist() == [[100, 2, 50], [1031, 1, 49], [2000, 0, 49], [2032, 0, 48], [3000, 4, 47], [nsym - 8192, 3, 52]]
    assert lrpt.frame_starts(np.zeros((0, 3), dtype=np.int64), nsym).shape == (0, 3)


def test_vcdu_header():
    h = lrpt.vcdu_header(bytes([0x40, 0x05, 0x12, 0x34, 0x56, 0x00]) + bytes(1014))
    assert h == dict(version=1, scid=0, vcid=5, counter=0x123456)


@pytest.mark.parametrize("seed", range(6))
def test_blocks_equal_whole_span_and_sent(seed):
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    nsym, p, nbits = 16984, 300, 8192
    sent = rng.integers(0, 2, nsym, dtype=np.uint8)
    soft = _lrpt.noisy_soft(lrpt.encode(sent).reshape(-1, 2), 90.0, 45.0, 200 + seed)
    blocks = lrpt.viterbi_blocks(soft, nsym, p, 0, nbits)
    whole = lrpt.viterbi_blocks(soft, nsym, p, 0, nbits, block=nbits)
    assert np.array_equal(blocks, whole)
    assert np.array_equal(blocks, sent[p:p + nbits])


def test_restatement_over_reference_walk():
    g = np.load(os.path.join(GOLDEN, "lrpt_a.npz"))
    soft, nsym = g["soft"], int(g["nsym"])
    assert soft.dtype == np.int8 and len(soft) == 2 * nsym
    p = _lrpt.CASES["a"]
    n = int(round(p["seconds"] * _lrpt.FS))
    assert n == int(g["n"]) and _lrpt.sha256(_lrpt.case("a")[0]) == str(g["sha256"])
    bodies, start, code = _lrpt.stream(p["seed"], n * 9 // 256 + 2)
    lag, hyp = _lrpt.aligned(soft, nsym, code)
    want = [8192 * i - start - lag for i in range(len(bodies))]
    want = [(i, q) for i, q in enumerate(want) if q >= 9000 and q + 8192 <= nsym]
    assert [i for i, _ in want] == list(range(2, 12)) and hyp == HYP
    assert [q for _, q in want] == [FIRST + 8192 * i for i in range(10)]

    starts = lrpt.frame_starts(lrpt.asm_candidates_np(soft, nsym), nsym)
    late = starts[starts[:, 0] >= 9000]
    assert late.tolist() == [[FIRST + 8192 * i, HYP, 52] for i in range(10)]
    for i, (q, h, _) in enumerate(late):
        bits = lrpt.viterbi_blocks(soft, nsym, int(q), int(h), 8192)
        body, asm_errors, corrected = lrpt.finish_np(bits, soft, nsym, int(q), int(h))
        assert asm_errors == 0
        assert np.array_equal(body, bodies[2 + i])
        assert 0 <= corrected < 2 * 8186 // 100                 # amp 40 / sigma 4: hardly a channel bit in error
