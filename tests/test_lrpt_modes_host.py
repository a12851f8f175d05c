"""The Meteor-M N2-x modes of DESIGN.md section 4.18 in lrpt.py's NumPy restatement alone (no GPU): NRZ-M, the differential marker
template, the convolutional interleaver, the 0x27 marker and its lock, the soft-symbol file, and the restatement end to end."""
import numpy as np
import pytest

import _lrpt_modes
from directdemod_amd import lrpt


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@pytest.mark.parametrize("prev", [0, 1])
def test_nrzm_round_trip(prev):
    d = _rng(500 + prev).integers(0, 2, 1000, dtype=np.uint8)
    m = lrpt.nrzm_encode(d, prev)
    assert m[0] == prev ^ d[0] and np.array_equal(m[1:], m[:-1] ^ d[1:])
    got = lrpt.nrzm_decode(m)
    assert got[0] == 0 and np.array_equal(got[1:], d[1:])
    assert len(lrpt.nrzm_encode([])) == 0 and len(lrpt.nrzm_decode([])) == 0


def _word(code):
    return int("".join(str(int(b)) for b in code), 2)


def test_nrzm_template_is_its_definition():
    asm = np.unpackbits(lrpt.ASM)
    assert _word(lrpt.encode(asm)) == lrpt.ASM_ENCODED
    assert _word(lrpt.encode(lrpt.nrzm_encode(asm, 0))) == lrpt.ASM_ENCODED_NRZM == 0x03B10B02F33D2076
    # with the level 1 before the marker every bit that does not depend on the encoder's start state is the complement: the same
    # template under hypothesis h ^ 2
    other = lrpt.encode(lrpt.nrzm_encode(asm, 1))
    mine = lrpt._asm_code_bits(lrpt.ASM_ENCODED_NRZM)
    assert np.array_equal(other[lrpt.ASM_SKIP:], 1 - mine[lrpt.ASM_SKIP:])
    assert np.array_equal(lrpt.encode(lrpt.nrzm_encode(asm, 1), state=63), 1 - mine)


@pytest.mark.parametrize("B,M", [(36, 8), (36, 2048), (1, 5), (72, 1)])
def test_interleaver_round_trip(B, M):
    x = _rng(510).integers(0, 2, 2 * 72 * 41 + 6, dtype=np.uint8)
    y = lrpt.interleave_np(x, B, M)
    assert len(y) == len(x) + B * M * (B - 1) and y.sum() == x.sum()
    assert np.array_equal(lrpt.deinterleave_np(y, B, M), x)
    assert len(lrpt.deinterleave_np(y[:B * M * (B - 1)], B, M)) == 0
    assert len(lrpt.deinterleave_np(y[:B * M * (B - 1) + 3], B, M)) == 2          # rounded down to even
    n = np.arange(len(x))
    assert np.array_equal(y[n + B * M * (n % B)], x)


def test_interleaver_rejects():
    for B, M in ((0, 1), (5, 1), (36, -1), (144, 1)):
        with pytest.raises(ValueError):
            lrpt.interleave_np(np.zeros(10, dtype=np.uint8), B, M)
        with pytest.raises(ValueError):
            lrpt.deinterleave_np(np.zeros(10, dtype=np.uint8), B, M)


def test_marker_images_are_distinct():
    mark = 64 * (2 * lrpt.marker_bits().astype(np.int32) - 1)
    images = set()
    for h in range(8):
        a, b = lrpt.hypothesis(mark[0::2], mark[1::2], h)
        images.add(tuple((np.stack((a, b), axis=1).ravel() > 0).tolist()))
    assert len(images) == 8
    assert lrpt.add_markers_np(np.ones(100, dtype=np.uint8)).tolist() == ([0, 0, 1, 0, 0, 1, 1, 1] + [1] * 72
                                                                           + [0, 0, 1, 0, 0, 1, 1, 1] + [1] * 28 + [0] * 44)


def test_marker_scores_of_a_clean_stream():
    bits = lrpt.add_markers_np(_rng(520).integers(0, 2, 72 * 30, dtype=np.uint8))
    soft = (50 * (2 * np.concatenate((np.zeros(2 * 7, dtype=np.uint8), bits)).astype(np.int32) - 1)).astype(np.int8)
    nsym = len(soft) // 2
    sc = lrpt.deint_scores_np(soft, nsym, seg=4)
    assert sc.shape == (-(-nsym // 160), 40, 8) and sc[:, 7, 0].sum() == 8 * 30
    lock = lrpt.deint_lock(sc, nsym, seg=4)
    assert (lock["offset"], lock["hypothesis"], lock["score"], lock["markers"], lock["groups"], lock["locked"]) == (7, 0, 240, 30, 30, True)
    assert lock["info"]["markers"].tolist() == [4] * 7 + [2] and lock["info"]["score"].tolist() == [32] * 7 + [16]
    # the segments' own best: the lock where four markers were counted; two markers can be tied by chance
    assert np.all(lock["info"]["offset"][:7] == 7) and np.all(lock["info"]["hypothesis"][:7] == 0)
    assert lock["info"]["best_score"].tolist() == [32] * 7 + [16]
    # every symbol whose marker fits is counted once per hypothesis and once only
    assert lrpt.deint_scores_np(np.full(2 * 43, 1, dtype=np.int8), 43).shape == (1, 40, 8)
    assert lrpt.deint_scores_np(soft, 0).shape == (0, 40, 8) and not lrpt.deint_scores_np(soft, 3).any()
    assert not lrpt.deint_lock(lrpt.deint_scores_np(soft, 3), 3)["locked"]


@pytest.fixture(scope="module")
def four_frames():
    return _lrpt_modes.random_bodies(530, 4)


@pytest.mark.parametrize("hyp", range(8))
def test_restatement_end_to_end(four_frames, hyp):
    """4 frames from bit 3000 of the first, differential and interleaved at (36, 8), behind 17 random symbols, sent under each
    hypothesis: the lock is (17, that hypothesis), and the three whole frames decode to their bodies"""
    s = _lrpt_modes.stream(four_frames, 531, differential=True, interleaved=True, branches=36, delay=8, start=3000, prefix=17, hyp=hyp)
    lock = lrpt.deint_lock(lrpt.deint_scores_np(s["soft"], s["nsym"]), s["nsym"])
    assert (lock["offset"], lock["hypothesis"], lock["locked"]) == (17, hyp, True)
    assert lock["score"] >= 0.99 * 8 * lock["markers"]                           # amplitude 64 / sigma 16: four sigma
    soft = lrpt.deint_np(s["soft"], s["nsym"], lock["offset"], lock["hypothesis"], 36, 8)
    nsym = len(soft) // 2
    assert nsym == 36 * lock["groups"] - 18 * 8 * 35
    starts = lrpt.frame_starts(lrpt.asm_candidates_np(soft, nsym, template=lrpt.ASM_ENCODED_NRZM), nsym)
    assert starts[:, 0].tolist() == s["starts"][1:] and set(starts[:, 1].tolist()) <= {0, 2} and np.all(starts[:, 2] >= 50)
    for (p, h, _), body in zip(starts, four_frames[1:]):
        bits = lrpt.viterbi_blocks(soft, nsym, int(p), int(h), lrpt.FRAME_BITS)
        got, asm_errors, _ = lrpt.finish_nrzm_np(bits, soft, nsym, int(p), int(h))
        assert asm_errors == 0 and np.array_equal(got, body)
        # h and h ^ 2 decode to the same data
        other = lrpt.viterbi_blocks(soft, nsym, int(p), int(h) ^ 2, lrpt.FRAME_BITS)
        assert np.array_equal(lrpt.finish_nrzm_np(other, soft, nsym, int(p), int(h) ^ 2)[0], body)


def test_soft_file_round_trip(tmp_path):
    soft = _rng(540).integers(-128, 128, 2 * 501, dtype=np.int8)
    path = tmp_path / "pass.s"
    lrpt.write_soft(path, soft)
    assert path.stat().st_size == 1002 and np.array_equal(lrpt.read_soft(path), soft)
    with open(path, "ab") as f:
        f.write(b"\x7f")
    got = lrpt.read_soft(str(path))
    assert got.dtype == np.int8 and np.array_equal(got, soft)                    # the odd byte is dropped
    for bad in (soft[:-1], soft.astype(np.int16)):
        with pytest.raises(ValueError):
            lrpt.write_soft(path, bad)
