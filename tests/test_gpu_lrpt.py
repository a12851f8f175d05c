"""The LRPT channel decoder on the device (dd_lrpt_soft / _asm_search / _viterbi / _finish, decode_meteorm2.getFrames) against
lrpt.py's NumPy restatement of DESIGN.md section 4.14.  Every stage is integer arithmetic and is compared exactly, at the smallest
shapes that reach each edge: a length off the workgroup size, the shortest streams the marker search accepts, a block with no, a
short and the full warm-up and tail, ties, -128 under a negating hypothesis, and decisions far from clean (amplitude 60 / sigma 60:
about 16 % of the channel bits wrong)."""
import numpy as np
import pytest

import _lrpt
from directdemod_amd import lrpt

pytestmark = pytest.mark.gpu
INVERSE = {h: next(g for g in range(8) if all(int(v) == w for v, w in zip(lrpt.hypothesis(*lrpt.hypothesis(3, 5, h), g), (3, 5))))
           for h in range(8)}


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def _dev(hip, a):
    return hip.DevArray.from_host(np.ascontiguousarray(a))


# ------------------------------------------------------------------ dd_lrpt_soft
def test_soft_edges(hip):
    v = np.array([0.0, -0.0, 0.5, -0.5, 1.9, -1.9, 2.0, -2.0, 3.9, -3.9, 253.9, -253.9, 254, -254, 256, -256, 300, -300, 1e9, -1e9])
    want = [0, 0, 1, -1, 1, -1, 1, -1, 1, -1, 126, -126, 127, -127, 127, -128, 127, -128, 127, -128]
    rng = np.random.Generator(np.random.PCG64(3))
    sym = np.concatenate((v + 1j * v[::-1], 300.0 * (rng.standard_normal(583) + 1j * rng.standard_normal(583))))
    assert len(sym) % 256 and len(sym) > 512
    got = lrpt.soft_symbols(_dev(hip, sym.astype(np.complex128))).to_host()
    assert got.dtype == np.int8 and got[0:40:2].tolist() == want and got[1:40:2].tolist() == want[::-1]
    assert np.array_equal(got, lrpt.soft_np(sym))
    assert lrpt.soft_symbols(hip.DevArray(0, np.complex128)).n == 0


# ------------------------------------------------------------------ dd_lrpt_asm_search
@pytest.fixture(scope="module")
def three_frames():
    """three frames from bit 5000 of the first, amplitude 60 / sigma 30: (soft int8[2 n], nsym, the markers' symbols)"""
    rng = np.random.Generator(np.random.PCG64(4))
    bodies = rng.integers(0, 256, size=(4, 1020), dtype=np.uint8)
    code = lrpt.encode(_lrpt.frames_bits(bodies)).reshape(-1, 2)[5000:5000 + 3 * 8192]
    soft = np.clip(_lrpt.noisy_soft(code, 60.0, 30.0, 5), -127, 127).astype(np.int8)
    return soft, len(code), [8192 * i - 5000 for i in (1, 2, 3)]


@pytest.mark.parametrize("g", range(8))
def test_asm_each_hypothesis(hip, three_frames, g):
    soft, nsym, marks = three_frames
    a, b = lrpt.hypothesis(soft[0::2], soft[1::2], g)                 # the channel's distortion; INVERSE[g] undoes it
    dist = np.stack((a, b), axis=1).ravel().astype(np.int8)
    got = lrpt.asm_candidates(_dev(hip, dist), nsym)
    want = lrpt.asm_candidates_np(dist, nsym)
    assert np.array_equal(got, want)
    found = {(int(p), int(h)) for p, h, _ in got}
    assert all((p, INVERSE[g]) in found for p in marks)
    assert lrpt.frame_starts(got, nsym)[:, :2].tolist() == [[p, INVERSE[g]] for p in marks[:2]]      # the third does not fit


@pytest.mark.parametrize("nsym", [31, 32, 33])
def test_asm_shortest_streams(hip, nsym):
    e = np.array([(lrpt.ASM_ENCODED >> (63 - j)) & 1 for j in range(64)], dtype=np.int8)
    soft = np.concatenate((50 * (2 * e - 1), [-50, 50, 50, -50])).astype(np.int8)[:2 * nsym]
    got = lrpt.asm_candidates(_dev(hip, soft), nsym)
    assert np.array_equal(got, lrpt.asm_candidates_np(soft, nsym))
    assert got.tolist() == ([] if nsym == 31 else [[0, 0, 52]])


def test_asm_cap_smaller_than_count(hip, three_frames):
    soft, nsym, _ = three_frames
    want = lrpt.asm_candidates_np(soft, nsym, min_score=36)
    cap = 5
    assert len(want) > 4 * cap
    cand = _dev(hip, np.full(3 * (cap + 16), -7, dtype=np.int64))
    cnt = _dev(hip, np.array([99], dtype=np.uint64))
    hip.check(hip.lib().dd_lrpt_asm_search(_dev(hip, soft).ptr, nsym, 36, cap, cand.ptr, cnt.ptr, None))
    assert int(cnt.to_host()[0]) == len(want)
    c = cand.to_host()
    assert np.all(c[3 * cap:] == -7)
    rows = {tuple(r) for r in want.tolist()}
    assert all(tuple(r) in rows for r in c[:3 * cap].reshape(cap, 3).tolist())
    assert len({tuple(r) for r in c[:3 * cap].reshape(cap, 3).tolist()}) == cap


# ------------------------------------------------------------------ dd_lrpt_viterbi
@pytest.fixture(scope="module")
def noisy():
    """1500 symbols of encoded random bits at amplitude 60 / sigma 60: (sent bits, soft)"""
    rng = np.random.Generator(np.random.PCG64(6))
    sent = rng.integers(0, 2, 1500, dtype=np.uint8)
    soft = _lrpt.noisy_soft(lrpt.encode(sent).reshape(-1, 2), 60.0, 60.0, 7)
    wrong = np.mean((soft > 0) != lrpt.encode(sent))
    assert 0.13 < wrong < 0.19                                      # Q(1) = 15.9 %
    return sent, soft


def _viterbi(hip, soft, nsym, spans, nbits):
    packed = lrpt.viterbi(_dev(hip, soft), nsym, spans, nbits).to_host()
    return np.unpackbits(packed).reshape(len(spans), nbits)


@pytest.mark.parametrize("p,nbits,nsym", [
    (0, 512, 512),                # no warm-up, no tail
    (5, 512, 5 + 512 + 7),        # short warm-up and tail
    (200, 1024, 1500),            # full warm-up, two blocks, full tail
    (128, 512, 128 + 512 + 128),  # exactly the full warm-up and tail
    (0, 1024, 1024),              # the second block's tail is missing, the first block's warm-up too
])
def test_viterbi_block_edges(hip, noisy, p, nbits, nsym):
    _, soft = noisy
    s = soft[:2 * nsym]
    got = _viterbi(hip, s, nsym, [(p, 0)], nbits)[0]
    assert np.array_equal(got, lrpt.viterbi_blocks(s, nsym, p, 0, nbits))


def test_viterbi_noisy_stream_decodes(hip, noisy):
    sent, soft = noisy
    got = _viterbi(hip, soft, 1500, [(200, 0)], 1024)[0]
    assert np.array_equal(got, lrpt.viterbi_blocks(soft, 1500, 200, 0, 1024))
    assert np.mean(got != sent[200:1224]) < 0.16                   # it decodes: fewer bits wrong than the channel delivered


def test_viterbi_two_spans_two_hypotheses(hip, noisy):
    _, soft = noisy
    spans = [(200, 5), (310, 3), (0, 7)]
    got = _viterbi(hip, soft, 1500, spans, 512)
    for row, (p, h) in zip(got, spans):
        assert np.array_equal(row, lrpt.viterbi_blocks(soft, 1500, p, h, 512)), (p, h)


@pytest.mark.parametrize("h", range(8))
def test_viterbi_all_ties(hip, h):
    soft = np.zeros(2 * 700, dtype=np.int8)
    got = _viterbi(hip, soft, 700, [(100, h)], 512)[0]
    assert not got.any()
    assert np.array_equal(got, lrpt.viterbi_blocks(soft, 700, 100, h, 512))


@pytest.mark.parametrize("h", [1, 2, 3, 6])
def test_viterbi_minus_128_negated(hip, h):
    rng = np.random.Generator(np.random.PCG64(8))
    sent = rng.integers(0, 2, 640, dtype=np.uint8)
    code = 127 * (2 * lrpt.encode(sent).astype(np.int32) - 1)
    flip = np.repeat(rng.random(640) < 0.1, 2)
    a, b = lrpt.hypothesis(*np.where(flip, -code, code).reshape(-1, 2).T, INVERSE[h])     # what the channel delivers, +-127
    soft = np.stack((a, b), axis=1).ravel()
    soft = np.where(soft < 0, -128, soft).astype(np.int8)           # every negative value is -128: 128 under a negating hypothesis
    assert set(soft.tolist()) == {-128, 127}
    got = _viterbi(hip, soft, 640, [(64, h)], 512)[0]
    assert np.array_equal(got, lrpt.viterbi_blocks(soft, 640, 64, h, 512))


def test_viterbi_bad_arguments(hip, noisy):
    _, soft = noisy
    d = _dev(hip, soft)
    for spans, nbits in (([(0, 0)], 500), ([(0, 0)], 0), ([(0, 8)], 512), ([(0, -1)], 512), ([(989, 0)], 512), ([(-1, 0)], 512),
                         ([(0, 0), (1200, 0)], 512)):
        with pytest.raises(ValueError):
            lrpt.viterbi(d, 1500, spans, nbits)
    assert lrpt.viterbi(d, 1500, [], 512).n == 0


# ------------------------------------------------------------------ dd_lrpt_finish
@pytest.fixture(scope="module")
def one_frame():
    """a frame from symbol 150 of 8192 + 300, amplitude 60, no noise: (body, soft)"""
    rng = np.random.Generator(np.random.PCG64(9))
    body = rng.integers(0, 256, size=(1, 1020), dtype=np.uint8)
    bits = np.concatenate((rng.integers(0, 2, 150, dtype=np.uint8), _lrpt.frames_bits(body), rng.integers(0, 2, 150, dtype=np.uint8)))
    return body[0], (60 * (2 * lrpt.encode(bits).astype(np.int32) - 1)).astype(np.int8)


def _finish(hip, soft, nsym, spans):
    ds = _dev(hip, soft)
    bits = lrpt.viterbi(ds, nsym, spans)
    bodies, info = lrpt.finish(bits, ds, nsym, spans)
    rows = np.unpackbits(bits.to_host()).reshape(len(spans), 8192)
    for row, (p, h), body, inf in zip(rows, spans, bodies, info):
        assert np.array_equal(row, lrpt.viterbi_blocks(soft, nsym, p, h, 8192))
        wb, wa, wc = lrpt.finish_np(row, soft, nsym, p, h)
        assert np.array_equal(body, wb) and (int(inf[0]), int(inf[1])) == (wa, wc)
        assert int(inf[2]) == lrpt.vcdu_header(wb)["vcid"]
    return bodies, info


def test_finish_clean_flipped_and_inverted(hip, one_frame):
    body, soft = one_frame
    nsym = len(soft) // 2
    rng = np.random.Generator(np.random.PCG64(10))
    hit = np.sort(rng.choice(np.arange(2 * 160, 2 * (150 + 8192) - 20), size=60, replace=False))
    hit = hit[np.r_[True, np.diff(hit) > 40]]                        # isolated channel errors: each one is corrected
    bad = soft.copy()
    bad[hit] = -bad[hit]
    both = np.concatenate((soft, bad))                               # the flipped copy starts at symbol nsym
    bodies, info = _finish(hip, both, 2 * nsym, [(150, 0), (nsym + 150, 0), (150, 2)])
    assert np.array_equal(bodies[0], body) and info[0, :2].tolist() == [0, 0]
    assert np.array_equal(bodies[1], body) and info[1, :2].tolist() == [0, len(hit)]
    assert info[2, 0] == 32 and info[2, 1] == 0                      # both polynomials have odd weight: the 180 degree stream is
    assert np.array_equal(bodies[2], ~body)                          # the code of the complemented bits


def test_finish_bad_arguments(hip, one_frame):
    _, soft = one_frame
    nsym = len(soft) // 2
    ds = _dev(hip, soft)
    bits = lrpt.viterbi(ds, nsym, [(150, 0)])
    for spans in ([(150, 8)], [(301, 0)], [(-1, 0)]):
        with pytest.raises(ValueError):
            lrpt.finish(bits, ds, nsym, spans)


# ------------------------------------------------------------------ decode_meteorm2.getFrames
def test_get_frames_end_to_end(hip):
    from directdemod_amd import decode_meteorm2, source
    raw, bodies, start = _lrpt.case("a")
    obj = decode_meteorm2.decode_meteorm2(source.IQarray(raw, _lrpt.FS), 0)
    frames, info = obj.getFrames, obj.frameInfo
    assert frames.dtype == np.uint8 and frames.shape == (len(info), 1020)
    assert np.all(np.diff(info["symbol"]) > 0)
    late = np.nonzero(info["symbol"] >= 9000)[0]
    assert info["symbol"][late].tolist() == [_lrpt.FIRST + 8192 * i for i in range(10)]
    assert np.array_equal(frames[late], bodies[2:12])
    assert not info["asm_errors"][late].any() and np.all(info["hypothesis"][late] == _lrpt.HYP)
    assert np.all(info["asm_score"][late] >= lrpt.MIN_SCORE) and np.all(info["corrected"][late] < 2 * 8186 // 100)
    w = obj.walker()
    aidx = w.view("aidx").to_host()
    assert np.array_equal(info["sample"], aidx[info["symbol"]])
    for b, r in zip(frames, info):
        hd = lrpt.vcdu_header(b)
        assert (hd["vcid"], hd["counter"]) == (int(r["vcid"]), int(r["counter"]))
    # where the frames lie, from the sent code bits and the device's own soft symbols rather than from the decoder
    n = raw.shape[0]
    _, _, code = _lrpt.stream(_lrpt.CASES["a"]["seed"], n * 9 // 256 + 2)
    soft = lrpt.soft_symbols(w.view("sym")).to_host()
    lag, hyp = _lrpt.aligned(soft, w.nsym, code)
    assert hyp == _lrpt.HYP and 8192 * 2 - start - lag == _lrpt.FIRST
    # the reference's 120-bit sync is absent from this recording: getSyncs is what it is without the frame decoder
    assert obj.getSyncs == [] and obj.useful == 0
    assert obj.getFrames is frames
    for k in ("lrpt_soft", "lrpt_asm", "lrpt_viterbi", "lrpt_finish", "walk", "lim"):
        assert obj.timings[k] >= 0.0
