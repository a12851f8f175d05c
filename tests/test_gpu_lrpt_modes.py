"""The Meteor-M N2-x modes on the device (dd_lrpt_asm_search_t / _finish_nrzm / _deint_scores / _deinterleave, decode_lrpt) against
lrpt.py's NumPy restatement of DESIGN.md section 4.18.  Every quantity is an integer and every comparison is exact.  Shapes: the
shortest streams a marker fits in, the segment boundary of the marker score and a partial last segment, segments shorter than a
workgroup, every hypothesis at the first, second and last offset, interleavers of one branch, of no delay and of 72 branches, a
stream that does not fill the branches, and one gather at the full depth of (36, 2048)."""
import os

import numpy as np
import pytest

import _lrpt
import _lrpt_modes
from directdemod_amd import lrpt

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def _dev(hip, a):
    return hip.DevArray.from_host(np.ascontiguousarray(a))


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "lrpt_a.npz"))
    return g["soft"], int(g["nsym"])


@pytest.fixture(scope="module")
def differential():
    """four frames from bit 3000 of the first behind 150 random symbols, NRZ-M coded: three whole frames"""
    bodies = _lrpt_modes.random_bodies(600, 4)
    return bodies, _lrpt_modes.stream(bodies, 601, differential=True, start=3000, prefix=150)


# ------------------------------------------------------------------ dd_lrpt_asm_search_t
def _search_t(hip, soft, nsym, template, min_score=lrpt.MIN_SCORE, cap=1 << 12):
    cand = hip.DevArray(3 * cap, np.int64)
    cnt = _dev(hip, np.array([99], dtype=np.uint64))
    hip.check(hip.lib().dd_lrpt_asm_search_t(_dev(hip, soft).ptr, nsym, template, min_score, cap, cand.ptr, cnt.ptr, None), "asm_search_t")
    m = int(cnt.to_host()[0])
    c = cand.view(0, 3 * m).to_host().reshape(m, 3)
    return c[np.lexsort((c[:, 1], c[:, 0]))]


def test_asm_t_with_the_plain_template_is_asm_search(hip, golden):
    soft, nsym = golden
    for min_score in (lrpt.MIN_SCORE, 40):
        old = lrpt.asm_candidates(_dev(hip, soft), nsym, min_score=min_score)
        assert len(old) >= 10 and np.array_equal(_search_t(hip, soft, nsym, lrpt.ASM_ENCODED, min_score), old)


def test_asm_t_with_the_nrzm_template(hip, differential):
    _, s = differential
    got = lrpt.asm_candidates(_dev(hip, s["soft"]), s["nsym"], template=lrpt.ASM_ENCODED_NRZM)
    assert np.array_equal(got, lrpt.asm_candidates_np(s["soft"], s["nsym"], template=lrpt.ASM_ENCODED_NRZM))
    starts = lrpt.frame_starts(got, s["nsym"])
    assert starts[:, 0].tolist() == s["starts"][1:] and set(starts[:, 1].tolist()) <= {0, 2}
    assert len(lrpt.asm_candidates(_dev(hip, s["soft"]), s["nsym"])) == 0          # the plain template finds none of them
    for nsym in (31, 32, 33):                                                     # the shortest streams, at a low bar
        want = lrpt.asm_candidates_np(s["soft"], nsym, min_score=20, template=lrpt.ASM_ENCODED_NRZM)
        assert np.array_equal(_search_t(hip, s["soft"][:2 * nsym], nsym, lrpt.ASM_ENCODED_NRZM, 20), want)
        assert len(want) == 0 if nsym == 31 else len(want) >= 1


# ------------------------------------------------------------------ dd_lrpt_finish_nrzm
def test_finish_nrzm_under_h_and_h_xor_2(hip, differential):
    bodies, s = differential
    soft, nsym = s["soft"], s["nsym"]
    ds = _dev(hip, soft)
    spans = [(p, h) for h in (0, 2) for p in s["starts"][1:]]
    bits = lrpt.viterbi(ds, nsym, spans)
    got, info = lrpt.finish(bits, ds, nsym, spans, nrzm=True)
    rows = np.unpackbits(bits.to_host()).reshape(len(spans), 8192)
    for row, (p, h), body, inf in zip(rows, spans, got, info):
        wb, wa, wc = lrpt.finish_nrzm_np(row, soft, nsym, p, h)
        assert np.array_equal(body, wb) and (int(inf[0]), int(inf[1])) == (wa, wc) and wa == 0
        assert int(inf[2]) == lrpt.vcdu_header(wb)["vcid"]
    assert np.array_equal(got[:3], bodies[1:]) and np.array_equal(got[3:], bodies[1:])
    # under h ^ 2 the decoder follows the complemented path, which is a code word too: as few channel bits are changed
    assert np.all(info[:, 1] < 40)
    # the plain finish of the same bits gives other bodies: the entry matters
    plain, _ = lrpt.finish(bits, ds, nsym, spans)
    assert not np.array_equal(plain[0], got[0])
    for bad in ([(s["starts"][1], 8)], [(nsym - 8191, 0)], [(-1, 0)]):
        with pytest.raises(ValueError):
            lrpt.finish(bits, ds, nsym, bad, nrzm=True)


# ------------------------------------------------------------------ dd_lrpt_deint_scores
@pytest.fixture(scope="module")
def marked():
    """3 * 10240 + 17 symbols: markers from symbol 5 on at amplitude 64 / sigma 16, with 0, -128 and 127 on marker positions"""
    nsym = 3 * 10240 + 17
    rng = _rng(610)
    bits = np.concatenate((rng.integers(0, 2, 10, dtype=np.uint8), lrpt.add_markers_np(rng.integers(0, 2, 72 * 770, dtype=np.uint8))))
    soft = np.clip(_lrpt.noisy_soft(bits.reshape(-1, 2)[:nsym], 64.0, 16.0, 611), -127, 127).astype(np.int8)
    for k, v in enumerate((0, -128, 127, 0, 0, -128, 127, -128)):               # the first marker's eight values, then scattered ones
        soft[2 * 5 + k] = v
    hit = 2 * (5 + 40 * rng.integers(1, 760, 300)) + rng.integers(0, 8, 300)
    soft[hit] = rng.choice(np.array([0, -128, 127], dtype=np.int8), 300)
    assert len(soft) == 2 * nsym
    return soft


@pytest.mark.parametrize("seg", [1, 256])
@pytest.mark.parametrize("nsym", [0, 3, 4, 39, 40, 43, 44, 10240 - 1, 10240, 10240 + 1, 3 * 10240 + 17])
def test_deint_scores(hip, marked, nsym, seg):
    soft = marked[:2 * nsym]
    got = lrpt.deint_scores(_dev(hip, soft if nsym else np.zeros(2, dtype=np.int8)), nsym, seg)
    want = lrpt.deint_scores_np(soft, nsym, seg)
    assert got.shape == want.shape == (-(-nsym // (40 * seg)), 40, 8) and np.array_equal(got, want)
    if nsym >= 10240 - 1:
        lock = lrpt.deint_lock(got, nsym, seg)
        assert (lock["offset"], lock["hypothesis"], lock["locked"]) == (5, 0, True) and lock["groups"] == (nsym - 5) // 40
        assert lock["info"]["markers"].sum() == lock["markers"] == (nsym - 4 - 5) // 40 + 1


def test_deint_scores_bad_arguments(hip, marked):
    d = _dev(hip, marked[:200])
    for nsym, seg in ((100, 0), (100, -1), (-1, 256), (100, (1 << 24) + 1)):
        with pytest.raises(ValueError):
            hip.check(hip.lib().dd_lrpt_deint_scores(d.ptr, nsym, seg, d.ptr, None))


# ------------------------------------------------------------------ dd_lrpt_deinterleave
def _deinterleave(hip, soft, nsym, o, h, B, M):
    got = lrpt.deint(_dev(hip, soft), nsym, o, h, B, M).to_host()
    want = lrpt.deint_np(soft, nsym, o, h, B, M)
    assert got.dtype == np.int8 and np.array_equal(got, want)
    return got


@pytest.fixture(scope="module")
def random_soft():
    """36 * 40960 = 1 474 560 random symbols over all of int8, -128 included: the (36, 2048) interleaver holds 36 * 2048 * 35 bits =
    1 433 600 symbols of stream, so this many let 2048 bits leave every branch"""
    return _rng(620).integers(-128, 128, 2 * 36 * 40960, dtype=np.int8)


@pytest.mark.parametrize("o", [0, 1, 39])
@pytest.mark.parametrize("h", range(8))
def test_deinterleave_every_hypothesis(hip, random_soft, h, o):
    nsym = 40 * 300 + 23                                   # 299 or 300 whole periods, more than one workgroup of output
    got = _deinterleave(hip, random_soft[:2 * nsym], nsym, o, h, 36, 8)
    assert len(got) == 72 * ((nsym - o) // 40) - 36 * 8 * 35


@pytest.mark.parametrize("B,M", [(36, 8), (1, 0), (72, 1), (1, 5), (2, 3)])
def test_deinterleave_branches_and_delays(hip, random_soft, B, M):
    nsym = 40 * 300 + 23
    got = _deinterleave(hip, random_soft[:2 * nsym], nsym, 7, 5, B, M)
    assert len(got) == (72 * 300 - B * M * (B - 1)) & ~1 and len(got) > 0
    # through the interleaver and back: what interleave_np spreads, the device gathers
    x = _rng(621).integers(-127, 128, 72 * 200, dtype=np.int8)
    y = lrpt.interleave_np(x, B, M)
    y = np.concatenate((y, np.zeros(-len(y) % 72, dtype=np.int8)))
    sent = np.concatenate((np.zeros((len(y) // 72, 8), dtype=np.int8), y.reshape(-1, 72)), axis=1).ravel()
    back = lrpt.deint(_dev(hip, sent), len(sent) // 2, 0, 0, B, M).to_host()
    assert np.array_equal(back[:len(x)], x)


def test_deinterleave_too_short_to_fill_the_branches(hip, random_soft):
    for nsym in (0, 39, 40 * 140, 40 * 140 + 39):           # 72 * 140 = 36 * 8 * 35 = 10080: exactly no bit comes out
        d = _dev(hip, random_soft[:max(2 * nsym, 2)])
        assert lrpt.deint(d, nsym, 0, 0, 36, 8).n == 0 and len(lrpt.deint_np(random_soft[:2 * nsym], nsym, 0, 0, 36, 8)) == 0
    assert lrpt.deint(_dev(hip, random_soft[:2 * 40 * 141]), 40 * 141, 0, 0, 36, 8).n == 72
    assert lrpt.deint(_dev(hip, random_soft[:2 * 40 * 141]), 40 * 141, 1, 0, 36, 8).n == 0


@pytest.mark.parametrize("h", [1, 2, 3, 5, 6, 7])
def test_deinterleave_minus_128_negated_is_127(hip, h):
    nsym = 40 * 3
    soft = np.full(2 * nsym, -128, dtype=np.int8)
    got = _deinterleave(hip, soft, nsym, 0, h, 1, 0)
    a, b = lrpt.hypothesis(-128, -128, h)
    assert 128 in (int(a), int(b)) and set(got.tolist()) == {127 if int(v) == 128 else -128 for v in (a, b)}
    assert got[:2].tolist() == [min(int(a), 127), min(int(b), 127)]


def test_deinterleave_full_depth(hip, random_soft):
    nsym = len(random_soft) // 2
    got = _deinterleave(hip, random_soft, nsym, 17, 3, lrpt.INTERLEAVER_BRANCHES, lrpt.INTERLEAVER_DELAY)
    assert len(got) == 72 * ((nsym - 17) // 40) - 36 * 2048 * 35 >= 36 * 2048 - 72


def test_deinterleave_bad_arguments(hip, random_soft):
    d = _dev(hip, random_soft[:2 * 4000])
    for o, h, B, M in ((-1, 0, 36, 8), (40, 0, 36, 8), (0, -1, 36, 8), (0, 8, 36, 8), (0, 0, 0, 8), (0, 0, 5, 8), (0, 0, 144, 8),
                       (0, 0, -36, 8), (0, 0, 36, -1)):
        with pytest.raises(ValueError):
            lrpt.deint(d, 4000, o, h, B, M)


# ------------------------------------------------------------------ decode_lrpt
def test_decode_lrpt_plain_on_the_reference_walk(hip, golden, tmp_path):
    from directdemod_amd import decode_lrpt
    soft, nsym = golden
    c = _lrpt.CASES["a"]
    bodies, _, _ = _lrpt.stream(c["seed"], int(round(c["seconds"] * _lrpt.FS)) * 9 // 256 + 2)
    obj = decode_lrpt.decode_lrpt(soft)
    frames, info = obj.getFrames, obj.frameInfo
    assert frames.dtype == np.uint8 and frames.shape == (len(info), 1020) and info.dtype == lrpt.INFO
    late = np.nonzero(info["symbol"] >= 9000)[0]
    assert info["symbol"][late].tolist() == [_lrpt.FIRST + 8192 * i for i in range(10)] and np.array_equal(frames[late], bodies[2:12])
    assert np.all(info["hypothesis"][late] == _lrpt.HYP) and not info["asm_errors"][late].any() and np.all(info["sample"] == -1)
    assert obj.locked is True and len(obj.deintInfo) == 0 and obj.deintInfo.dtype == lrpt.DEINT_INFO and obj.getFrames is frames
    assert obj.getVCDUs.shape == (len(frames), 892) and obj.rsInfo.dtype == lrpt.RS_INFO and obj.packetInfo.dtype == lrpt.PACKET_INFO
    assert obj.getImage.shape[1:] == (1568, 3) and obj.imageInfo.dtype == lrpt.IMAGE_INFO
    # a device array and a file give what the host array gives
    path = tmp_path / "a.s"
    lrpt.write_soft(path, soft)
    for other in (_dev(hip, soft), str(path), path):
        o = decode_lrpt.decode_lrpt(other)
        assert np.array_equal(o.getFrames, frames) and np.array_equal(o.frameInfo, info)
    for bad in (soft.astype(np.int16), soft.reshape(-1, 2), hip.DevArray(4, np.uint8)):
        with pytest.raises(TypeError):
            decode_lrpt.decode_lrpt(bad)
    with pytest.raises(ValueError):
        decode_lrpt.decode_lrpt(soft, interleaved=True, branches=5)
    with pytest.raises(ValueError):
        decode_lrpt.decode_lrpt(soft, apids=(64, 64, 65))


def test_decode_lrpt_of_get_soft_is_get_frames(hip):
    from directdemod_amd import decode_lrpt, decode_meteorm2, source
    raw, _, _ = _lrpt.case("a")
    ref = decode_meteorm2.decode_meteorm2(source.IQarray(raw, _lrpt.FS), 0)
    soft = ref.getSoft
    assert isinstance(soft, np.ndarray) and soft.dtype == np.int8 and len(soft) == 2 * ref.walker().nsym
    obj = decode_lrpt.decode_lrpt(soft)
    assert len(ref.getFrames) >= 10 and np.array_equal(obj.getFrames, ref.getFrames)
    names = [n for n in lrpt.INFO.names if n != "sample"]
    assert np.array_equal(obj.frameInfo[names], ref.frameInfo[names]) and np.all(ref.frameInfo["sample"] >= 0)
    assert obj.getPackets == ref.getPackets and np.array_equal(obj.getVCDUs, ref.getVCDUs)


@pytest.fixture(scope="module")
def picture():
    """a picture of 2 strip cycles in as many frames as it fills: (bodies, the packets completed in them, image_np of those)"""
    built, sent = _lrpt_modes.picture_frames(630, strips=2)
    return built["bodies"], sent, lrpt.image_np(sent)


@pytest.mark.parametrize("interleaved,prefix,hyp", [(False, 123, 6), (True, 57, 5)])
def test_decode_lrpt_picture(hip, picture, interleaved, prefix, hyp):
    from directdemod_amd import decode_lrpt
    bodies, sent, (want_img, want_info) = picture
    s = _lrpt_modes.stream(bodies, 631, differential=True, interleaved=interleaved, branches=36, delay=8, prefix=prefix, hyp=hyp)
    obj = decode_lrpt.decode_lrpt(s["soft"], differential=True, interleaved=interleaved, branches=36, delay=8)
    info = obj.frameInfo
    assert info["symbol"].tolist() == s["starts"] and len(s["starts"]) == len(bodies) >= 8
    assert np.array_equal(obj.getFrames, bodies) and not info["asm_errors"].any() and np.all(obj.rsInfo["ok"])
    assert set(info["hypothesis"].tolist()) <= ({0, 2} if interleaved else {hyp, hyp ^ 2})
    assert obj.getPackets == sent
    assert want_img.shape[0] == 16 and want_img.any() and len(want_info) >= 60
    assert np.array_equal(obj.getImage, want_img) and np.array_equal(obj.imageInfo, want_info)
    assert np.array_equal(obj.getChannel(65), want_img[:, :, 1])
    assert obj.locked is True
    if interleaved:
        lock, di = obj.lock, obj.deintInfo
        assert (lock["offset"], lock["hypothesis"]) == (prefix % 40, hyp) and lock["score"] >= 0.99 * 8 * lock["markers"]
        assert di.dtype == lrpt.DEINT_INFO and len(di) == -(-s["nsym"] // 10240) and di["markers"].sum() == lock["markers"]
        full = di["markers"] >= 16                        # a last segment of a few markers can be tied by chance
        assert full.sum() >= len(di) - 1 and np.all(di["offset"][full] == prefix % 40) and np.all(di["hypothesis"][full] == hyp)
        assert np.array_equal(di["score"][full], di["best_score"][full])
        for k in ("lrpt_deint_scores", "lrpt_deinterleave", "lrpt_soft", "lrpt_asm", "lrpt_viterbi", "lrpt_finish"):
            assert obj.timings[k] >= 0.0
        # without the differential decoding the same stream gives no frame
        assert len(decode_lrpt.decode_lrpt(s["soft"], interleaved=True, branches=36, delay=8).getFrames) == 0


def test_decode_lrpt_noise_is_not_locked(hip):
    from directdemod_amd import decode_lrpt
    soft = np.clip(40.0 * _rng(640).standard_normal(2 * 60000), -128, 127).astype(np.int8)
    obj = decode_lrpt.decode_lrpt(soft, differential=True, interleaved=True, branches=36, delay=8)
    assert obj.locked is False and obj.getFrames.shape == (0, 1020) and len(obj.frameInfo) == 0
    assert obj.getPackets == [] and obj.getImage.shape == (0, 1568, 3)
    lock = obj.lock
    assert lock["markers"] >= 1499 and 4 * lock["score"] < 3 * 8 * lock["markers"] and len(obj.deintInfo) == 6
