"""The Funcube frame decoder on the device (dd_fc_diff / _sync_search / _viterbi / _rs, funcube_fec.py's wrappers) stage by stage
against funcube_fec.py's NumPy restatement of DESIGN.md section 4.17, and decode_funcube.getFrames / frameInfo end to end.  All
arithmetic is integer and every comparison is exact.  The shapes are single frames and the lengths at which a kernel takes another
way: nothing to do, one output, one more than a workgroup."""
import numpy as np
import pytest

import _funcube
import _funcube_frames as F
from directdemod_amd import funcube_fec as fec
from directdemod_amd import lrpt

pytestmark = pytest.mark.gpu
SPAN = fec.SPAN                       # 51991 entries of D per frame


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def _dev(hip, a, dtype):
    """a device copy of `a` (at least one element is allocated, the view has len(a))"""
    a = np.ascontiguousarray(a, dtype=dtype)
    return hip.DevArray.from_host(a) if a.size else hip.DevArray(1, dtype).view(0, 0)


# ------------------------------------------------------------------ dd_fc_diff
def _diff_patterns(n):
    g = F.rng(100 + n)
    yield "random", g.integers(-128, 128, n).astype(np.int8)
    yield "low", np.full(n, -128, dtype=np.int8)
    yield "high", np.full(n, 127, dtype=np.int8)
    r = np.resize(np.array([5, -5], dtype=np.int8), n)               # every ten-symbol sum is 0 ...
    r[n // 2:] = 90                                                  # ... up to the middle
    yield "zero sums", r
    r = g.integers(-128, 128, n).astype(np.int8)
    r[:max(n - 25, 0):2] = -128                                      # sums of both signs next to runs at the limit
    yield "mixed", r


@pytest.mark.parametrize("n", [0, 19, 20, 21, 275, 276])
def test_diff(hip, n):
    m = max(n - 19, 0)
    for name, r in _diff_patterns(n):
        want = fec.diff_np(r)
        assert want.shape == (m,)
        soft = _dev(hip, F.pairs(r, n), np.int8)
        got = fec.diff(soft, n)
        assert got.n == m and got.dtype == np.int8 and np.array_equal(got.to_host(), want), name
        out = hip.DevArray.from_host(np.full(m + 16, 0x5A, dtype=np.int8))          # the tail beyond the output stays
        hip.check(hip.lib().dd_fc_diff(soft.ptr, n, out.ptr, None))
        o = out.to_host()
        assert np.array_equal(o[:m], want) and np.all(o[m:] == 0x5A), name
    with pytest.raises(ValueError):
        hip.check(hip.lib().dd_fc_diff(None, 20, None, None))
    with pytest.raises(ValueError):
        hip.check(hip.lib().dd_fc_diff(None, -1, None, None))


def test_soft_bits_from_complex_symbols(hip):
    g = F.rng(120)
    sym = (g.uniform(-300, 300, 300) + 1j * g.uniform(-300, 300, 300)).astype(np.complex128)
    sym[:8] = [0.4, -0.4, 1.9, -1.9, 255.9, -257.0, 0.0, 2.0]
    got = fec.soft_bits(hip.DevArray.from_host(sym))
    assert np.array_equal(got.to_host(), fec.soft_bits_np(sym)) and got.n == 281


# ------------------------------------------------------------------ dd_fc_sync_search
def _sync_d(npos, seed, frames=(), noise=3):
    """D of 51990 + npos entries: small noise, then the sync bits of (p, inverted, flipped sync bits) frames"""
    D = F.rng(seed).integers(-noise, noise + 1, SPAN - 1 + npos).astype(np.int8)
    for p, inverted, flips in frames:
        v = fec.sync_vector().copy()
        v[list(flips)] ^= 1
        D[p + 800 * np.arange(65)] = np.where(v > 0, 60, -60) * (-1 if inverted else 1)
    return D


def _search(hip, D, **kw):
    got = fec.sync_candidates(_dev(hip, D, np.int8), **kw)
    want = fec.sync_candidates_np(D, **{k: v for k, v in kw.items() if k == "min_score"})
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
    return got


@pytest.mark.parametrize("npos", [0, 1, 256, 257])
def test_sync_search_positions(hip, npos):
    frames = [(0, False, ())] if npos else []
    if npos > 1:
        frames.append((npos - 1, True, ()))                       # the last position: at 257 the second workgroup's only thread
    got = _search(hip, _sync_d(npos, 200 + npos, frames))
    assert got.tolist() == [[p, (-1 if inv else 1) * 65 * 60, 65] for p, inv, _ in frames]
    assert len(_search(hip, _sync_d(npos, 210 + npos, frames), min_score=0)) == npos       # every position, in order of p


def test_sync_search_too_short_and_zero(hip):
    for m in (0, 1, SPAN - 1):
        assert _search(hip, np.ones(m, dtype=np.int8)).shape == (0, 3)
    assert _search(hip, np.zeros(SPAN + 300, dtype=np.int8)).shape == (0, 3)             # D all zero: the vector's zeros score


def test_sync_search_score_threshold(hip):
    g = F.rng(220)
    for nflip, kept in ((11, True), (12, False)):
        for inverted in (False, True):
            flips = g.choice(65, nflip, replace=False)
            got = _search(hip, _sync_d(40, 221, [(17, inverted, flips)], noise=0))
            sign = -1 if inverted else 1
            assert got.tolist() == ([[17, sign * (65 - 2 * nflip) * 60, 65 - nflip]] if kept else [])
    D = _sync_d(40, 222, [(17, False, g.choice(65, 12, replace=False))], noise=0)
    assert _search(hip, D, min_score=53).tolist() == [[17, 41 * 60, 53]]                # the keyword moves the threshold


def test_sync_search_cap_and_true_count(hip):
    D = _sync_d(257, 230)
    want = fec.sync_candidates_np(D, min_score=0)
    assert len(want) == 257
    dev = _dev(hip, D, np.int8)
    cand = hip.DevArray.from_host(np.full(3 * 5 + 6, -77, dtype=np.int64))
    cnt = hip.DevArray.from_host(np.full(1, 99, dtype=np.uint64))
    hip.check(hip.lib().dd_fc_sync_search(dev.ptr, dev.n, 0, 5, cand.ptr, cnt.ptr, None))
    c = cand.to_host()
    assert int(cnt.to_host()[0]) == 257 and np.all(c[15:] == -77)
    rows = {tuple(r) for r in want.tolist()}
    assert len({tuple(r) for r in c[:15].reshape(5, 3).tolist()} & rows) == 5            # five of them, whichever came first
    with pytest.raises(RuntimeError):
        fec.sync_candidates(dev, min_score=0, cap=5)
    hip.check(hip.lib().dd_fc_sync_search(dev.ptr, dev.n, 0, 0, None, cnt.ptr, None))    # cap 0: the count alone
    assert int(cnt.to_host()[0]) == 257
    for args in ((dev.ptr, -1, 54, 5, cand.ptr, cnt.ptr), (dev.ptr, dev.n, 54, -1, cand.ptr, cnt.ptr),
                 (dev.ptr, dev.n, 54, 5, cand.ptr, None), (None, dev.n, 54, 5, cand.ptr, cnt.ptr), (dev.ptr, dev.n, 54, 5, None, cnt.ptr)):
        with pytest.raises(ValueError):
            hip.check(hip.lib().dd_fc_sync_search(*args, None))


def test_sync_search_plateau_goes_to_the_lowest_position(hip):
    D = _sync_d(300, 240, [(100, False, ())], noise=0)
    for k in range(65):
        D[101 + 800 * k] = D[102 + 800 * k] = D[100 + 800 * k]
    D[255 + 800 * np.arange(65)] = D[256 + 800 * np.arange(65)] = D[100 + 800 * np.arange(65)]    # across the workgroups
    got = _search(hip, D)
    assert got[:, 0].tolist() == [100, 101, 102, 255, 256] and len(set(got[:, 1].tolist())) == 1
    assert fec.frame_starts(got)[:, 0].tolist() == [100, 255]


# ------------------------------------------------------------------ dd_fc_viterbi
@pytest.fixture(scope="module")
def coded():
    """name -> (D, [(p, inv)], [viterbi_np's (block, corrected) per frame]); computed once"""
    out = {}

    def add(name, D, frames):
        out[name] = (D, frames, [fec.viterbi_np(D, p, inv) for p, inv in frames])
    a, b = F.payload(300), F.payload(301)
    r = F.symbols(302, 5300 + fec.CHANNEL_BITS + 1, [(1, a, False), (5300, b, True)], lead=7)
    add("clean", fec.diff_np(r), [(F.position(7, 1), 0), (F.position(7, 5300), 1)])
    assert np.array_equal(out["clean"][2][0][0], fec.rs_block(a)) and np.array_equal(out["clean"][2][1][0], fec.rs_block(b))
    assert [c for _, c in out["clean"][2]] == [0, 0]
    r = F.symbols(303, fec.CHANNEL_BITS + 2, [(1, a, False)], lead=3, sigma=90.0)
    add("noisy", fec.diff_np(r), [(F.position(3, 1), 0)])
    assert np.array_equal(out["noisy"][2][0][0], fec.rs_block(a)) and out["noisy"][2][0][1] > 0
    add("zero", np.zeros(SPAN + 5, dtype=np.int8), [(0, 0), (5, 1)])
    assert all(np.array_equal(blk, lrpt.pn_sequence(320)) and c == 0 for blk, c in out["zero"][2])      # the tie rule: all zeros
    D = np.where(F.rng(304).integers(0, 2, SPAN + 3) > 0, 127, -128).astype(np.int8)
    add("extremes", D, [(0, 0), (3, 1), (1, 1)])                                                     # -(-128) = 128 under inv
    D = F.rng(305).integers(-128, 128, SPAN).astype(np.int8)
    add("random", D, [(0, 0), (0, 1)])
    return out


@pytest.mark.parametrize("name", ["clean", "noisy", "zero", "extremes", "random"])
def test_viterbi(hip, coded, name):
    D, frames, want = coded[name]
    dev = _dev(hip, D, np.int8)
    blocks, corrected = fec.viterbi(dev, frames)
    assert blocks.dtype == np.uint8 and blocks.shape == (len(frames), 320) and corrected.dtype == np.int32
    assert corrected.tolist() == [c for _, c in want]
    assert np.array_equal(blocks, np.stack([b for b, _ in want]))
    one, c1 = fec.viterbi(dev, frames[-1:])                                                          # alone as in the batch
    assert np.array_equal(one[0], want[-1][0]) and c1.tolist() == [want[-1][1]]


def test_viterbi_no_frames_tails_and_bad_arguments(hip, coded):
    D, frames, want = coded["clean"]
    dev = _dev(hip, D, np.int8)
    blocks, corrected = fec.viterbi(dev, np.zeros((0, 2), dtype=np.int64))
    assert blocks.shape == (0, 320) and corrected.shape == (0,)
    out = hip.DevArray.from_host(np.full(2 * 320 + 16, 0xA5, dtype=np.uint8))
    cor = hip.DevArray.from_host(np.full(2 + 4, -77, dtype=np.int32))
    s = np.ascontiguousarray(frames, dtype=np.int64)
    hip.check(hip.lib().dd_fc_viterbi(dev.ptr, dev.n, s.ctypes.data, 2, out.ptr, cor.ptr, None))
    o, c = out.to_host(), cor.to_host()
    assert np.array_equal(o[:640].reshape(2, 320), np.stack([b for b, _ in want])) and np.all(o[640:] == 0xA5)
    assert c[:2].tolist() == [0, 0] and np.all(c[2:] == -77)
    last = dev.n - SPAN
    fec.viterbi(dev, [(last, 0)])                                                                    # the last frame that fits
    for bad in ([(-1, 0)], [(last + 1, 0)], [(0, 2)], [(0, -1)], [(0, 0), (dev.n, 0)]):
        with pytest.raises(ValueError):
            fec.viterbi(dev, bad)
    short = _dev(hip, np.zeros(SPAN - 1, dtype=np.int8), np.int8)
    with pytest.raises(ValueError):
        fec.viterbi(short, [(0, 0)])
    for args in ((None, dev.n, s.ctypes.data, 1, out.ptr, cor.ptr), (dev.ptr, dev.n, None, 1, out.ptr, cor.ptr),
                 (dev.ptr, dev.n, s.ctypes.data, 1, None, cor.ptr), (dev.ptr, dev.n, s.ctypes.data, 1, out.ptr, None),
                 (dev.ptr, dev.n, s.ctypes.data, -1, out.ptr, cor.ptr)):
        with pytest.raises(ValueError):
            hip.check(hip.lib().dd_fc_viterbi(*args, None))


# ------------------------------------------------------------------ dd_fc_rs
def _hit(block, c, positions, g, value=None):
    """damage bytes `positions` (0..159) of codeword c of a 320-byte block"""
    idx = c + 2 * np.asarray(positions)
    block[idx] ^= g.integers(1, 256, len(idx), dtype=np.uint8) if value is None else np.uint8(value)


def _rs_both(blocks):
    frames, errors = fec.reed_solomon(blocks)
    want_frames, want_errors = fec.reed_solomon_np(blocks)
    assert frames.dtype == np.uint8 and frames.shape == (len(blocks), 256) and errors.shape == (len(blocks), 2)
    assert errors.dtype == np.int32 and np.array_equal(errors, want_errors), (errors.tolist(), want_errors.tolist())
    assert np.array_equal(frames, want_frames)
    return frames, errors


def test_rs_error_counts(hip):
    g = F.rng(400)
    data = [F.payload(401 + i) for i in range(4)]
    got = np.stack([fec.rs_block(d) for d in data])
    counts = [[0, 1], [16, 17], [17, 16], [1, 0]]                   # each codeword by each way through the wave, beside each other
    for f, pair in enumerate(counts):
        for c, e in enumerate(pair):
            _hit(got[f], c, g.choice(160, e, replace=False), g)
    frames, errors = _rs_both(got)
    assert errors.tolist() == [[e if e <= 16 else -1 for e in pair] for pair in counts]
    for f, pair in enumerate(counts):
        for c, e in enumerate(pair):
            assert np.array_equal(frames[f, c::2], data[f][c::2] if e <= 16 else got[f, c::2][:128])


def test_rs_errors_at_the_ends_and_in_the_parity(hip):
    g = F.rng(410)
    data = [F.payload(411 + i) for i in range(2)]
    got = np.stack([fec.rs_block(d) for d in data])
    _hit(got[0], 0, [0], g)
    _hit(got[0], 1, [159], g)
    _hit(got[1], 0, 128 + g.choice(32, 16, replace=False), g)
    _hit(got[1], 1, [0, 127, 128, 159], g, value=0x01)
    frames, errors = _rs_both(got)
    assert errors.tolist() == [[1, 1], [16, 4]] and np.array_equal(frames, np.stack(data))


def test_rs_shortened_positions_reject(hip):
    """a word one byte (at a padded position j < 95) from a full-length codeword: the (255,223) decoder would put that byte back"""
    data = F.payload(420)
    got = np.stack([fec.rs_block(data)] * 4)
    for f, (c, j) in enumerate(((0, 0), (1, 94), (0, 40), (1, 63))):
        unit = np.zeros(223, dtype=np.uint8)
        unit[j] = 1 + 50 * f
        full = lrpt.rs_encode(unit)
        assert full[:95].any() and not full[95:223].any()
        got[f, c::2] ^= full[95:]
        word = np.concatenate((np.zeros(95, dtype=np.uint8), got[f, c::2]))
        fixed, err = lrpt.rs_decode_np(word)
        assert err == 1 and fixed[j] == unit[j]                      # the full-length code's answer
    frames, errors = _rs_both(got)
    assert errors.tolist() == [[-1, 0], [0, -1], [-1, 0], [0, -1]]
    assert np.array_equal(frames, got.reshape(4, 160, 2)[:, :128].reshape(4, 256))       # the parity differs, the data bytes do not


def test_rs_random_block_no_frames_tails_and_bad_arguments(hip):
    blk = F.rng(430).integers(0, 256, size=(1, 320), dtype=np.uint8)
    frames, errors = _rs_both(blk)
    assert errors.tolist() == [[-1, -1]] and np.array_equal(frames[0], blk.reshape(160, 2)[:128].ravel())
    frames, errors = _rs_both(np.zeros((0, 320), dtype=np.uint8))
    assert frames.shape == (0, 256) and errors.shape == (0, 2)
    g = F.rng(431)
    got = np.stack([fec.rs_block(F.payload(432 + i)) for i in range(3)])
    for f in range(3):
        for c in range(2):
            _hit(got[f], c, g.choice(160, 9, replace=False), g)
    want_frames, want_errors = fec.reed_solomon_np(got)
    dev = hip.DevArray.from_host(got.ravel())
    frames, errors = fec.reed_solomon(dev)                                               # a device array in
    assert np.array_equal(frames, want_frames) and np.array_equal(errors, want_errors) and np.all(errors == 9)
    out = hip.DevArray.from_host(np.full(3 * 256 + 16, 0xA5, dtype=np.uint8))
    err = hip.DevArray.from_host(np.full(3 * 2 + 4, -77, dtype=np.int32))
    hip.check(hip.lib().dd_fc_rs(dev.ptr, 3, out.ptr, err.ptr, None))
    o, e = out.to_host(), err.to_host()
    assert np.array_equal(o[:768].reshape(3, 256), want_frames) and np.all(o[768:] == 0xA5)
    assert np.array_equal(e[:6].reshape(3, 2), want_errors) and np.all(e[6:] == -77)
    hip.check(hip.lib().dd_fc_rs(None, 0, None, None, None))                             # no frames: nothing is touched
    for args in ((dev.ptr, -1, out.ptr, err.ptr), (None, 1, out.ptr, err.ptr), (dev.ptr, 1, None, err.ptr), (dev.ptr, 1, out.ptr, None)):
        with pytest.raises(ValueError):
            hip.check(hip.lib().dd_fc_rs(*args, None))
    for bad in (np.zeros((2, 319), dtype=np.uint8), np.zeros(320, dtype=np.uint8), hip.DevArray(321, np.uint8),
                hip.DevArray(320, np.int8)):
        with pytest.raises(ValueError):
            fec.reed_solomon(bad)


# ------------------------------------------------------------------ decode_funcube.getFrames / frameInfo
def test_frames_end_to_end(hip):
    from directdemod_amd import decode_funcube, source
    data = F.payload(500)
    raw, start = F.recording(501, data)
    obj = decode_funcube.decode_funcube(source.IQarray(raw, F.FS), 0, None, _funcube.CENTER, _funcube.CHANNEL)
    syncs, useful, before = obj.getSyncs, obj.useful, dict(obj.timings)
    frames, info = obj.getFrames, obj.frameInfo
    print("funcube frames: %s" % {k: info[k].tolist() for k in info.dtype.names})
    assert frames.dtype == np.uint8 and frames.shape == (1, 256) and info.dtype == fec.INFO and info.shape == (1,)
    assert np.array_equal(frames[0], data)
    assert info["ok"].tolist() == [True] and info["rs_errors"].tolist() == [[0, 0]]
    assert info["sync_score"].tolist() == [65] and info["corrected"].tolist() == [0] and info["inverted"].tolist() == [0]
    assert (int(info["sat_id"][0]), int(info["frame_type"][0])) == (int(data[0]) >> 6, int(data[0]) & 0x3F)
    assert abs(int(info["sample"][0]) - start) <= F.FS // 1200 + 1                       # within one bit of where it was put
    # the same stages by hand on the cached walk
    w = obj.walker()
    D = fec.soft_bits(w.view("sym"))
    Dh = D.to_host()
    assert np.array_equal(Dh, fec.soft_bits_np(w.view("sym").to_host()))
    cands = fec.sync_candidates(D)
    assert np.array_equal(cands, fec.sync_candidates_np(Dh))
    starts = fec.frame_starts(cands)
    assert info["symbol"].tolist() == (starts[:, 0] + 10).tolist() and info["sync_corr"].tolist() == starts[:, 1].tolist()
    assert info["sample"].tolist() == [int(w.view("aidx").to_host()[int(k)]) for k in info["symbol"]]
    blocks, corrected = fec.viterbi(D, [(int(starts[0, 0]), 0)])
    assert np.array_equal(blocks[0], fec.viterbi_np(Dh, int(starts[0, 0]), 0)[0])
    assert np.array_equal(fec.reed_solomon(blocks)[0], frames) and corrected.tolist() == [0]
    # cached, and what was there before stays
    assert obj.getFrames is frames and obj.frameInfo is info
    assert obj.getSyncs == syncs and obj.useful == useful
    for k, v in before.items():
        assert obj.timings[k] == v
    for k in ("fc_soft", "fc_sync", "fc_viterbi", "fc_rs"):
        assert k not in before and obj.timings[k] >= 0.0


def test_noise_only_recording_gives_empty_arrays(hip):
    from directdemod_amd import decode_funcube, source
    raw, off, corr = _funcube.case("d")
    obj = decode_funcube.decode_funcube(source.IQarray(raw, _funcube.FS), off, None, _funcube.CENTER, _funcube.CHANNEL, corr)
    frames, info = obj.getFrames, obj.frameInfo                   # before getSyncs: the walk is made for them
    assert frames.dtype == np.uint8 and frames.shape == (0, 256) and info.dtype == fec.INFO and info.shape == (0,)
    assert obj.walker().nsym < SPAN
    fresh = decode_funcube.decode_funcube(source.IQarray(raw, _funcube.FS), off, None, _funcube.CENTER, _funcube.CHANNEL, corr)
    assert obj.getSyncs == fresh.getSyncs and obj.useful == fresh.useful
