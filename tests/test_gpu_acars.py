"""The ACARS kernels on the device (dd_acars.h through dd_acars_candidates, dd_acars_blocks and the diagnostic dd_debug_acars_masks,
the wrappers of directdemod_amd/acars.py and decode_acars) against the NumPy restatement in acars.py.

Everything behind the quantiser is integer, so every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import _acars as T
from directdemod_amd import acars, decode_acars, source

pytestmark = pytest.mark.gpu

SENT = np.int64(-0x5A5A5A5A5A5A5A5B)
SPARE = 16
SPS = [8.0, 10.5, 20.0, 20.317, 64.0]
KEYS = ("t", "bytes", "score") + acars.META


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def w_of(sps):
    return acars.params(sps * 2400.0)[1]


def dev_candidates(hip, audio, sps, w, slack, cap):
    """dd_acars_candidates with `cap` places and SPARE sentinels behind them -> (rc, count, the places, the sentinels still whole)"""
    x = hip.DevArray.from_host(np.ascontiguousarray(audio if len(audio) else np.zeros(1), dtype=np.float64))
    lst = hip.DevArray.from_host(np.full(cap + SPARE, SENT))
    count = C.c_int64(-1)
    rc = hip.lib().dd_acars_candidates(x.ptr, len(audio), float(sps), int(w), int(slack), lst.ptr, cap, C.byref(count), None)
    hip.sync()
    got = lst.to_host()
    return rc, count.value, got[:cap], bool(np.all(got[cap:] == SENT))


def check_candidates(hip, audio, sps, w=None, slack=2):
    """the device's list and, through the diagnostic entry, its mask bytes against the restatement's"""
    w = w_of(sps) if w is None else w
    masks = acars.masks_host(audio, sps, w, slack)
    want = np.flatnonzero(masks & 1).astype(np.int64)
    rc, count, got, whole = dev_candidates(hip, audio, sps, w, slack, len(want) + 3)
    assert rc == 0 and count == len(want) and whole
    assert np.array_equal(got[:count], want) and np.all(got[count:] == SENT)
    if len(audio):
        x = hip.DevArray.from_host(np.ascontiguousarray(audio, dtype=np.float64))
        mask = hip.DevArray.from_host(np.full(len(audio) + SPARE, 0xA5, np.uint8))
        assert hip.lib().dd_debug_acars_masks(x.ptr, len(audio), float(sps), int(w), int(slack), mask.ptr, None) == 0
        hip.sync()
        dev = mask.to_host()
        assert np.array_equal(dev[:len(masks)], masks) and not dev[len(masks):len(audio)].any() and np.all(dev[len(audio):] == 0xA5)
    return want


def dev_blocks(hip, audio, sps, w, fix, ts):
    """dd_acars_blocks with sentinels behind every output -> the dict of acars.blocks_host"""
    m = len(ts)
    x = hip.DevArray.from_host(np.ascontiguousarray(audio, dtype=np.float64))
    lst = hip.DevArray.from_host(np.ascontiguousarray(ts, dtype=np.int64))
    data = hip.DevArray.from_host(np.full(acars.CHARS * m + SPARE, 0xA5, np.uint8))
    meta = hip.DevArray.from_host(np.full(8 * m + SPARE, -0x5A5A5A5B, np.int32))
    score = hip.DevArray.from_host(np.full(m + SPARE, SENT))
    rc = hip.lib().dd_acars_blocks(x.ptr, len(audio), float(sps), int(w), int(fix), lst.ptr, m, data.ptr, meta.ptr, score.ptr, None)
    hip.sync()
    assert rc == 0
    by, mt, sc = data.to_host(), meta.to_host(), score.to_host()
    k = acars.CHARS * m
    assert np.all(by[k:] == 0xA5) and np.all(mt[8 * m:] == -0x5A5A5A5B) and np.all(sc[m:] == SENT)
    mt = mt[:8 * m].reshape(m, 8)
    out = {"t": np.asarray(ts, dtype=np.int64), "bytes": by[:k].reshape(m, acars.CHARS), "score": sc[:m]}
    out.update({key: mt[:, i] for i, key in enumerate(acars.META)})
    return out


def check_blocks(hip, audio, sps, ts, w=None, fix=2):
    w = w_of(sps) if w is None else w
    got = dev_blocks(hip, audio, sps, w, fix, ts)
    want = acars.blocks_host(audio, sps, w, fix, ts)
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    return got


def one_block(sps, block=T.SHORT, start=50.3, sigma=3.0, seed=1, prekey=acars.PREKEY, **kw):
    """(the envelope of one block over noise at `sps` samples per bit, the sample its template starts at)"""
    rate = sps * 2400.0
    x = acars.encode_audio([block], rate, [start], sigma=sigma, seed=seed, prekey=prekey, **kw)
    return x, int(acars.block_start(rate, start, prekey))


# ---------------------------------------------------------------------------------------------------------------- candidates
@pytest.mark.parametrize("sps", SPS)
def test_masks_and_lists(hip, sps):
    x, t = one_block(sps, seed=int(sps))
    for w in sorted({1, w_of(sps), acars.W_MAX}):
        for slack in (0, 2, acars.SLACK_MAX):
            want = check_candidates(hip, x, sps, w, slack)
            if w == w_of(sps):
                assert len(want) >= 2 and np.all(np.abs(want - t) < sps)                             # the block, and nothing else
    noise = np.random.default_rng(int(sps * 10)).normal(40.0, 12.0, 1 << 15)                         # 128 tiles of noise
    assert len(check_candidates(hip, noise, sps, slack=acars.SLACK_MAX)) > 0


@pytest.mark.parametrize("sps", [8.0, 20.317, 64.0])
def test_lengths(hip, sps):
    w = w_of(sps)
    full = acars.reach(sps, w)
    x, t = one_block(sps, start=0.0, prekey=0, sigma=0.0)            # the template starts at sample 8 sps, behind the +
    x = x[t:]
    assert acars.n_starts(full - 1, sps, w) == 0 and acars.n_starts(full, sps, w) == 1
    for n in (0, 1, full - 1):
        rc, count, got, whole = dev_candidates(hip, x[:n], sps, w, 0, 4)
        assert (rc, count, whole) == (0, 0, True) and np.all(got == SENT)
    assert check_candidates(hip, x[:full], sps, slack=0).tolist() == [0]                             # the one start there is
    for starts in (255, 256, 257, 513):
        y = np.concatenate((np.full(starts - 1, x[0]), x[:full]))    # the template on the last start of the last tile
        want = check_candidates(hip, y, sps, slack=0)
        assert acars.n_starts(len(y), sps, w) == starts and want[-1] == starts - 1


@pytest.mark.parametrize("edge", [256, 1024])
def test_a_block_across_a_tile_edge(hip, edge):
    for sps in (8.0, 20.0):
        start = edge - (8 * acars.PREKEY + 8) * sps + 0.5            # the template's true start half a sample behind the edge
        x, t = one_block(sps, start=start, sigma=0.0)
        assert t == edge
        want = check_candidates(hip, x, sps, slack=0)
        assert np.any(want < edge) and np.any(want >= edge)
        det = check_blocks(hip, x, sps, want)
        assert edge in want and det["status"][want.tolist().index(edge)] == acars.OK


def test_capacities(hip):
    x, _ = one_block(20.0)
    want = acars.candidates_host(x, 20.0, 10)
    m = len(want)
    assert m >= 3
    for cap in (0, 1, m - 1, m, m + 1, m + 5):
        rc, count, got, whole = dev_candidates(hip, x, 20.0, 10, 2, cap)
        assert count == m and whole
        assert rc == (0 if cap >= m else hip.DD_ERR_INVALID)
        kept = min(cap, m)
        assert np.array_equal(got[:kept], want[:kept]) and np.all(got[kept:] == SENT)
    lst, count = acars.candidates(hip.DevArray.from_host(x), 20.0, 10, cap=1)                        # the wrapper asks again at the true count
    assert count == m and np.array_equal(lst.view(0, m).to_host(), want)


# ---------------------------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize("sps", SPS)
def test_starts_inside_and_outside(hip, sps):
    x, t = one_block(sps)
    n, w = len(x), w_of(sps)
    last = acars.n_starts(n, sps, w) - 1
    ts = np.array([0, last, n - 1, t, t + 1, t - 1, -1, n, 1 << 40, -(1 << 62)])
    for wv in sorted({1, w, acars.W_MAX}):
        det = check_blocks(hip, x, sps, ts, wv)
        assert det["status"][6:].tolist() == [acars.OUTSIDE] * 4 and not det["bytes"][6:].any() and np.all(det["end"][6:] == -1)
        assert np.all(det["status"][:6] != acars.OUTSIDE)
    det = check_blocks(hip, x, sps, ts)
    assert det["status"][3] == acars.OK and det["end"][3] == 12 and bytes(det["bytes"][3][:16]) == T.SHORT


@pytest.mark.parametrize("polarity", [0, 1])
@pytest.mark.parametrize("more", [False, True])
def test_ends(hip, polarity, more):
    for block, e, status in ((T.text_block(None, more), 12, acars.OK), (T.text_block(0, more), 13, acars.OK),
                             (T.block_ending_at(236, more), 236, acars.OK), (T.block_ending_at(237, more), 237, acars.OK),
                             (T.block_ending_at(238, more), -1, acars.NO_END)):
        x, t = one_block(10.5, block, polarity=polarity, sigma=1.0)
        det = check_blocks(hip, x, 10.5, [t, t + 1])
        assert (det["status"][0], det["end"][0], det["polarity"][0], det["mis"][0]) == (status, e, polarity, 0)
        assert det["del"][0] == (0 <= e <= 236) and bytes(det["bytes"][0][:len(block)]) == block
        if e >= 0:
            assert block[e] == (acars.ETB if more else acars.ETX)


def test_nan_and_samples_out_of_range(hip):
    x, t = one_block(20.0, T.text_block(12))
    rng = np.random.default_rng(8)
    bad = x.copy()
    at = rng.integers(0, len(x), 400)
    bad[at] = np.resize([np.nan, np.inf, -np.inf, 512.0 + T.UNIT, -512.0 - T.UNIT, 512.0, -512.0, 1e300], len(at))
    bad[t + 20 * np.arange(1, 33)] = np.nan                          # on every boundary of the template
    want = check_candidates(hip, bad, 20.0, slack=acars.SLACK_MAX)
    check_blocks(hip, bad, 20.0, np.concatenate((want, [t, t - 3, t + 4])))
    for fill in (np.nan, np.inf, 1e9):                               # nothing but samples that quantise to 0
        flat = np.full(3000, fill)
        assert len(check_candidates(hip, flat, 20.0, slack=acars.SLACK_MAX)) == 0
        det = check_blocks(hip, flat, 20.0, [0, 17])
        assert not det["bytes"].any() and np.all(det["score"] == 0)


def test_ties_read_zero(hip):
    """v = 0 is a 0: constant audio gives 32 zeros, ten places from the template (its ten ones), polarity 0 and zero bytes; and a
    lone tie on a boundary where the template holds a 1 costs that place"""
    for fill in (0.0, 37.0, 512.0, -512.0):
        flat = np.full(20000, fill)
        assert len(check_candidates(hip, flat, 8.0, slack=acars.SLACK_MAX)) == 0
        det = check_blocks(hip, flat, 8.0, [0, 100, 4000, 19999])    # (the third crosses the audio's end: a step, no tie)
        assert np.all(det["mis"] == 10) and np.all(det["polarity"] == 0) and not det["bytes"][:2].any()
        assert np.all(det["status"][:2] == acars.NO_END)
    q = T.integer_audio([T.SHORT], 8, [40.0])
    t = int(acars.block_start(19200.0, 40.0))
    ones = np.flatnonzero(acars.TEMPLATE_BITS)
    assert check_blocks(hip, T.as_audio(q), 8.0, [t], 1)["mis"][0] == 0
    for k in ones[[0, 3, 9]]:
        tie = q.copy()
        B = t + 8 * (k + 1)
        tie[B] = tie[B - 1]                                          # w = 1: v = q[B] - q[B - 1] = 0
        det = check_blocks(hip, T.as_audio(tie), 8.0, [t], 1)
        assert det["mis"][0] == 1
        assert t in check_candidates(hip, T.as_audio(tie), 8.0, 1, slack=1) and t not in check_candidates(hip, T.as_audio(tie), 8.0, 1, slack=0)
        tie[B] += 1
        assert check_blocks(hip, T.as_audio(tie), 8.0, [t], 1)["mis"][0] == 0


ROUTES = {"clean": ({}, 0, 0, acars.OK, 0), "one_character": ({5: 0x10}, 1, 1, acars.OK, 1), "bcs": ({44: 0x04}, 0, 1, acars.OK, 1),
          "two_characters": ({15: 0x01, 40: 0x80}, 2, 2, acars.OK, 2), "three_characters": ({1: 1, 2: 2, 3: 4}, 3, 0, acars.BAD_BCS, 3),
          "two_in_one_character": ({20: 0x03}, 0, 0, acars.BAD_BCS, 3), "etx": ({43: 0x01}, 0, 0, acars.NO_END, 3)}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_each_repair_route(hip, route):
    """every route hit, and refused where `fix` is below its need; need 3 stands for a pattern that is never repaired"""
    flips, flags, repaired, status, need = ROUTES[route]
    block = T.text_block(30)                                         # ETX is byte 43, the block check bytes 44 and 45
    x, t = one_block(20.0, block, flips=[flips], sigma=0.5)
    for fix in (0, 1, 2):
        det = check_blocks(hip, x, 20.0, [t, t + 2, t - 2], fix=fix)
        ok = fix >= need
        if route == "etx":                                           # no end, or a later one among what follows the block
            assert det["status"][0] != acars.OK and det["end"][0] != 43
            continue
        assert det["status"][0] == (status if ok or need == 3 else acars.BAD_BCS)
        assert det["repaired"][0] == (repaired if ok else 0) and det["flags"][0] == flags
        assert (bytes(det["bytes"][0][:len(block)]) == block) == (ok and status == acars.OK)


def test_two_hits_in_the_pair_search(hip):
    f1, i, f2, j, i2, j2 = T.twin_pairs()
    block = T.block_ending_at(236)
    for flips, status in (({f1: 1 << i, f2: 1 << j}, acars.BAD_BCS), ({f1: 1 << i2, f2: 1 << j2}, acars.BAD_BCS),
                          ({f1: 1 << i}, acars.OK), ({f1: (1 << i) | (1 << i2)}, acars.BAD_BCS)):
        x, t = one_block(8.0, block, flips=[flips], sigma=0.5)
        det = check_blocks(hip, x, 8.0, [t])
        assert det["status"][0] == status and det["end"][0] == 236 and det["flags"][0] == sum(bin(v).count("1") & 1 for v in flips.values())


@pytest.mark.parametrize("m", [1, 65, 300])
def test_list_lengths(hip, m):
    x, t = one_block(10.5, T.text_block(3), seed=m)
    ts = np.random.default_rng(m).integers(-5, len(x) + 5, m)
    ts[0] = t
    det = check_blocks(hip, x, 10.5, ts)
    assert det["status"][0] == acars.OK


def test_prefix_sums_that_wrap(hip):
    """64 samples per bit and w = 32: a tile's stage holds 2370 words, and at the quantiser's ceiling of 2^21 their sum passes
    2^32; the differences of the wrapped sums are still exact"""
    sps = 64.0
    x, t = one_block(sps, amplitudes=2.0, sigma=0.0)
    high = x + 508.0                                                 # the envelope swings between 508.4 and 511.6 inside the block
    assert high.max() < 512.0 and acars.quantise(high)[:2400].sum() > 1 << 32
    want = check_candidates(hip, high, sps, slack=0)
    assert len(want) >= 16 and np.all(np.abs(want - t) < sps)
    assert check_blocks(hip, high, sps, want[:4])["status"].tolist() == [acars.OK] * 4
    top = np.full(6000, 512.0)                                       # the ceiling itself, constant: all ties
    assert len(check_candidates(hip, top, sps, slack=acars.SLACK_MAX)) == 0


def test_invalid_arguments(hip):
    L = hip.lib()
    x = hip.DevArray.from_host(np.zeros(4096))
    lst = hip.DevArray.from_host(np.full(8, SENT))
    data, meta, score = hip.DevArray(acars.CHARS * 8, np.uint8), hip.DevArray(64, np.int32), hip.DevArray(8, np.int64)
    mask = hip.DevArray(4096, np.uint8)
    count = C.c_int64(0)
    good = {"n": 4096, "sps": 20.0, "w": 10, "slack": 2, "fix": 2, "cap": 8, "m": 8}
    bad = [("n", -1), ("n", 0x7FFFFFF1), ("sps", 7.999), ("sps", 64.001), ("sps", float("nan")), ("w", 0), ("w", 33), ("slack", -1),
           ("slack", acars.SLACK_MAX + 1), ("fix", -1), ("fix", 3), ("cap", -1), ("m", -1), ("m", 1 << 31)]
    for key, value in bad:
        a = dict(good, **{key: value})
        if key not in ("fix", "m"):
            if key != "cap":
                assert L.dd_debug_acars_masks(x.ptr, a["n"], a["sps"], a["w"], a["slack"], mask.ptr, None) == hip.DD_ERR_INVALID, (key, value)
            rc = L.dd_acars_candidates(x.ptr, a["n"], a["sps"], a["w"], a["slack"], lst.ptr, a["cap"], C.byref(count), None)
            assert rc == hip.DD_ERR_INVALID, (key, value)
        if key not in ("slack", "cap"):
            rc = L.dd_acars_blocks(x.ptr, a["n"], a["sps"], a["w"], a["fix"], lst.ptr, a["m"], data.ptr, meta.ptr, score.ptr, None)
            assert rc == hip.DD_ERR_INVALID, (key, value)
    assert L.dd_acars_candidates(None, 4096, 20.0, 10, 2, lst.ptr, 8, C.byref(count), None) == hip.DD_ERR_INVALID
    assert L.dd_acars_candidates(x.ptr, 4096, 20.0, 10, 2, None, 8, C.byref(count), None) == hip.DD_ERR_INVALID
    assert L.dd_acars_candidates(x.ptr, 4096, 20.0, 10, 2, lst.ptr, 8, None, None) == hip.DD_ERR_INVALID
    assert L.dd_acars_blocks(x.ptr, 4096, 20.0, 10, 2, lst.ptr, 8, None, meta.ptr, score.ptr, None) == hip.DD_ERR_INVALID
    assert L.dd_debug_acars_masks(x.ptr, 4096, 20.0, 10, 2, None, None) == hip.DD_ERR_INVALID
    hip.sync()
    assert np.all(lst.to_host() == SENT)                             # nothing was touched
    with pytest.raises(TypeError):
        acars.candidates(np.zeros(100), 20.0, 10)


# ---------------------------------------------------------------------------------------------------------------- end to end
def same_blocks(got, want):
    assert len(got) == len(want)
    for g, v in zip(got, want):
        assert g == v


def test_end_to_end(hip):
    """decode_acars over the host test's recording.  Its front end is float32 on the device, which float64 NumPy does not repeat
    bit for bit; so the device decoder is held exactly (blocks, frameInfo, candidates) to the restatement run over the device's own
    audio, and to decode_host of the recording and to the blocks encoded in what does not hang on a rounding."""
    raw = np.array(T.recording())
    dec = decode_acars.decode_acars(source.IQarray(raw, T.FS), T.OFFSETS)
    assert dec.audioRate == 48000.0
    audios = [a.to_host() for a in dec.audio()]
    found, info, cands = acars.decode(audios, dec.audioRate, ["A", "B"], ops=acars.HostOps())
    same_blocks(dec.getBlocks, found)
    assert dec.frameInfo == info and dec.getText == [acars.line(b) for b in found] and dec.useful == 1
    assert dec.getMessages == acars.messages(found) and len(dec.getMessages) == 4
    got = dec.candidateInfo
    for ch in "AB":
        for key in KEYS:
            assert np.array_equal(got[ch][key], cands[ch][key]), (ch, key)
    assert [(b["channel"], b["bytes"]) for b in found] == T.expected()
    assert set(dec.timings) == {"front_end", "candidates", "blocks", "host"}
    hfound, hinfo, hmsgs = decode_acars.decode_host(raw, T.FS, T.OFFSETS)
    assert len(hfound) == 6 and [m["text"] for m in hmsgs] == [m["text"] for m in dec.getMessages]
    for g, v in zip(dec.getBlocks, hfound):
        for key in ("channel", "mode", "address", "ack", "label", "block_id", "downlink", "msgno", "flight", "text", "more", "corrected",
                    "parity_errors", "polarity", "closed", "bytes"):
            assert g[key] == v[key], key
        assert abs(g["start"] - v["start"]) <= 8 * 20                # the merge picks one start of eight bit times of them
    same = decode_acars.decode_acars(source.IQarray(raw, T.FS), T.OFFSETS, use_device_raw=False)
    same_blocks(same.getBlocks, found)


def test_from_audio(hip):
    rate = 48000.0
    blks = [T.text_block(30), T.text_block(None), T.text_block(7, True)]
    flips = [{5: 0x10}, None, {15: 0x01, 18: 0x80}]
    x = acars.encode_audio(blks, rate, [300.25, 20000.5, 30000.75], sigma=1.0, seed=4, polarity=(1, 0, 0), flips=flips)
    found, info, msgs = decode_acars.decode_audio_host(x, rate, "C")
    assert [b["bytes"] for b in found] == [b[:-1] for b in blks] and [b["corrected"] for b in found] == [1, 0, 2]
    assert [b["polarity"] for b in found] == [1, 0, 0] and len(msgs) == 3
    for audio in (x, hip.DevArray.from_host(x)):
        dec = decode_acars.decode_acars.fromAudio(audio, rate, "C")
        same_blocks(dec.getBlocks, found)
        assert dec.frameInfo == info and dec.getMessages == msgs
    ac = decode_acars.decode_acars.fromAudio(x - x.mean(), rate, "C")                                 # a receiver's audio: no carrier level
    assert [b["bytes"] for b in ac.getBlocks] == [b["bytes"] for b in found]
    empty = decode_acars.decode_acars.fromAudio(np.zeros(10), rate)
    assert empty.getBlocks == [] and empty.useful == 0 and empty.frameInfo["blocks"] == 0 and empty.getMessages == []
