"""The POCSAG kernels on the device (dd_pocsag.h through dd_pocsag_candidates, dd_pocsag_batches and the diagnostic
dd_debug_pocsag_masks, the wrappers of directdemod_amd/pocsag.py and decode_pocsag) against the NumPy restatement in pocsag.py.

Everything behind the quantiser is integer, so every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import _pocsag as T
from directdemod_amd import decode_pocsag, pocsag, source

pytestmark = pytest.mark.gpu

SENT = np.int64(-0x5A5A5A5A5A5A5A5B)
SPARE = 16
SPS = [4.0, 7.5, 20.0, 40.0, 93.75, 128.0]


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def w_of(sps):
    return pocsag.params(sps * 1200.0, 1200)[1]


def dev_candidates(hip, audio, sps, w, slack, cap):
    """dd_pocsag_candidates with `cap` places and SPARE sentinels behind them -> (rc, count, the places, the sentinels still whole)"""
    x = hip.DevArray.from_host(np.ascontiguousarray(audio if len(audio) else np.zeros(1), dtype=np.float64))
    lst = hip.DevArray.from_host(np.full(cap + SPARE, SENT))
    count = C.c_int64(-1)
    rc = hip.lib().dd_pocsag_candidates(x.ptr, len(audio), float(sps), int(w), int(slack), lst.ptr, cap, C.byref(count), None)
    hip.sync()
    got = lst.to_host()
    return rc, count.value, got[:cap], bool(np.all(got[cap:] == SENT))


def check_candidates(hip, audio, sps, w=None, slack=2):
    """the device's list and, through the diagnostic entry, its mask bytes against the restatement's"""
    w = w_of(sps) if w is None else w
    masks = pocsag.masks_host(audio, sps, w, slack)
    want = np.flatnonzero(masks & 1).astype(np.int64)
    rc, count, got, whole = dev_candidates(hip, audio, sps, w, slack, len(want) + 3)
    assert rc == 0 and count == len(want) and whole
    assert np.array_equal(got[:count], want) and np.all(got[count:] == SENT)
    if len(audio):
        dev = pocsag.masks_device(hip.DevArray.from_host(np.ascontiguousarray(audio, dtype=np.float64)), sps, w, slack)
        assert np.array_equal(dev[:len(masks)], masks) and not dev[len(masks):].any()
    return want


def dev_batches(hip, audio, sps, w, fix, ts):
    """dd_pocsag_batches with sentinels behind every output -> the dict of pocsag.batches_host"""
    m = len(ts)
    x = hip.DevArray.from_host(np.ascontiguousarray(audio, dtype=np.float64))
    lst = hip.DevArray.from_host(np.ascontiguousarray(ts, dtype=np.int64))
    words = hip.DevArray.from_host(np.full(pocsag.WORDS * m + SPARE, 0xA5A5A5A5, np.uint32))
    errs = hip.DevArray.from_host(np.full(pocsag.WORDS * m + SPARE, 0xA5, np.uint8))
    meta = hip.DevArray.from_host(np.full(4 * m + SPARE, -0x5A5A5A5B, np.int32))
    score = hip.DevArray.from_host(np.full(m + SPARE, SENT))
    rc = hip.lib().dd_pocsag_batches(x.ptr, len(audio), float(sps), int(w), int(fix), lst.ptr, m, words.ptr, errs.ptr, meta.ptr, score.ptr,
                                     None)
    hip.sync()
    assert rc == 0
    wd, er, mt, sc = words.to_host(), errs.to_host(), meta.to_host(), score.to_host()
    k = pocsag.WORDS * m
    assert np.all(wd[k:] == 0xA5A5A5A5) and np.all(er[k:] == 0xA5) and np.all(mt[4 * m:] == -0x5A5A5A5B) and np.all(sc[m:] == SENT)
    mt = mt[:4 * m].reshape(m, 4)
    return {"t": np.asarray(ts, dtype=np.int64), "words": wd[:k].reshape(m, pocsag.WORDS), "errs": er[:k].reshape(m, pocsag.WORDS),
            "status": mt[:, 0], "polarity": mt[:, 1], "good": mt[:, 2], "mis": mt[:, 3], "score": sc[:m]}


KEYS = ("t", "words", "errs", "status", "polarity", "good", "mis", "score")


def check_batches(hip, audio, sps, ts, w=None, fix=2):
    w = w_of(sps) if w is None else w
    got = dev_batches(hip, audio, sps, w, fix, ts)
    want = pocsag.batches_host(audio, sps, w, fix, ts)
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    return got


# ---------------------------------------------------------------------------------------------------------------- candidates
@pytest.mark.parametrize("sps", SPS)
@pytest.mark.parametrize("slack", [0, 2, 8])
def test_candidates_on_noise(hip, sps, slack):
    """Gaussian noise of 2^16 samples, 256 tiles: at slack 8 about 0.7 % of the starts pass (15 033 173 of the 2^32 words lie
    within eight places of the sync codeword, as many of its inverse, and both are listed)"""
    audio = np.random.default_rng(int(sps * 1000) + slack).normal(0.0, 0.6, 1 << 16)
    want = check_candidates(hip, audio, sps, slack=slack)
    if slack == 8:
        assert len(want) > 300


@pytest.mark.parametrize("sps", SPS)
def test_zero_and_full_scale_audio(hip, sps):
    for fill in (0.0, np.pi, -np.pi):
        audio = np.full(9000, fill)
        assert len(check_candidates(hip, audio, sps, slack=8)) == 0  # every comparison an equality: all read 1, sixteen places off


@pytest.mark.parametrize("sps", [4, 40, 128])
def test_shortest_audio_and_a_sync_codeword_on_the_last_sample(hip, sps):
    w = w_of(float(sps))
    full = pocsag.reach(float(sps), w)
    x = T.as_audio(T.sync_rect(sps, t=0, n=full + 2000))
    assert pocsag.n_starts(full - 1, float(sps), w) == 0 and pocsag.n_starts(full, float(sps), w) == 1
    rc, count, got, whole = dev_candidates(hip, x[:full - 1], float(sps), w, 0, 4)
    assert (rc, count, whole) == (0, 0, True) and np.all(got == SENT)
    assert check_candidates(hip, x[:full], float(sps), slack=0).tolist() == [0]      # the one start there is
    rc, count, got, whole = dev_candidates(hip, x[:0], float(sps), w, 0, 4)         # n = 0
    assert (rc, count, whole) == (0, 0, True) and np.all(got == SENT)
    for t in (1, 300, 1021):                                         # the sync codeword ends on the last sample
        y = T.as_audio(T.sync_rect(sps, t=t, n=t + full))
        want = check_candidates(hip, y, float(sps), slack=0)
        assert want[-1] == t == pocsag.n_starts(len(y), float(sps), w) - 1


@pytest.mark.parametrize("edge", [256, 1024])
def test_passes_around_tile_edges(hip, edge):
    for sps in (4, 7):
        for t in (edge - 1, edge, edge + 1):
            want = check_candidates(hip, T.as_audio(T.sync_rect(sps, t=t)), float(sps), slack=0)
            assert t in want
    # a run of adjacent passes that lies across the edge
    x = T.as_audio(T.sync_rect(40, t=edge - 12))
    want = check_candidates(hip, x, 40.0, slack=0)
    assert np.any(want < edge) and np.any(want >= edge) and len(want) >= 16


@pytest.mark.parametrize("polarity", [0, 1])
@pytest.mark.parametrize("wrong", [0, 1, 2, 3])
def test_polarities_and_slack(hip, polarity, wrong):
    for sps in (4, 20):
        x = T.as_audio(T.sync_rect(sps, t=77, wrong=wrong, polarity=polarity))
        w = w_of(float(sps))
        masks = pocsag.masks_host(x, float(sps), w, 2)
        assert masks[77] == (0 if wrong > 2 else (3 if polarity else 1))
        want = check_candidates(hip, x, float(sps), slack=2)
        assert (77 in want) == (wrong <= 2)                          # the list holds both polarities' passes
        det = check_batches(hip, x, float(sps), [77])
        assert det["polarity"][0] == polarity and det["mis"][0] == wrong


@pytest.mark.parametrize("k", range(32))
def test_each_comparison_is_strict(hip, k):
    tie, up, zero = T.tie_cases()[k]
    assert (0 in check_candidates(hip, T.as_audio(tie), 4.0, 3, slack=0)) == (not zero)      # 32 v = S reads 1
    assert (0 in check_candidates(hip, T.as_audio(up), 4.0, 3, slack=0)) == zero


def test_capacities(hip):
    x = pocsag.encode_audio([[(8, 0, "1")]], 9600.0, [50.5], 2400, sigma=0.05, seed=7, preamble=64)
    want = pocsag.candidates_host(x, 4.0, 3)
    m = len(want)
    assert m >= 3
    for cap in (0, 1, m - 1, m, m + 1, m + 5):
        rc, count, got, whole = dev_candidates(hip, x, 4.0, 3, 2, cap)
        assert count == m and whole
        assert rc == (0 if cap >= m else hip.DD_ERR_INVALID)
        kept = min(cap, m)
        assert np.array_equal(got[:kept], want[:kept]) and np.all(got[kept:] == SENT)
    lst, count = pocsag.candidates(hip.DevArray.from_host(x), 4.0, 3, cap=1)     # the wrapper asks again at the true count
    assert count == m and np.array_equal(lst.view(0, m).to_host(), want)


# ---------------------------------------------------------------------------------------------------------------- batches
@pytest.mark.parametrize("fix", [0, 1, 2])
def test_every_error_pattern(hip, fix):
    """the 5488 patterns of one, two and three bits as 343 batches: corrected where the weight is within `fix`, as received else"""
    x, ts, sent, laid = T.pattern_batches()
    det = check_batches(hip, T.as_audio(x), 4.0, ts, 3, fix)
    weight = pocsag.popcount(laid[:, 1:])
    ok = weight <= fix
    assert np.array_equal(det["errs"][:, 1:], np.where(ok, weight, 255)) and np.array_equal(det["good"], ok.sum(axis=1))
    assert np.array_equal(det["words"][:, 1:][ok], sent[:, 1:][ok]) and np.array_equal(det["words"][:, 1:][~ok], (sent ^ laid)[:, 1:][~ok])


@pytest.mark.parametrize("polarity", [0, 1])
def test_two_bit_errors_across_the_halves(hip, polarity):
    """a two-bit error with one bit in each 16-lane half of a codeword's 32 lanes, in both codewords of a ballot word, in the
    codeword the sync codeword shares its ballot with, and in codeword 16, which has a ballot's lower half to itself"""
    body = T.some_codewords(16, 9)
    sent = T.batch_words(body)
    for slot in (1, 2, 3, 8, 15, 16):
        for mask in (0x80000002, 0x00018000, 0x40000001, 0x00010002):
            bad = sent.copy()
            bad[slot] ^= mask
            det = check_batches(hip, T.as_audio(T.rect(T.word_bits(bad), 4, t=5, polarity=polarity)), 4.0, [5], 3)
            assert det["words"][0].tolist() == sent.tolist() and det["errs"][0, slot] == 2 and det["good"][0] == 16
            assert det["polarity"][0] == polarity


@pytest.mark.parametrize("sps", [7.5, 93.75])
def test_fractional_samples_per_bit(hip, sps):
    sent = T.batch_words(T.some_codewords(16, 11))
    bad = sent.copy()
    bad[4] ^= 0x00400100
    bad[9] ^= 0x7
    for polarity in (0, 1):
        x = T.as_audio(T.fractional(T.word_bits(bad), sps, t=301.3, polarity=polarity))
        ts = check_candidates(hip, x, sps, slack=0)
        assert len(ts) >= int(sps) // 2 and np.all(np.abs(ts - 301.3) < sps)
        det = check_batches(hip, x, sps, [301, 302, 305, 299])
        assert det["words"][0, [0, 1, 4]].tolist() == sent[[0, 1, 4]].tolist() and det["errs"][0, 4] == 2 and det["errs"][0, 9] == 255
        assert det["polarity"][0] == polarity and det["good"][0] == 15


def test_a_batch_cut_off_and_starts_outside(hip):
    sent = T.batch_words(T.some_codewords(16, 12))
    x = T.as_audio(T.rect(T.word_bits(sent), 4, t=9))
    for cw in (1, 8, 16):                                            # the audio ends behind codeword cw
        n = 9 + 4 * 32 * (cw + 1)
        det = check_batches(hip, x[:n], 4.0, [9], 3)
        assert det["words"][0, :cw + 1].tolist() == sent[:cw + 1].tolist() and det["good"][0] >= cw
        det = check_batches(hip, x[:n - 3], 4.0, [9], 3)             # and inside its last bit
    n = len(x)
    det = check_batches(hip, x, 4.0, np.array([-1, n, n - 1, 9, 1 << 40, -(1 << 62)]), 3)
    assert det["status"].tolist() == [pocsag.OUTSIDE, pocsag.OUTSIDE, pocsag.OK, pocsag.OK, pocsag.OUTSIDE, pocsag.OUTSIDE]
    assert not det["words"][[0, 1, 4, 5]].any() and not det["errs"][[0, 1, 4, 5]].any() and det["good"][3] == 16


@pytest.mark.parametrize("m", [1, 65, 300])
def test_list_lengths(hip, m):
    x = pocsag.encode_audio([[(8, 0, "12345"), (1000007, 3, "list lengths")]], 9600.0, [50.0], 1200, sigma=0.1, seed=m, preamble=64)
    ts = np.random.default_rng(m).integers(0, len(x), m)
    ts[0] = pocsag.candidates_host(x, 8.0, 5)[0]
    det = check_batches(hip, x, 8.0, ts)
    assert det["good"][0] == 16


# ---------------------------------------------------------------------------------------------------------------- end to end
def same_pages(got, want):
    assert len(got) == len(want)
    for g, v in zip(got, want):
        assert g == v


def test_end_to_end(hip):
    """decode_pocsag over the host test's recording.  Its front end is float32 on the device, which float64 NumPy does not repeat
    bit for bit; so the device decoder is held exactly (pages, batches, frameInfo, candidates) to the restatement run over the
    device's own audio, and to decode_host of the recording in what does not hang on a rounding: the pages' addresses, functions,
    bits and text."""
    raw, starts = T.recording()
    dec = decode_pocsag.decode_pocsag(source.IQarray(np.array(raw), T.FS), T.OFFSET)
    assert dec.audioRate == 48000.0
    audio = dec.audio().to_host()
    found, info, cands, kept = pocsag.decode(audio, dec.audioRate, ops=pocsag.HostOps())
    same_pages(dec.getPages, found)
    assert dec.frameInfo == info and dec.getText == [pocsag.line(p) for p in found] and dec.useful == 1
    words, errs, ts, bauds = dec.getBatches
    assert np.array_equal(words, np.array([b["words"] for b in kept])) and np.array_equal(errs, np.array([b["errs"] for b in kept]))
    assert ts.tolist() == [b["t"] for b in kept] and bauds.tolist() == [512, 1200, 1200, 2400]
    got = dec.candidateInfo
    for baud in pocsag.BAUDS:
        for key in KEYS:
            assert np.array_equal(got[baud][key], cands[baud][key]), (baud, key)
    assert all(T.same_content(p, v) for p, v in zip(found, T.expected_pages())) and len(found) == 5
    assert all(p["corrected"] == 0 and p["complete"] for p in found)
    assert set(dec.timings) == {"front_end", "candidates", "batches", "host"}
    hfound, hinfo = decode_pocsag.decode_host(np.array(raw), T.FS, T.OFFSET)
    assert len(hfound) == 5 and hinfo["batches"] == info["batches"] == 4
    for g, v in zip(dec.getPages, hfound):
        for key in ("baud", "polarity", "address", "function", "nbits", "bits", "text", "kind", "complete", "batches"):
            assert g[key] == v[key], key
        assert abs(g["start"] - v["start"]) <= 48000.0 / g["baud"]               # the merge picks one start of a bit time of them
    same = decode_pocsag.decode_pocsag(source.IQarray(np.array(raw), T.FS), T.OFFSET, use_device_raw=False)
    same_pages(same.getPages, found)


def test_from_audio(hip):
    rate = 48000.0
    tx = [[(1234560, 0, "0800-555"), (1000007, 3, "from audio")], [(77, 2, "")], [(4242, 3, "x" * 60)]]
    x = pocsag.encode_audio(tx, rate, [300.25, 120000.5, 170000.75], (512, 1200, 2400), (1, 0, 0), sigma=0.3, seed=4,
                            carrier_offsets=(-800.0, 0.0, 800.0), preamble=(32, 576, 576))
    found, info = decode_pocsag.decode_audio_host(x, rate)
    assert [(p["address"], p["text"], p["kind"]) for p in found] == [(1234560, "0800-555", "numeric"), (1000007, "from audio", "alpha"),
                                                                     (77, "", "tone"), (4242, "x" * 60, "alpha")]
    for audio in (x, hip.DevArray.from_host(x)):
        dec = decode_pocsag.decode_pocsag.fromAudio(audio, rate)
        same_pages(dec.getPages, found)
        assert dec.frameInfo == info
    empty = decode_pocsag.decode_pocsag.fromAudio(np.zeros(10), rate)
    assert empty.getPages == [] and empty.useful == 0 and empty.frameInfo["pages"] == 0 and empty.getBatches[0].shape == (0, 17)


def test_following_a_lost_sync_codeword(hip):
    rate = 48000.0
    tx = [(1000007, 3, "crosses the second batch's sync codeword"), (4247, 0, "555")]
    flips = [{(1, 0): 0x80908080}]                                   # five places of the second batch's sync codeword
    x = pocsag.encode_audio([tx], rate, [200.5], 1200, 0, sigma=0.1, seed=6, carrier_offsets=300.0, flips=flips)
    dev = hip.DevArray.from_host(x)
    dec = decode_pocsag.decode_pocsag.fromAudio(dev, rate, bauds=(1200,), follow=1)
    assert [p["text"] for p in dec.getPages] == [tx[0][2], "555"] and dec.getPages[0]["complete"] and dec.getPages[0]["batches"] == 2
    assert dec.frameInfo["bauds"][1200]["followed"] == 1 and dec.frameInfo["batches"] == 2
    assert dec.getBatches[1][1, 0] == 5                              # the followed batch's sync codeword: five places off
    same_pages(dec.getPages, decode_pocsag.decode_audio_host(x, rate, (1200,), follow=1)[0])
    cut = decode_pocsag.decode_pocsag.fromAudio(dev, rate, bauds=(1200,), follow=0)
    assert len(cut.getPages) == 1 and len(cut.getPages[0]["text"]) < len(tx[0][2]) and cut.frameInfo["bauds"][1200]["followed"] == 0
    same_pages(cut.getPages, decode_pocsag.decode_audio_host(x, rate, (1200,), follow=0)[0])


def test_a_recording_that_starts_inside_a_transmission(hip):
    """cut a few samples before the second batch's sync codeword the recording still gives that batch's pages; cut inside the
    second batch it gives the third's and the fourth's"""
    rate = 48000.0
    tx = [(1000007, 3, "crosses the second batch's sync codeword"), (4247, 0, "555")] + [(90001, 3, "third batch")] * 2
    clean = pocsag.encode_audio([tx], rate, [200.5], 2400, 1, sigma=0.1, seed=7)
    second = int(pocsag.batch_start(rate, 2400, 200.5, 1))
    for cut, want in ((second - 10, ["555", "third batch", "third batch"]), (second + 5000, ["third batch"] * 2)):
        dec = decode_pocsag.decode_pocsag.fromAudio(clean[cut:], rate)
        assert [p["text"] for p in dec.getPages] == want and all(p["polarity"] == 1 and p["baud"] == 2400 for p in dec.getPages)
        same_pages(dec.getPages, decode_pocsag.decode_audio_host(clean[cut:], rate)[0])
