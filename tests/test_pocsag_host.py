"""The host side of the POCSAG decoder (directdemod_amd/pocsag.py, decode_pocsag.decode_host): the block code, the numeric and
alphanumeric codecs, the pages, the merge and the chain, the limits, and the NumPy restatement of the kernels on the shared
recording.  No GPU."""
import numpy as np
import pytest

import _pocsag as T
import directdemod_amd
from directdemod_amd import decode_pocsag, pocsag, source


# ---------------------------------------------------------------------------------------------------------------- the block code
def test_the_fixed_codewords_and_the_encoder():
    for word in (pocsag.FSC, pocsag.IDLE):
        assert pocsag.syndrome(word) == 0 and pocsag.popcount(word) == 16
        assert pocsag.bch_encode(word >> 11) == word
    words = T.some_codewords(3000, 1)
    assert not np.any(pocsag.syndrome(words)) and not np.any(pocsag.popcount(words) & 1)
    assert np.array_equal(pocsag.bch_encode(words >> 11), words)
    assert pocsag.GEN == (1 << 10) | (1 << 9) | (1 << 8) | (1 << 6) | (1 << 5) | (1 << 3) | 1
    # the remainder by long division, bit by bit, against the table route
    for word in words[:50].tolist():
        r = word >> 1
        for p in range(30, 9, -1):
            if (r >> p) & 1:
                r ^= pocsag.GEN << (p - 10)
        assert r == 0


def test_the_496_syndromes_are_distinct():
    one = [pocsag.syndrome(1 << p) for p in range(1, 32)]
    two = [pocsag.syndrome((1 << p) | (1 << r)) for p in range(1, 32) for r in range(p + 1, 32)]
    assert len(one) == 31 and len(two) == 465 and len(set(one + two)) == 496 and 0 not in one + two
    assert pocsag.syndrome(1) == 0                                   # the parity bit is outside the BCH code


def test_every_pattern_of_one_two_and_three_bits():
    pats = T.patterns()
    assert len(pats) == 5488
    weight = pocsag.popcount(pats)
    for cw in (pocsag.IDLE, pocsag.bch_encode(0x1ABCDE), pocsag.bch_encode(0x012345)):
        fixed, errs = pocsag.correct(pats ^ cw)
        assert np.all(fixed[weight <= 2] == cw) and np.array_equal(errs[weight <= 2], weight[weight <= 2])
        assert np.all(errs[weight == 3] == pocsag.UNCORRECTABLE) and np.array_equal(fixed[weight == 3], (pats ^ cw)[weight == 3])
    assert pocsag.correct(pocsag.IDLE) == (pocsag.IDLE, 0)           # scalars too


def test_fix_limits():
    cw = pocsag.bch_encode(0x155555)
    pats = T.patterns((1, 2))
    weight = pocsag.popcount(pats)
    for fix in (0, 1, 2):
        fixed, errs = pocsag.correct(pats ^ cw, fix)
        ok = weight <= fix
        assert np.all(fixed[ok] == cw) and np.array_equal(errs[ok], weight[ok])
        assert np.all(errs[~ok] == pocsag.UNCORRECTABLE) and np.array_equal(fixed[~ok], (pats ^ cw)[~ok])
        assert pocsag.correct(cw, fix) == (cw, 0)
    assert pocsag.correct(cw ^ 1, 0) == (cw ^ 1, pocsag.UNCORRECTABLE)          # a lone parity-bit error counts as one error
    assert pocsag.correct(cw ^ 1, 1) == (cw, 1)
    assert pocsag.correct(cw ^ 0x80000001, 1) == (cw ^ 0x80000001, pocsag.UNCORRECTABLE) and pocsag.correct(cw ^ 0x80000001, 2) == (cw, 2)


def test_a_random_word_decodes_about_one_time_in_four():
    words = np.random.default_rng(3).integers(0, 1 << 32, 200000)
    share = np.mean(pocsag.correct(words)[1] != pocsag.UNCORRECTABLE)
    assert abs(share - (1 + 31 + 465 + 1 + 31) * 2.0 ** 21 / 2.0 ** 32) < 0.005   # 529 patterns around each of 2^21 codewords: 0.258


# ---------------------------------------------------------------------------------------------------------------- the codecs
def test_numeric_codec():
    assert pocsag.numeric(pocsag.numeric_bits(pocsag.NUMERIC)) == pocsag.NUMERIC
    assert len(pocsag.numeric_bits(pocsag.NUMERIC)) == 80             # 16 characters: four codewords
    assert pocsag.numeric_bits("1").tolist()[:8] == [1, 0, 0, 0, 0, 0, 1, 1]     # least significant bit first, then the space fill
    assert pocsag.numeric(pocsag.numeric_bits("911")) == "911" and len(pocsag.numeric_bits("911")) == 20
    assert pocsag.numeric(pocsag.numeric_bits("12 34-5")) == "12 34-5"
    with pytest.raises(ValueError):
        pocsag.numeric_bits("12a")


def test_alpha_codec():
    assert pocsag.alpha_bits("A").tolist()[:7] == [1, 0, 0, 0, 0, 0, 1]
    for text in ("", "A", "abc", "Hello, world", "".join(chr(c) for c in range(32, 127))):
        bits = pocsag.alpha_bits(text)
        assert len(bits) % 20 == 0 and pocsag.alpha(bits) == text
    bits = pocsag.alpha_bits("abc")                                  # 21 bits: the third character is split across two codewords
    assert len(bits) == 40 and pocsag.alpha(bits[:20]) == "ab" and pocsag.alpha(bits) == "abc"
    tail = pocsag.alpha_bits("xy\x03\x04\x00")
    assert pocsag.alpha(tail) == "xy"                                # trailing ETX, EOT and NUL are dropped
    assert pocsag.alpha(pocsag.alpha_bits("x\x03y")) == "x\x03y"     # not one inside
    with pytest.raises(ValueError):
        pocsag.alpha_bits("é")


# ---------------------------------------------------------------------------------------------------------------- pages
def batch(body, t=0, sps=40.0, baud=1200, errs=None):
    e = np.zeros(pocsag.WORDS, dtype=np.uint8)
    for slot, v in (errs or {}).items():
        e[slot] = v
    return {"t": t, "baud": baud, "sps": sps, "words": T.batch_words(body).astype(np.uint32), "errs": e, "polarity": 0, "good": 16,
            "mis": 0, "score": 0, "corrected": 0, "followed": False}


def slots(entries):
    """16 codewords: idle, with `entries` {slot (1 .. 16): codeword}"""
    body = [pocsag.IDLE] * 16
    for slot, w in entries.items():
        body[slot - 1] = w
    return body


def test_pages_across_a_batch_edge():
    text = "runs into the next batch"
    msg = pocsag.message_words(pocsag.alpha_bits(text))
    assert len(msg) == 9
    first = slots({15: pocsag.address_word(1000007, 3), 16: msg[0]})
    second = slots({i + 1: w for i, w in enumerate(msg[1:])})
    tx = [batch(first, t=100), batch(second, t=100 + 544 * 40)]
    got, counts = pocsag.pages(tx, 48000.0)
    assert len(got) == 1 and counts["orphans"] == 0 and counts["idle"] == 14 + 8 and counts["codewords"] == {0: 32, 1: 0, 2: 0}
    p = got[0]
    assert (p["address"], p["function"], p["kind"], p["text"], p["alpha"]) == (1000007, 3, "alpha", text, text)
    assert p["nbits"] == 180 and len(p["bits"]) == 23 and p["batches"] == 2 and p["complete"] and p["corrected"] == 0
    assert p["start"] == 100 + 32 * 15 * 40 and p["t"] == p["start"] / 48000.0 and p["baud"] == 1200 and p["polarity"] == 0
    assert pocsag.line(p) == "POCSAG1200: Address: 1000007 Function: 3 Alpha: " + text
    assert pocsag.transmission_words([(1000007, 3, text)]).tolist() == [T.batch_words(first).tolist(), T.batch_words(second).tolist()]


def test_two_pages_in_a_batch_and_how_a_page_closes():
    num = pocsag.message_words(pocsag.numeric_bits("12345"))
    alp = pocsag.message_words(pocsag.alpha_bits("hi"))
    body = slots({1: pocsag.address_word(8, 0), 2: num[0], 3: pocsag.address_word(4097, 3), 4: alp[0]})
    got, counts = pocsag.pages([batch(body)], 48000.0)
    assert [(p["address"], p["function"], p["kind"], p["text"], p["complete"]) for p in got] == [(8, 0, "numeric", "12345", True),
                                                                                               (4097, 3, "alpha", "hi", True)]
    assert counts["idle"] == 12                                      # the first closed by an address, the second by idle
    # closed by the transmission's end
    got, _ = pocsag.pages([batch(slots({15: pocsag.address_word(7, 0), 16: num[0]}))], 48000.0)
    assert len(got) == 1 and got[0]["complete"] and got[0]["text"] == "12345" and got[0]["address"] == 7
    # closed by an uncorrectable codeword: what came before stays, what comes behind is an orphan
    long = pocsag.message_words(pocsag.numeric_bits("1234567890" * 2))
    body = slots({1: pocsag.address_word(8, 0), 2: long[0], 3: long[1], 4: long[2], 5: long[3]})
    got, counts = pocsag.pages([batch(body, errs={1: 1, 2: 2, 4: pocsag.UNCORRECTABLE})], 48000.0)
    assert len(got) == 1 and not got[0]["complete"] and got[0]["text"] == "1234567890" and got[0]["corrected"] == 3
    assert counts["uncorrectable"] == 1 and counts["orphans"] == 1 and counts["codewords"] == {0: 13, 1: 1, 2: 1}
    # an address codeword alone: a tone page
    got, _ = pocsag.pages([batch(slots({5: pocsag.address_word(18, 2)}))], 48000.0)
    assert (got[0]["kind"], got[0]["text"], got[0]["nbits"], got[0]["address"], got[0]["function"]) == ("tone", "", 0, 18, 2)
    assert pocsag.line(got[0]).endswith("Function: 2 Tone")


def test_orphans_wrong_frames_and_content():
    msg = pocsag.message_words(pocsag.alpha_bits("abc"))
    got, counts = pocsag.pages([batch(slots({1: msg[0], 2: msg[1]}))], 48000.0)
    assert got == [] and counts["orphans"] == 2
    # an address whose low bits say frame 5, sent in frame 2 (slot 6): parsed by position
    got, _ = pocsag.pages([batch(slots({6: pocsag.address_word(1005, 3), 7: msg[0], 8: msg[1]}))], 48000.0)
    assert got[0]["address"] == (1005 & ~7) | 2 and got[0]["text"] == "abc"
    # functions 1 and 2: alpha when every character prints, else numeric; content forces either
    num = pocsag.message_words(pocsag.numeric_bits("0123456789"))
    body = slots({1: pocsag.address_word(8, 1), 2: msg[0], 3: msg[1], 5: pocsag.address_word(16, 2), 6: num[0], 7: num[1]})
    got, _ = pocsag.pages([batch(body)], 48000.0)
    assert [(p["kind"], p["text"]) for p in got] == [("alpha", "abc"), ("numeric", "0123456789")]
    got, _ = pocsag.pages([batch(body)], 48000.0, "numeric")
    assert [p["kind"] for p in got] == ["numeric", "numeric"] and got[1]["text"] == "0123456789"
    got, _ = pocsag.pages([batch(body)], 48000.0, "alpha")
    assert [p["kind"] for p in got] == ["alpha", "alpha"] and got[0]["text"] == "abc"


# ---------------------------------------------------------------------------------------------------------------- merge and chain
def det_of(rows):
    """a candidates' dict from (t, errs of the 16, score)"""
    det = pocsag._empty_det(len(rows))
    for i, (t, errs, score) in enumerate(rows):
        det["t"][i], det["score"][i], det["status"][i] = t, score, pocsag.OK
        det["errs"][i, 1:] = errs
        det["good"][i] = np.count_nonzero(np.asarray(errs) != 255)
        det["words"][i] = T.batch_words()
    return det


def test_merge_collapses_adjacent_starts():
    clean, one, bad = [0] * 16, [1] + [0] * 15, [255] * 5 + [0] * 11
    det = det_of([(1000, one, 900), (1010, clean, 500), (1020, clean, 700), (1039, clean, 700), (1041, clean, 990), (1500, bad, 999),
                  (30000, [255] * 4 + [2] * 12, 5)])
    keep, dup = pocsag.merge(det, 40.0)
    assert keep == [2, 4, 6] and dup == 3         # fewest repaired, then the largest score, then the earliest; 1041 is past one bit time
    assert pocsag.accepted(det) == [0, 1, 2, 3, 4, 6]
    assert pocsag.merge(det_of([]), 40.0) == ([], 0)


def test_overlapping_detections_at_two_baud_rates_resolve_to_one():
    a = pocsag.batch_of(det_of([(1000, [1] * 3 + [0] * 13, 5)]), 0, 1200, 40.0)
    b = pocsag.batch_of(det_of([(9000, [255] * 4 + [2] * 12, 5)]), 0, 2400, 20.0)
    c = pocsag.batch_of(det_of([(1000 + 544 * 40, [0] * 16, 5)]), 0, 1200, 40.0)
    d = pocsag.batch_of(det_of([(100000, [2] * 16, 5)]), 0, 2400, 20.0)
    kept, dropped = pocsag.resolve([a, b, c, d])
    assert [k["t"] for k in kept] == [1000, 1000 + 544 * 40, 100000] and dropped == 1
    assert a["corrected"] == 3 and b["corrected"] == 24
    kept, dropped = pocsag.resolve([b, d])                           # alone it stays
    assert len(kept) == 2 and dropped == 0


def test_chain_and_a_gap_of_two_batches():
    step = 544 * 40
    mk = lambda t, pol=0: dict(pocsag.batch_of(det_of([(t, [0] * 16, 5)]), 0, 1200, 40.0), polarity=pol)
    runs = pocsag.chain([mk(500), mk(500 + step + 20), mk(500 + 2 * step + 3), mk(500 + 5 * step), mk(500 + 6 * step - 21)], 40.0)
    assert [[b["t"] - 500 for b in tx] for tx in runs] == [[0, step + 20, 2 * step + 3], [5 * step], [6 * step - 21]]
    runs = pocsag.chain([mk(500), mk(500 + step, 1)], 40.0)          # the other polarity is another transmission
    assert len(runs) == 2
    # a follower supplied at the predicted start joins, at most `follow` in a row
    asked = []

    def extend(asks):
        asked.extend(at for at, pol in asks)
        return [dict(mk(at, pol), followed=True) for at, pol in asks]
    runs = pocsag.chain([mk(500), mk(500 + 3 * step)], 40.0, extend, 2)
    assert len(runs) == 1 and [b["followed"] for b in runs[0]] == [False, True, True, False, True, True]
    assert asked[:4] == [500 + step, 500 + 4 * step, 500 + 2 * step, 500 + 5 * step]      # one call per round
    runs = pocsag.chain([mk(500), mk(500 + 3 * step)], 40.0, extend, 1)
    assert [len(tx) for tx in runs] == [2, 2]
    assert pocsag.next_start(500, 93.75) == 500 + 51000


# ---------------------------------------------------------------------------------------------------------------- limits
def test_params_and_limits():
    assert pocsag.params(48000, 1200) == (40.0, 25, 2, 2) and pocsag.params(48000, 512)[:2] == (93.75, 57)
    assert pocsag.params(48000, 2400)[1] == 13 and pocsag.params(9600, 2400)[1] == 3 and pocsag.params(128 * 512, 512)[1] == 77
    for rate in (3.9 * 1200, 128.1 * 1200, float("nan")):
        with pytest.raises(ValueError, match="samples per bit"):
            pocsag.params(rate, 1200)
        with pytest.raises(ValueError):
            decode_pocsag.decode_pocsag.fromAudio(np.zeros(10), rate, bauds=(1200,))
    assert pocsag.params(4.0 * 1200, 1200)[0] == 4.0 and pocsag.params(128.0 * 1200, 1200)[0] == 128.0
    for w in (0, 2, 22, 79):
        with pytest.raises(ValueError):
            pocsag.params(48000, 1200, w)
    for kw in ({"slack": 9}, {"slack": -1}, {"fix": 3}, {"fix": -1}, {"content": "hex"}, {"follow": -1}):
        with pytest.raises(ValueError):
            decode_pocsag.decode_pocsag.fromAudio(np.zeros(10), 48000.0, **kw)
        with pytest.raises(ValueError):
            decode_pocsag.decode_pocsag(source.IQarray(np.zeros((1000, 2), np.uint8), 240000), 0.0, **kw)
    with pytest.raises(ValueError):
        pocsag.params(48000, 1200, None, 9)
    with pytest.raises(ValueError):
        pocsag.params(48000, 1200, None, 2, 3)
    raw = source.IQarray(np.zeros((1000, 2), np.uint8), 240000)
    with pytest.raises(ValueError, match="samples per bit"):
        decode_pocsag.decode_pocsag(raw, 0.0, bw=8000)               # 8 kS/s: 3.33 samples per bit at 2400 baud
    with pytest.raises(ValueError, match="samples per bit"):
        decode_pocsag.decode_pocsag(raw, 0.0, bw=80000)              # 80 kS/s: 156 samples per bit at 512 baud
    assert decode_pocsag.decode_pocsag(raw, 0.0, bw=80000, bauds=(1200, 2400)).audioRate == 80000.0


def test_all_entries():
    assert "pocsag" in directdemod_amd.__all__ and "decode_pocsag" in directdemod_amd.__all__


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_quantiser_and_strict_comparisons_in_the_restatement():
    k = np.random.default_rng(3).integers(-(1 << 21), (1 << 21) + 1, 50000)
    assert np.array_equal(pocsag.quantise(T.as_audio(k)), k)
    for k, (tie, up, zero) in enumerate(T.tie_cases()):
        v = pocsag.values(pocsag.quantise(T.as_audio(tie)), [0], np.arange(32), 4.0, 3)[0]
        assert 32 * v[k] == v.sum() and np.count_nonzero(32 * v == v.sum()) == 1, k
        assert (0 in pocsag.candidates_host(T.as_audio(tie), 4.0, 3, 0)) == (not zero), k      # equality reads 1
        assert (0 in pocsag.candidates_host(T.as_audio(up), 4.0, 3, 0)) == zero, k


def test_crafted_batches_in_the_restatement():
    x, ts, sent, laid = T.pattern_batches()
    weight = pocsag.popcount(laid[:, 1:])
    for fix in (0, 1, 2):
        det = pocsag.batches_host(T.as_audio(x), 4.0, 3, fix, ts)
        ok = weight <= fix
        assert np.all(det["status"] == pocsag.OK) and not det["polarity"].any() and not det["mis"].any()
        assert np.array_equal(det["words"][:, 0], sent[:, 0]) and np.array_equal(det["words"][:, 1:][ok], sent[:, 1:][ok])
        assert np.array_equal(det["words"][:, 1:][~ok], (sent ^ laid)[:, 1:][~ok])
        assert np.array_equal(det["errs"][:, 1:], np.where(ok, weight, 255)) and np.array_equal(det["good"], ok.sum(axis=1))
    for sps, w in ((4, 3), (40, 23), (128, 77)):
        words = T.batch_words(T.some_codewords(16, sps))
        for pol in (0, 1):
            y = T.as_audio(T.rect(T.word_bits(words), sps, t=37, polarity=pol))
            assert 37 in pocsag.candidates_host(y, float(sps), w, 0)
            det = pocsag.batches_host(y, float(sps), w, 2, [37, -1, len(y)])
            assert det["words"][0].tolist() == words.tolist() and det["polarity"][0] == pol and det["good"][0] == 16
            assert det["status"].tolist() == [pocsag.OK, pocsag.OUTSIDE, pocsag.OUTSIDE] and not det["words"][1:].any()


@pytest.fixture(scope="module")
def decoded():
    raw, starts = T.recording()
    return decode_pocsag.decode_host(raw, T.FS, T.OFFSET)


def test_decode_host_finds_every_page(decoded):
    found, info = decoded
    assert min(T.ebn0_db(T.AMPLITUDE, T.SIGMA, T.FS, b) for b in T.BAUDS) >= 30.0
    want = T.expected_pages()
    assert len(found) == len(want) == 5 and info["pages"] == 5
    for p, v in zip(found, want):
        assert T.same_content(p, v), (p, v)
        assert p["corrected"] == 0 and p["complete"]
    assert [p["kind"] for p in found] == ["numeric", "alpha", "alpha", "alpha", "numeric"]
    assert [p["polarity"] for p in found] == [0, 0, 0, 1, 1] and [p["batches"] for p in found] == [1, 1, 2, 1, 1]
    assert info["codewords"][0] == 16 * info["batches"] and info["batches"] == 4 and info["transmissions"] == 3
    assert info["uncorrectable"] == 0 and info["orphans"] == 0 and info["overlaps"] == 0
    for baud, nb in zip(T.BAUDS, (1, 2, 1)):
        assert info["bauds"][baud]["accepted"] == nb and info["bauds"][baud]["followed"] == 0
        assert info["bauds"][baud]["duplicates"] >= nb * 48000 // baud // 2      # about one bit time of adjacent starts per batch
    raw, starts = T.recording()
    at = pocsag.batch_start(T.FS, 1200, starts[1], 0) / 5.0 + 32 * 15 * 40      # the alpha page's address is slot 15 of the first batch
    delay = 7 / 5.0 + 20 - 0.5                                                  # the 15-tap window at 240 kS/s, the 41-tap low-pass, the discriminator
    assert abs(found[2]["start"] - at - delay) <= 20                            # within half a bit time


def test_audio_level_decode_follow_and_a_cold_start():
    rate = 48000.0
    tx = [(1000007, 3, "crosses the second batch's sync codeword"), (4247, 0, "555")]
    flips = [{(1, 0): 0x80808088 ^ 0x00000008 ^ 0x00100000}]         # five places of the second batch's sync codeword
    assert bin(flips[0][(1, 0)]).count("1") == 5
    x = pocsag.encode_audio([tx], rate, [200.5], 1200, 0, sigma=0.1, seed=6, carrier_offsets=300.0, flips=flips)
    whole, info = decode_pocsag.decode_audio_host(x, rate, (1200,), follow=1)
    assert [p["text"] for p in whole] == [tx[0][2], "555"] and info["bauds"][1200]["followed"] == 1 and info["batches"] == 2
    cut, info = decode_pocsag.decode_audio_host(x, rate, (1200,), follow=0)
    assert len(cut) == 1 and cut[0]["address"] == 1000007 and len(cut[0]["text"]) < len(tx[0][2]) and info["bauds"][1200]["followed"] == 0
    # a recording that starts a few samples before a transmission's second batch, and one that starts inside it
    clean = pocsag.encode_audio([tx + [(90001, 3, "third batch")] * 2], rate, [200.5], 2400, 1, sigma=0.1, seed=7)
    second = int(pocsag.batch_start(rate, 2400, 200.5, 1))
    got, _ = decode_pocsag.decode_audio_host(clean[second - 10:], rate)
    assert [p["text"] for p in got][:1] == ["555"] and [p["text"] for p in got][1:] == ["third batch"] * 2
    got, info = decode_pocsag.decode_audio_host(clean[second + 5000:], rate)
    assert len(got) >= 1 and all(p["text"] == "third batch" and p["polarity"] == 1 for p in got) and info["batches"] >= 1


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
    assert lib.dd_pocsag_candidates(None, 0, 40.0, 23, 2, None, 0, C.byref(count), None) == 0 and count.value == 0
    assert lib.dd_pocsag_batches(None, 0, 40.0, 23, 2, None, 5, None, None, None, None, None) == 0
    assert lib.dd_pocsag_batches(None, 5000, 40.0, 23, 2, None, 0, None, None, None, None, None) == 0
    assert lib.dd_debug_pocsag_masks(None, 0, 40.0, 23, 2, None, None) == 0
    # null buffers with n > 0
    assert lib.dd_pocsag_candidates(None, 5000, 40.0, 23, 2, None, 0, C.byref(count), None) == bad
    assert lib.dd_pocsag_candidates(None, 5000, 40.0, 23, 2, None, 0, None, None) == bad
    assert lib.dd_pocsag_batches(None, 5000, 40.0, 23, 2, None, 5, None, None, None, None, None) == bad
    assert lib.dd_debug_pocsag_masks(None, 5000, 40.0, 23, 2, None, None) == bad
    assert b"null buffer" in lib.dd_last_error()
    # sizes, samples per bit, windows, slack and fix, with buffers that must not be touched
    wild = C.c_void_p(16)
    for n, sps, w, cap in ((-1, 40.0, 23, 8), (5000, 3.99, 3, 8), (5000, 128.01, 77, 8), (5000, float("nan"), 3, 8), (5000, 40.0, 2, 8),
                           (5000, 40.0, 0, 8), (5000, 128.0, 79, 8), (5000, 40.0, 23, -1), (1 << 31, 40.0, 23, 8)):
        assert lib.dd_pocsag_candidates(wild, n, sps, w, 2, wild, cap, C.byref(count), None) == bad
        assert lib.dd_pocsag_batches(wild, n, sps, w, 2, wild, cap, wild, wild, wild, wild, None) == bad
        if cap >= 0:
            assert lib.dd_debug_pocsag_masks(wild, n, sps, w, 2, wild, None) == bad
    for slack in (-1, 9):
        assert lib.dd_pocsag_candidates(wild, 5000, 40.0, 23, slack, wild, 8, C.byref(count), None) == bad
        assert lib.dd_debug_pocsag_masks(wild, 5000, 40.0, 23, slack, wild, None) == bad
    for fix in (-1, 3):
        assert lib.dd_pocsag_batches(wild, 5000, 40.0, 23, fix, wild, 8, wild, wild, wild, wild, None) == bad
