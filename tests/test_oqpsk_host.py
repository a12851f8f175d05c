"""The OQPSK walk's definition on the CPU: the table phasor against np.exp, the Python restatement
(tests/_oqpsk.py walk_host) on synthesised recordings at both symbol rates and both lock outcomes, its branch counters, the
re-stagger and the rule by which decode_lrpt's stagger="auto" chooses, and one recording through the whole NumPy chain."""
import numpy as np
import pytest

import _lrpt_modes
import _oqpsk as oq
from directdemod_amd import lrpt, oqpsk


def test_table_and_constants_are_the_package_s():
    assert np.array_equal(oq.table(), oqpsk.phasor_table()) and oq.table().shape == (1024, 2)
    for rate in oq.RATES:
        assert np.array_equal(oq.params_array(oq.params(rate))[:7], np.array(oqpsk.leading_params(oq.FS, rate)))
    assert (oq.AMEAN0, oq.BW, oq.start_state(72000)["freq"]) == (oqpsk.AMEAN0, oqpsk.COSTAS_BW, oqpsk.FREQ0)
    assert oqpsk.STATE.names == oq.FLOAT_FIELDS + oq.INT_FIELDS and oqpsk.STATE.itemsize == 160


def test_phasor_against_exp():
    """0, every table knot, the largest float below 1, the floats around the knots and a random grid: within 1e-12 of np.exp (the
    polynomials' truncation is below 1e-15 for d < 2 pi / 1024; the bound leaves room for the roundings of np.exp's argument)"""
    knots = np.arange(1024) / 1024.0
    rng = np.random.Generator(np.random.PCG64(7))
    u = np.concatenate(([0.0, np.nextafter(1.0, 0.0)], knots, np.nextafter(knots[1:], 0.0), np.nextafter(knots, 1.0), rng.random(20000)))
    assert u.min() == 0.0 and u.max() < 1.0
    got = oqpsk.phasor_np(u)
    assert np.max(np.abs(got - np.exp(2j * np.pi * u))) < 1e-12
    tab = oq.table().tolist()
    one = np.array([complex(*oq.phasor(float(v), tab)) for v in u[:4100]])
    assert np.array_equal(one.view(np.int64), got[:4100].view(np.int64))          # the scalar and the array form: the same bits
    assert got[0] == 1.0 and oq.frac(-1e-20) == 0.0 and oq.frac(1.25) == 0.25 and oq.frac(-0.25) == 0.75 and oq.frac(float("nan")) == 0.0


@pytest.fixture(scope="module")
def walked():
    """name -> (recording, walk_host's state, arrays, counters) of RECORDINGS, each walked once"""
    cache = {}

    def get(name):
        if name not in cache:
            c = oq.RECORDINGS[name]
            rec = oq.recording(**c)
            x = oq.front_end(rec["raw"], rec["carrier"], c["symbol_rate"])
            cache[name] = (rec,) + oq.walk_host(x, 0, oq.start_state(c["symbol_rate"]), oq.params(c["symbol_rate"]))
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(oq.RECORDINGS))
def test_walk_decides_every_bit_past_acquisition(walked, name):
    rec, state, arr, cnt = walked(name)
    rot, ok = oq.decisions(arr, rec["code"], rec["symbol_rate"])
    want = 0 if name.endswith("s0") else 1
    assert rot % 2 == want, (name, rot)
    bad = np.nonzero(~ok.all(axis=1))[0]
    print("\n[oqpsk] %s: rotation %d, %d symbols, last wrong decision at symbol %d" % (name, rot, len(ok), bad[-1] if len(bad) else -1))
    assert len(ok) > 0.95 * 0.9 * rec["symbol_rate"] and ok[oq.ACQ:].all(), (name, bad[-5:])
    assert state["overflow"] == 0 and cnt["b_before_a"] == 1 and cnt["a_events"] >= state["ctr"] == len(ok)
    # the stagger the rails come out with: 0 at 0 / 180 degrees, -1 at 90 / 270
    soft = lrpt.soft_np(arr["sym"])
    scores = lrpt.stagger_scores_np(soft, len(ok), template=lrpt.ASM_ENCODED_NRZM)
    assert lrpt.stagger_pick(scores) == -want and 4 * sorted(scores)[1] < 3.5 * max(scores), scores


@pytest.mark.parametrize("name", sorted(oq.CASES))
def test_named_cases_reach_their_branches(name):
    rate, x, st = oq.case(name)
    s, arr, cnt = oq.walk_host(x, 0, st, oq.params(rate))
    for key in oq.CASES[name]["reaches"]:
        assert cnt[key] > 0, (key, cnt)
    assert len(arr["sym"]) == s["ctr"] - st["ctr"] and np.all(np.isfinite(arr["uf"])) and np.all((arr["uf"][:, 0] >= 0) & (arr["uf"][:, 0] < 1))
    if name == "a_run":
        assert cnt["a_events"] > 2 * oq.TILE and cnt["b_events"] < cnt["a_events"] - 2 * oq.TILE
    assert cnt["pmean_margin"] > 1e-9                     # no lock decision hangs on a last bit


def test_length_runs_put_their_event_where_they_say():
    for rate in oq.RATES:
        x = oq.signal(rate, **oq.LENGTH_SIGNAL)
        for n, timing, event in oq.length_runs(rate):
            if event is None:
                continue
            st = oq.start_state(rate, timing=timing, seen_a=1)
            s, arr, cnt = oq.walk_host(x[:event[1] + 1], 0, st, oq.params(rate))
            first = cnt["a_events"] if event[0] == "A" else cnt["b_events"]
            assert first == 1 and (s["aidx"] if event[0] == "A" else (arr["bidx"][-1] if len(arr["bidx"]) else -1)) == event[1], (n, event)


@pytest.mark.parametrize("nsym", [0, 1, 2, 5])
def test_restagger_np(nsym):
    soft = (np.arange(2 * nsym + 4) * 7 - 128).astype(np.int8)          # longer than nsym pairs: the rest is not read
    i, q = soft[0:2 * nsym:2], soft[1:2 * nsym:2]
    for s in (-1, 0, 1):
        got = lrpt.restagger_np(soft, nsym, s)
        pairs = [(i[k], q[k + s]) for k in range(nsym) if 0 <= k + s < nsym]
        assert got.dtype == np.int8 and len(got) == 2 * max(nsym - abs(s), 0) == 2 * len(pairs)
        assert got.tolist() == [int(v) for p in pairs for v in p]
    for bad in (2, -2):
        with pytest.raises(ValueError):
            lrpt.restagger_np(soft, nsym, bad)


def test_stagger_pick_order():
    assert lrpt.STAGGERS == (0, -1, 1)
    assert [lrpt.stagger_pick(v) for v in ([5, 5, 5], [1, 5, 5], [1, 2, 3], [0, 0, 0], [3, 2, 3])] == [0, -1, 1, 0, 0]


@pytest.mark.parametrize("differential,interleaved", [(False, False), (True, False), (True, True)])
def test_auto_rule_on_restaggered_streams(differential, interleaved):
    """A stream whose rails were moved apart by -s is recognised as stagger s.  Under a wrong stagger the 52 scored bits of a frame
    marker are half random (about 39 of 52: below MIN_SCORE, no frame start).  The 8-bit marker 0x27 does better: its I rail reads
    0 1 0 1, so at the neighbouring offset and with the I rail inverted seven of its bits match and one is random -- 15/16 of
    the right stagger's score, with a scatter of 0.2 % over the roughly 900 markers here: the bound is 0.95."""
    s0 = _lrpt_modes.stream(_lrpt_modes.random_bodies(650, 3), 651, differential=differential, interleaved=interleaved, prefix=77, hyp=5)
    template = lrpt.ASM_ENCODED_NRZM if differential else lrpt.ASM_ENCODED
    for s in (0, -1, 1):
        soft = lrpt.restagger_np(s0["soft"], s0["nsym"], -s)
        scores = lrpt.stagger_scores_np(soft, len(soft) // 2, interleaved=interleaved, template=template)
        assert lrpt.stagger_pick(scores) == s, (s, scores)
        best = scores[lrpt.STAGGERS.index(s)]
        if interleaved:
            assert all(v < 0.95 * best for k, v in zip(lrpt.STAGGERS, scores) if k != s), scores
        else:                                             # (the last of the three frames no longer fits where a symbol was lost)
            assert best >= 2 * lrpt.MIN_SCORE and all(v < best for k, v in zip(lrpt.STAGGERS, scores) if k != s), scores


def test_end_to_end_in_numpy(walked):
    """recording -> restatement -> soft pairs -> the auto rule -> re-stagger -> the NumPy frame chain: the sent bodies of every
    whole frame past ACQ, with no marker bit in error (the 90 degree lock: the rails come out one symbol apart)"""
    rec, state, arr, _ = walked("72k_s1")
    nsym = len(arr["sym"])
    soft = lrpt.soft_np(arr["sym"])
    s = lrpt.stagger_pick(lrpt.stagger_scores_np(soft, nsym, template=lrpt.ASM_ENCODED_NRZM))
    assert s == -1
    soft = lrpt.restagger_np(soft, nsym, s)
    n = len(soft) // 2
    starts = lrpt.frame_starts(lrpt.asm_candidates_np(soft, n, template=lrpt.ASM_ENCODED_NRZM), n)
    frames, errs = [], []
    for p, h, _ in starts:
        bits = lrpt.viterbi_blocks(soft, n, int(p), int(h), lrpt.FRAME_BITS)
        body, asm_errors, _ = lrpt.finish_nrzm_np(bits, soft, n, int(p), int(h))
        frames.append(body)
        errs.append(asm_errors)
    expected = oq.expected_frames(rec, arr["aidx"])
    assert len(expected) >= 5
    info = np.zeros(len(frames), dtype=lrpt.INFO)
    info["asm_errors"] = errs
    oq.frames_found(frames, info, rec["bodies"], expected)
