"""The float64 restatement of the symbol walk (tests/_symbolwalk.py: walk_host, signal, CASES) against the reference's own loop
(tests/golden/symbolwalk_*.npz, tools/gen_golden.py --symbolwalk: decode_meteorm2's and decode_funcube's agc / Gardner / costas
loop over the same seeded samples), and the properties of its cases that tests/test_gpu_symbolwalk.py relies on.  No GPU.

Measured here (x86-64, glibc): walk_host(magnitude="pow") against the six fixtures gives equal B / A indices, 0 in agc.adjust's
output, and in four cases 0 in the corrected symbols, phase and freq; meteor_default 7.9e-17 in one symbol, funcube_locking
1.9e-16 (symbols), 1.1e-16 rad (phase), 8.8e-18 (freq): NumPy's complex exp against math.cos / math.sin, a last bit.  The cap below
is a condition, not a measurement: 1e-12, three orders above a one-ulp libm difference carried through loops whose gain is at most
1 / alpha (about 100), six below the 1e-6 of the end-to-end golden tests."""
import os

import numpy as np
import pytest

import _symbolwalk as sw
from directdemod_amd import bpsk, qpsk, symbolsync

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = [k for k, c in sw.CASES.items() if c.get("fixture")]
REL = ABS = 1e-12
WALKERS = {"meteor": qpsk.Walker, "funcube": bpsk.Walker}

_walks = {}


def _walk(name, magnitude):
    if (name, magnitude) not in _walks:
        policy, x, st = sw.case(name)
        _walks[name, magnitude] = sw.walk_host(x, 0, st, sw.params(policy), policy, magnitude)
    return _walks[name, magnitude]


@pytest.mark.parametrize("policy", sorted(sw.POLICIES))
def test_params_and_start_state_are_the_walkers(policy):
    W = WALKERS[policy]
    want = np.concatenate((W.leading_params(sw.FS), symbolsync.hyp_table()))
    assert np.array_equal(sw.params_array(sw.params(policy)), want)
    assert sw.POLICIES[policy]["symbol_rate"] == W.SYMBOL_RATE and sw.POLICIES[policy]["amean0"] == W.AMEAN0
    num, den = sw.POLICIES[policy]["rate"]
    assert num * sw.FS == den * W.SYMBOL_RATE
    assert tuple(symbolsync._STATE.names) == sw.FLOAT_FIELDS + sw.INT_FIELDS
    st = sw.start_state(policy)
    assert sw.state_dict(sw.state_struct(st, symbolsync._STATE)) == st


@pytest.mark.parametrize("name", FIXTURES)
def test_signal_reproduces_the_fixture_input(name):
    g = np.load(os.path.join(GOLDEN, "symbolwalk_%s.npz" % name))
    policy, x, st = sw.case(name)
    assert x.dtype == np.complex128 and len(x) == int(g["n"])
    assert sw.sha256(x) == str(g["sha256"])
    assert np.array_equal(x.real * 8, np.rint(x.real * 8)) and np.array_equal(x.imag * 8, np.rint(x.imag * 8))
    assert not np.signbit(x.real[x.real == 0]).any() and not np.signbit(x.imag[x.imag == 0]).any()
    assert (st["amean"], st["pmean"], st["lock"]) == (float(g["amean"]), float(g["pmean"]), int(g["lock"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_against_the_reference(name, capsys):
    """magnitude="pow", the reference's own: indices exact; values within 1e-12 of max(|ref|, 1), phase and freq within 1e-12.
    Measured: see the module's text (0 but for a last bit of exp in two cases)."""
    g = np.load(os.path.join(GOLDEN, "symbolwalk_%s.npz" % name))
    st, a, _ = _walk(name, "pow")
    assert st["ctr"] == len(g["aidx"]) == len(a["aidx"])
    assert np.array_equal(a["aidx"], g["aidx"])
    assert np.array_equal(a["bidx"], np.where(g["bidx"] < 0, 0, g["bidx"]))            # the state's bidx starts at 0
    d = {}
    for key in ("agc", "sym"):
        d[key] = float(np.max(np.abs(a[key] - g[key]) / np.maximum(np.abs(g[key]), 1.0), initial=0.0))
    d["phase"] = float(np.max(np.abs(a["pf"][:, 0] - g["phase"]), initial=0.0))
    d["freq"] = float(np.max(np.abs(a["pf"][:, 1] - g["freq"]), initial=0.0))
    with capsys.disabled():
        print("\n[symbolwalk host] %s: %d symbols, restatement - reference: %s" % (name, st["ctr"], d))
    assert d["agc"] <= REL and d["sym"] <= REL and d["phase"] <= ABS and d["freq"] <= ABS


def _all_inputs():
    """every (policy, x, base, start state) the GPU tests walk"""
    for name in sw.CASES:
        policy, x, st = sw.case(name)
        yield name, policy, x, st
    for policy in sorted(sw.POLICIES):
        for n, t0, _ in sw.length_runs(policy):
            yield "len %d timing %r" % (n, t0), policy, sw.signal(policy, **sw.LENGTH_SIGNAL[policy])[:n], sw.start_state(policy, timing=t0)


def test_sqrt_and_pow_give_the_same_indices_and_the_margin_holds():
    """on every input of the GPU tests: the device's sqrt and the reference's pow decide alike, and costas.mean stays 1e-9 clear of
    0.2 and 0.5, so a last bit of libm cannot move a lock event"""
    for name, policy, x, st in _all_inputs():
        p = sw.params(policy)
        s1, a1, c1 = sw.walk_host(x, 0, st, p, policy, "sqrt")
        s2, a2, c2 = sw.walk_host(x, 0, st, p, policy, "pow")
        assert np.array_equal(a1["aidx"], a2["aidx"]) and np.array_equal(a1["bidx"], a2["bidx"]), name
        assert s1["lock"] == s2["lock"] and {k: c1[k] for k in sw.COUNTERS} == {k: c2[k] for k in sw.COUNTERS}, name
        assert c1["pmean_margin"] > 1e-9 and c2["pmean_margin"] > 1e-9, name


@pytest.mark.parametrize("name", sorted(sw.CASES))
def test_case_reaches_its_branches(name):
    _, _, cnt = _walk(name, "sqrt")
    for key in sw.CASES[name]["reaches"]:
        assert cnt[key] > 0, (key, cnt)


def test_every_branch_counter_is_reached_by_some_case_of_each_policy():
    for policy in sorted(sw.POLICIES):
        total = dict.fromkeys(sw.COUNTERS, 0)
        for name, c in sw.CASES.items():
            if c["policy"] == policy:
                for k in sw.COUNTERS:
                    total[k] += _walk(name, "sqrt")[2][k]
        missing = [k for k, v in total.items() if v == 0]
        assert not missing, (policy, missing)


@pytest.mark.parametrize("policy", sorted(sw.POLICIES))
def test_length_runs_put_events_on_the_tile_edges(policy):
    """each (n, timing, (kind, sample)) of the GPU lengths test: the restatement has that event on that sample, and an A and a B
    event each fall on the last sample of a tile and on the first sample of the next"""
    p = sw.params(policy)
    xs = sw.signal(policy, **sw.LENGTH_SIGNAL[policy])
    seen = set()
    for n, t0, want in sw.length_runs(policy):
        if want is None:
            continue
        kind, j = want
        assert 0 <= j < n
        st = sw.start_state(policy, timing=t0)
        before = sw.walk_host(xs[:j], 0, st, p, policy)[2]
        upto = sw.walk_host(xs[:j + 1], 0, st, p, policy)[2]
        key = "a_events" if kind == "A" else "b_events"
        assert upto[key] == before[key] + 1, (n, t0, want)
        if (j + 1) % sw.TILE == 0:
            seen.add((kind, "last"))
        elif j and j % sw.TILE == 0:
            seen.add((kind, "first"))
    assert seen == {("A", "last"), ("A", "first"), ("B", "last"), ("B", "first")}


@pytest.mark.parametrize("name", sorted(sw.CASES))
def test_case_is_well_conditioned(name, monkeypatch):
    """The Costas loop's gain per step is alpha * |symbol| / 255 where the error is not clamped; above one, a last bit of the
    phasor grows without limit (a case with Funcube symbols of 2000 came apart by 1 rad on the device), and such a case says
    nothing about a kernel.  Every case here carries a cosine raised by one ulp at every third symbol to a phase difference below
    1e-12: measured 0 to 3.6e-15."""
    import math
    import types
    calls = [0]

    def cos(v):
        calls[0] += 1
        return math.nextafter(math.cos(v), 2.0) if calls[0] % 3 == 0 else math.cos(v)
    policy, x, st = sw.case(name)
    _, a, _ = _walk(name, "sqrt")
    monkeypatch.setattr(sw, "math", types.SimpleNamespace(cos=cos, sin=math.sin, sqrt=math.sqrt, fmod=math.fmod))
    _, b, _ = sw.walk_host(x, 0, st, sw.params(policy), policy, "sqrt")
    assert np.array_equal(a["aidx"], b["aidx"])
    d = np.abs(a["pf"][:, 0] - b["pf"][:, 0])
    assert float(np.max(np.minimum(d, np.abs(sw.TWO_PI - d)), initial=0.0)) < 1e-12
    assert calls[0] == len(a["aidx"])


def test_walk_host_chunks_carry_the_state():
    """the restatement itself: two calls with the state carried equal one"""
    policy, x, st = sw.case("meteor_default")
    p = sw.params(policy)
    s1, a1, _ = _walk("meteor_default", "sqrt")
    sa, aa, _ = sw.walk_host(x[:5000], 0, st, p, policy)
    sb, ab, _ = sw.walk_host(x[5000:], 5000, sa, p, policy)
    assert sb == s1
    for k in a1:
        assert np.array_equal(np.concatenate((aa[k], ab[k])), a1[k])
