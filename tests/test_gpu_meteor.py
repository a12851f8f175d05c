"""decode_meteorm2 on the device (dd_meteor_walk / _lim / _minsync / _maxcorr) against the reference's own getSyncs runs on the
recordings of tests/_meteor.py (tests/golden/meteor_*.npz, tools/gen_golden.py --meteor).

Exact: the B / A sample index of every symbol, the MINSYNC list and templates, the MAXSYNC buffers and argmaxes, getSyncs, useful.
Toleranced: the AGC'd symbols and the Costas phase / frequency.  The front end is not the reference's bit for
bit -- butter agrees with SciPy to 1e-9 relative, the mixer as DESIGN.md section 5 states -- and the symbol walk's float64 chain
carries that difference on, so the trace is compared with bounds (AGC_REL relative, PHASE_ABS / FREQ_ABS absolute) an order of
magnitude above what the fixtures show and far below any decision threshold."""
import os

import numpy as np
import pytest

import _meteor

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(_meteor.CASES)
AGC_REL = 1e-6
PHASE_ABS = 1e-6
FREQ_ABS = 1e-8


@pytest.fixture(scope="module")
def dd():
    from directdemod_amd import _hip
    _hip.require_gpu()
    from directdemod_amd import decode_meteorm2, source
    return decode_meteorm2, source


_runs = {}


def _run(dd, name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _runs:
        dmet, source = dd
        raw, off = _meteor.case(name)
        obj = dmet.decode_meteorm2(source.IQarray(raw, _meteor.FS), off, None, **kw)
        syncs = obj.getSyncs
        _runs[key] = (obj, syncs)
    return _runs[key]


def _load(name):
    return np.load(os.path.join(GOLDEN, "meteor_%s.npz" % name))


def _a_idx(g):
    if int(g["nsym"]) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate(([int(g["a_first"])], int(g["a_first"]) + np.cumsum(g["a_diff"].astype(np.int64))))


@pytest.mark.parametrize("name", NAMES)
def test_syncs_exact(dd, name):
    g = _load(name)
    obj, syncs = _run(dd, name)
    w = obj.walker()
    a = _a_idx(g)
    assert w.nsym == int(g["nsym"])
    assert np.array_equal(w.view("aidx").to_host(), a)
    assert np.array_equal(w.view("bidx").to_host(), a - g["ab_gap"].astype(np.int64))
    assert [m for m, _ in obj.minsyncs] == g["minsync"].tolist()
    tm = [t for _, t in obj.minsyncs][:len(g["template"])]
    assert tm == g["template"].tolist()
    iv = g["buf_intervals"]
    assert len(obj.buffers) == len(g["argmax"])
    for i, (ivs, start, _) in enumerate(obj.buffers):
        assert ivs == [(int(lo), int(c)) for j, lo, c in iv if j == i]
        assert start == int(g["buf_start"][i])
    assert obj.argmax == g["argmax"].tolist()
    assert all(type(s) is np.float64 for s in syncs)
    if int(g["one_maxsync"]):                                 # the reference raises ValueError here (np.min of an empty diff)
        assert len(obj.argmax) == 1 and syncs == [] and obj.useful == 0
    else:
        assert syncs == g["syncs"].tolist()
        assert obj.useful == int(g["useful"])


@pytest.mark.parametrize("name", NAMES)
def test_walk_trace_toleranced(dd, name):
    g = _load(name)
    obj, _ = _run(dd, name)
    w = obj.walker()
    sel = g["trace_sel"]
    if len(sel) == 0:
        return
    agc = w.view("agc").to_host()[sel]
    pf = w.view("pf").to_host()[sel]
    ref = g["trace_agc"]
    rel = np.abs(agc - ref) / np.maximum(np.abs(ref), 1.0)
    assert rel.max() < AGC_REL, rel.max()
    dph = np.abs(np.angle(np.exp(1j * (pf.real - g["trace_phase"]))))
    assert dph.max() < PHASE_ABS, dph.max()
    assert np.abs(pf.imag - g["trace_freq"]).max() < FREQ_ABS


def test_symbols_match_trace(dd):
    g = _load("a")
    obj, _ = _run(dd, "a")
    s = obj.getSymbols
    assert s.sampRate == 72000 and s.length == int(g["nsym"])
    sym = s.device_signal.to_host()
    n = min(4096, int(g["nsym"]))
    ph = np.r_[0.0, g["trace_phase"][:n - 1]]                  # costas.loop rotates by the phase before its own step
    want = g["trace_agc"][:n] * np.exp(-1j * ph)
    assert np.abs(sym[:n] - want).max() < 1e-3


def test_device_raw_matches_host_input(dd):
    obj, syncs = _run(dd, "b")
    obj2, syncs2 = _run(dd, "b", use_device_raw=False)
    assert syncs2 == syncs and obj2.minsyncs == obj.minsyncs and obj2.argmax == obj.argmax
    a, b = obj.walker(), obj2.walker()
    assert np.array_equal(a.view("aidx").to_host(), b.view("aidx").to_host())
    for name in ("bidx", "agc", "ph", "sym", "pf"):           # the same complex64 samples reach the mixer on both paths
        assert np.array_equal(a.view(name).to_host(), b.view(name).to_host()), name
    assert np.array_equal(a.lim_values.to_host(), b.lim_values.to_host())


def test_two_runs_bit_identical(dd):
    dmet, source = dd
    raw, off = _meteor.case("c")
    outs = []
    for _ in range(2):
        o = dmet.decode_meteorm2(source.IQarray(raw, _meteor.FS), off, None)
        s = o.getSyncs
        w = o.walker()
        outs.append((s, w.view("sym").to_host().tobytes(), w.lim_values.to_host().tobytes(), o.useful))
    assert outs[0] == outs[1]


def test_useful_zero_before_getsyncs_and_short_recording(dd):
    dmet, source = dd
    raw, _ = _meteor.case("a")
    o = dmet.decode_meteorm2(source.IQarray(raw[:20], _meteor.FS), 0, None)
    assert o.useful == 0
    assert o.getSyncs == [] and o.useful == 0
    assert o.getSymbols.length == 0
