"""decode_funcube on the device (dd_funcube_walk / _lim / _minsync / _maxcorr / _mix_ramp) against the reference's own getSyncs runs on
the recordings of tests/_funcube.py (tests/golden/funcube_*.npz, tools/gen_golden.py --funcube).

Exact: the B / A sample index of every symbol, the MINSYNC list, the MAXSYNC buffers and argmaxes, getSyncs and its element type,
useful, with corrfreq the per-chunk Doppler ramps, and the low-pass against scipy.signal.lfilter.  Toleranced:
the AGC'd symbols and the Costas phase / frequency at the fixtures' trace stride.  With the low-pass bit for bit lfilter's, what is
left is the ulp of the device's sin / cos (mixer, rounded to complex64; costas.loop) and sqrt against NumPy's ** 0.5.  Measured on
an MI355X over the seven fixtures: AGC'd symbols equal (0), phase within 4.44e-15 rad (case f), frequency within 9.85e-16 rad per
symbol (case f).  Each bound is ten times the largest figure; for the symbols, where that figure is 0, ten float64 ulps."""
import os

import numpy as np
import pytest

import _funcube

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(_funcube.CASES)
AGC_REL = 2.3e-15
PHASE_ABS = 5e-14
FREQ_ABS = 1e-14


@pytest.fixture(scope="module")
def dd():
    from directdemod_amd import _hip
    _hip.require_gpu()
    from directdemod_amd import bpsk, decode_funcube, source
    return decode_funcube, source, bpsk, _hip


_runs = {}


def _run(dd, name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _runs:
        dfc, source = dd[:2]
        raw, off, corr = _funcube.case(name)
        obj = dfc.decode_funcube(source.IQarray(raw, _funcube.FS), off, None, _funcube.CENTER, _funcube.CHANNEL, corr, **kw)
        syncs = obj.getSyncs
        _runs[key] = (obj, syncs)
    return _runs[key]


def _load(name):
    return np.load(os.path.join(GOLDEN, "funcube_%s.npz" % name))


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
    if int(g["corrfreq"]):                                    # before the walk: what the mixer was given
        assert len(obj.ramps) == len(g["chunk_offset"])
        for i, (shift, r, current) in enumerate(obj.ramps):
            assert shift == g["chunk_offset"][i]
            assert r.start == g["dopp_start"][i] and r.target == g["dopp_target"][i] and current == g["dopp_current"][i]
            if g["dopp_delta"][i] != 0.0:                     # (a ramp that starts on its target is clipped from its second sample on)
                assert r.delta == g["dopp_delta"][i]
    else:
        assert obj.ramps == []
    assert w.nsym == int(g["nsym"])
    assert np.array_equal(w.view("aidx").to_host(), a)
    assert np.array_equal(w.view("bidx").to_host(), a - g["ab_gap"].astype(np.int64))
    assert obj.minsyncs == g["minsync"].tolist()
    iv = g["buf_intervals"]
    assert len(obj.buffers) == len(g["argmax"])
    for i, (ivs, start) in enumerate(obj.buffers):
        assert ivs == [(int(lo), int(c)) for j, lo, c in iv if j == i]
        assert start == int(g["buf_start"][i])
    assert obj.argmax == g["argmax"].tolist()
    assert all(type(s) is np.int64 for s in syncs)
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
    assert len(sel) > 0 and w.nsym == int(g["nsym"])
    agc = w.view("agc").to_host()[sel]
    pf = w.view("pf").to_host()[sel]
    ref = g["trace_agc"]
    rel = np.abs(agc - ref) / np.maximum(np.abs(ref), 1.0)
    dph = np.abs(np.angle(np.exp(1j * (pf.real - g["trace_phase"]))))
    dfr = np.abs(pf.imag - g["trace_freq"])
    print("funcube %s: agc rel %.3g, phase %.3g rad, freq %.3g rad/symbol" % (name, rel.max(), dph.max(), dfr.max()))
    assert rel.max() < AGC_REL, rel.max()
    assert dph.max() < PHASE_ABS, dph.max()
    assert dfr.max() < FREQ_ABS, dfr.max()


def test_symbols_match_trace(dd):
    g = _load("a")
    obj, _ = _run(dd, "a")
    s = obj.getSymbols
    assert s.sampRate == 12000 and s.length == int(g["nsym"])
    sym = s.device_signal.to_host()
    n = min(2048, int(g["nsym"]))
    assert np.array_equal(g["trace_sel"][:n], np.arange(n))
    ph = np.r_[0.0, g["trace_phase"][:n - 1]]                  # costas.loop rotates by the phase before its own step
    want = g["trace_agc"][:n] * np.exp(-1j * ph)
    assert np.abs(sym[:n] - want).max() < 1e-9                 # |sym| < 4000: the host's exp against the device's sincos, an ulp each


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
    dfc, source = dd[:2]
    raw, off, corr = _funcube.case("c")
    outs = []
    for _ in range(2):
        o = dfc.decode_funcube(source.IQarray(raw, _funcube.FS), off, None, _funcube.CENTER, _funcube.CHANNEL, corr)
        s = o.getSyncs
        w = o.walker()
        outs.append((s, w.view("sym").to_host().tobytes(), w.lim_values.to_host().tobytes(), o.useful))
    assert outs[0] == outs[1]


def test_useful_zero_before_getsyncs_and_short_recording(dd):
    dfc, source = dd[:2]
    raw, _, _ = _funcube.case("a")
    o = dfc.decode_funcube(source.IQarray(raw[:20], _funcube.FS), 0, None, _funcube.CENTER, _funcube.CHANNEL)
    assert o.useful == 0
    assert o.getSyncs == [] and o.useful == 0
    assert o.getSymbols.length == 0


def test_ramp_mixer_with_a_constant_frequency_equals_the_plain_mixer(dd):
    """the ramp form of the float64 mixer: a ramp that sits on its target gives dd_meteor_mix's bits, a moving one follows
    np.arange's fill and the clip (checked against NumPy's exp to the precision of complex64)"""
    _, _, bpsk, _hip = dd
    from directdemod_amd import frequency_shift as fsh
    raw, _, _ = _funcube.case("d")
    n = 100001
    d = _hip.DevArray.from_host(raw[:n].copy().view(_hip.IQ8).reshape(-1))
    x = (raw[:n, 0] + 1j * raw[:n, 1]).astype(np.complex64) - np.complex64(127.5 + 127.5j)
    plain = bpsk.mix(d, _funcube.FS, 25336.9565).to_host()
    same = bpsk.mix_ramp(d, _funcube.FS, fsh.ramp(25336.9565, -1e-4, 25336.9565, n)).to_host()
    assert np.array_equal(plain, same)
    for start, delta, target in ((25336.9565, -1e-4, 25330.0), (-20000.0, 1e-4, -19995.0)):
        f = start + np.arange(n) * delta
        f = np.minimum(f, target) if target > start else np.maximum(f, target)
        want = x.astype(np.complex128) * np.exp(-1.0j * 2.0 * np.pi * f * np.arange(n) / _funcube.FS)
        got = bpsk.mix_ramp(d, _funcube.FS, fsh.ramp(start, delta, target, n)).to_host()
        assert np.abs(got - want).max() < 2e-5                 # |x| < 181: half a float32 ulp of 128 is 7.6e-6 per component
        host = bpsk.mix_ramp(_hip.DevArray.from_host(x), _funcube.FS, fsh.ramp(start, delta, target, n)).to_host()
        assert np.array_equal(host, got)


def _maxcorr(dd, buf, ivs, rep):
    _, _, bpsk, _hip = dd
    lv = _hip.DevArray.from_host(np.asarray(buf, dtype=np.int8))
    return bpsk.maxsync_argmax(lv, [(ivs, ivs[0][0])], rep)[0]


@pytest.mark.parametrize("where", ["first", "last", "middle"])
def test_maxcorr_alone_matches_numpy(dd, where):
    """dd_funcube_maxcorr on synthetic int8 buffers: the full 56298-sample template on a buffer whose length (57001) is no multiple
    of the 1024 lags a pass of the workgroup takes, the maximum planted at the first lag, at the last lag, or inside; a buffer
    given as two intervals; and a short template against np.correlate itself"""
    bpsk = dd[2]
    rng = np.random.default_rng(7)
    t = bpsk.template_bits()
    tm = np.repeat(t, bpsk.REP)
    L, left = 57001, bpsk.TLEN // 2
    buf = rng.integers(-3, 4, L)
    if where == "first":
        buf[:bpsk.TLEN - left] = np.where(tm[left:] > 0, 127, -128)
    elif where == "last":
        buf[L - 1 - left:] = np.where(tm[:left + 1] > 0, 127, -128)
    else:
        buf = rng.integers(-128, 128, L)
    ref = np.abs(bpsk.correlate_same_blocks(buf, t))           # equal to np.correlate(..., 'same') (tests/test_funcube_host.py)
    want = int(np.argmax(ref))
    if where != "middle":
        assert want == (0 if where == "first" else L - 1)
    arg, mx = _maxcorr(dd, buf, [(0, L)], bpsk.REP)
    assert (int(arg), int(mx)) == (want, int(ref[want]))
    # the same buffer as two intervals of a longer lim array
    n0 = 30011
    wide = np.concatenate((buf[:n0], rng.integers(-128, 128, 77), buf[n0:]))
    arg, mx = _maxcorr(dd, wide, [(0, n0), (n0 + 77, L - n0)], bpsk.REP)
    assert (int(arg), int(mx)) == (want, int(ref[want]))
    # a short template (5 samples per bit) against np.correlate, ties included
    for small in (rng.integers(-128, 128, 1501), np.zeros(1501, dtype=np.int64), np.full(165, 127)):
        r = np.abs(np.correlate(list(small), np.repeat(t, 5), mode="same"))
        arg, mx = _maxcorr(dd, small, [(0, len(small))], 5)
        assert (int(arg), int(mx)) == (int(np.argmax(r)), int(r.max()))


def test_lowpass_7khz_is_scipy_lfilter_bit_for_bit(dd):
    """butter(2048000, 7000) -- decode_funcube's default, the poles closer to the unit circle than any other shape in the suite --
    alone on case a's samples, in two chunks with the state carried.  bpsk.Lowpass runs lfilter's recurrence in lfilter's operation
    order, so equality is exact.  The package's block-parallel IIR (filters.butter -> dd_iir_c64) on the same samples is measured
    beside it and printed: 5.6e-6 relative on an MI355X, against 1e-9 at 20 kHz -- the reason decode_funcube
    does not use it."""
    ss = pytest.importorskip("scipy.signal")
    from directdemod_amd import comm, filters
    _, _, bpsk, _hip = dd
    raw, _, _ = _funcube.case("a")
    x = ((raw[:, 0] + 1j * raw[:, 1]).astype(np.complex64) - np.complex64(127.5 + 127.5j))
    lp = bpsk.Lowpass(_funcube.FS, 7000)
    f = filters.butter(_funcube.FS, 7000)
    n = 1000003
    got, blk = [], []
    for part in (x[:n], x[n:]):
        d = _hip.DevArray.from_host(part)
        got.append(lp.apply(d).to_host())
        sig = comm.commSignal(_funcube.FS, d)
        sig.filter(f)
        blk.append(sig.device_signal.to_host())
    got, blk = np.concatenate(got), np.concatenate(blk)
    ref, zf = ss.lfilter(lp.b, lp.a, x.astype(np.complex128), zi=ss.lfilter_zi(lp.b, lp.a).astype(np.complex128))
    print("butter 7 kHz at 2.048 MS/s against scipy.signal.lfilter: serial %.3g, block-parallel dd_iir_c64 %.3g (relative)" %
          (np.abs(got - ref).max() / np.abs(ref).max(), np.abs(blk - ref).max() / np.abs(ref).max()))
    assert got.dtype == np.complex128 and np.array_equal(got, ref)
    st = lp.state.to_host()
    assert np.array_equal(st[:6], zf.real) and np.array_equal(st[6:], zf.imag)
