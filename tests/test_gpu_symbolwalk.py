"""The symbol walk (dd_meteor_walk / dd_funcube_walk: dd_sym_walk in dd_symbol_walk.h) and the kernels beside it (dd_*_lim, dd_*_minsync,
dd_meteor_maxcorr, dd_funcube_maxcorr) alone, at their edges, against plain restatements fed the same numbers.

The walk is compared with tests/_symbolwalk.py's walk_host -- a sample-by-sample float64 loop that tests/test_symbolwalk_host.py ties
to the reference's own loop (tests/golden/symbolwalk_*.npz) -- on the same complex128 samples.  The timing chain is + - * / and sqrt,
each rounded on its own, so the symbol count, the B / A indices, agc.adjust's output and the carried timing, B, C, dc, mean, bidx,
overflow are compared bit for bit, and so is the lock.  Only the Costas chain goes through sincos, where the device's and the host's
libm may differ in a last bit: ph, sym, pf and the carried freq, phase, pmean are compared to bounds of 64 times the largest
device-minus-restatement difference measured on an MI355X over all walk inputs of this file:

    sym    relative to max(|ref|, 1)   measured 1.01e-15   bound 6.5e-14
    ph     absolute                    measured 9.56e-16   bound 6.1e-14
    phase  absolute on the circle      measured 8.89e-16   bound 5.7e-14 rad
    freq   absolute                    measured 2.50e-16   bound 1.6e-14 rad per symbol

(pmean, a mean of |error| = |f(sym)| / 255, takes sym's bound.)  Chunked calls against one call are the same device code and are
compared bit for bit in every array.  lim, MINSYNC and the correlations are integer results and exact.

These figures hold where the Costas loop contracts (gain per step alpha * |symbol| / 255 below one where the error is not clamped);
tests/test_symbolwalk_host.py keeps every case there.  A case outside it came apart by 0.87 rad with the timing chain still equal
bit for bit, on the device as under a one-ulp change of one cosine on the host: it measured the loop, not the kernel."""
import ctypes as C

import numpy as np
import pytest

import _symbolwalk as sw

pytestmark = pytest.mark.gpu

SYM_MEASURED, PH_MEASURED, PHASE_MEASURED, FREQ_MEASURED = 1.01e-15, 9.56e-16, 8.89e-16, 2.50e-16
SYM_REL = 64 * SYM_MEASURED
PH_ABS = 64 * PH_MEASURED
PHASE_ABS = 64 * PHASE_MEASURED
FREQ_ABS = 64 * FREQ_MEASURED
assert max(SYM_REL, PH_ABS, PHASE_ABS, FREQ_ABS) <= 1e-9

SPARE = 16                                     # entries past the capacity, which must keep the sentinel
SENT_I = np.int64(-0x5A5A5A5A5A5A5A5B)
SENT_C = np.complex128(complex(-7.25e300, 3.5e-300))
SENT_8 = np.int8(-77)
ARRAYS = ("bidx", "aidx", "agc", "ph", "sym", "pf")
POLICIES = sorted(sw.POLICIES)
FIXTURES = [k for k, c in sw.CASES.items() if c.get("fixture")]
WALK = {"meteor": "dd_meteor_walk", "funcube": "dd_funcube_walk"}
LIM = {"meteor": ("dd_meteor_lim", np.int16), "funcube": ("dd_funcube_lim", np.int8)}
MINSYNC = {"meteor": ("dd_meteor_minsync", 3), "funcube": ("dd_funcube_minsync", 2)}
MEASURED = dict(sym=0.0, ph=0.0, phase=0.0, freq=0.0)


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def _bits(a):
    """an array's bytes as int64 words"""
    return np.ascontiguousarray(a).reshape(-1).view(np.int64)


def _state_type():
    from directdemod_amd.symbolsync import _STATE
    return _STATE


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ------------------------------------------------------------------------------------------------------------------ the walk
def dev_walk(hip, policy, x, st, cuts=(), cap=None, base=0):
    """the policy's walk entry point over x from the state st (a dict), cut into calls of the lengths `cuts` and a last call with
    the rest, `base` running on -> (the state record after, the six arrays whole: cap + SPARE entries, sentinel where not written)"""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    n = len(x)
    cap = n if cap is None else cap
    dev = {k: hip.DevArray.from_host(np.full(cap + SPARE, SENT_I if k in ("bidx", "aidx") else SENT_C)) for k in ARRAYS}
    dx = hip.DevArray.from_host(x) if n else hip.DevArray(1, np.complex128)
    dstate = hip.DevArray.from_host(sw.state_struct(st, _state_type()).view(np.uint8))
    prm = sw.params_array(sw.params(policy))
    fn = getattr(hip.lib(), WALK[policy])
    at = 0
    assert sum(cuts) <= n
    for m in list(cuts) + [n - sum(cuts)]:
        hip.check(fn(dx.ptr + 16 * at, m, base + at, dstate.ptr, _pd(prm), cap, *(dev[k].ptr for k in ARRAYS), None), WALK[policy])
        at += m
    hip.sync()
    return dstate.to_host().view(_state_type())[0], {k: dev[k].to_host() for k in ARRAYS}


def _circle(d):
    d = np.abs(d)
    return np.minimum(d, np.abs(sw.TWO_PI - d))


def _costas_differences(got, ref, state, ref_state):
    """the four Costas figures of device arrays `got` ([0, m)) against ref, and of the carried freq / phase / pmean"""
    m = len(ref["sym"])
    gpf, rpf = got["pf"][:m].view(np.float64).reshape(-1, 2), ref["pf"]
    d = dict(sym=float(np.max(np.abs(got["sym"][:m] - ref["sym"]) / np.maximum(np.abs(ref["sym"]), 1.0), initial=0.0)),
             ph=float(np.max(np.abs(got["ph"][:m] - ref["ph"]), initial=0.0)),
             phase=float(np.max(_circle(gpf[:, 0] - rpf[:, 0]), initial=0.0)),
             freq=float(np.max(np.abs(gpf[:, 1] - rpf[:, 1]), initial=0.0)))
    if state is not None:
        d["phase"] = max(d["phase"], float(_circle(np.float64(state["phase"] - ref_state["phase"]))))
        d["freq"] = max(d["freq"], abs(float(state["freq"]) - ref_state["freq"]))
        d["sym"] = max(d["sym"], abs(float(state["pmean"]) - ref_state["pmean"]))
    return d


def _report(capsys, what, d):
    with capsys.disabled():
        print("\n[symbolwalk] %s: device - restatement %s" % (what, {k: float("%.3g" % v) for k, v in d.items()}))


def _assert_costas(d, what, capsys=None):
    """the four figures against their bounds; they go into MEASURED (the largest of the session) and, with capsys, to the output"""
    for k in MEASURED:
        MEASURED[k] = max(MEASURED[k], float(d[k]))
    if capsys is not None:
        _report(capsys, what, d)
    assert d["sym"] <= SYM_REL and d["ph"] <= PH_ABS and d["phase"] <= PHASE_ABS and d["freq"] <= FREQ_ABS, (what, d)


def check_walk(policy, x, st, state, got, capsys, what, base=0, cap=None):
    """device result (state record, whole arrays) against walk_host over the same samples -> the restatement's counters"""
    cap = len(x) if cap is None else cap
    hs, ref, cnt = sw.walk_host(x, base, st, sw.params(policy), policy, "sqrt")
    nsym = hs["ctr"] - st["ctr"]
    assert st["ctr"] == 0
    assert int(state["ctr"]) == hs["ctr"], what
    m = min(nsym, cap)
    for k in ("bidx", "aidx"):
        assert np.array_equal(got[k][:m], ref[k][:m]), (what, k)
    assert np.array_equal(_bits(got["agc"][:m]), _bits(ref["agc"][:m])), (what, "agc.adjust's output differs in its bits")
    for k in ARRAYS:
        sent = SENT_I if k in ("bidx", "aidx") else SENT_C
        assert np.array_equal(_bits(got[k][m:]), _bits(np.full(len(got[k]) - m, sent))), (what, k, "written past min(ctr, cap)")
    for f in sw.TIMING_FIELDS:
        if f == "overflow":
            assert int(state[f]) == (1 if nsym > cap else st["overflow"]), (what, f)
        elif f == "bidx":
            assert int(state[f]) == hs[f], (what, f)
        else:
            assert np.float64(state[f]).view(np.int64) == np.float64(hs[f]).view(np.int64), (what, f, float(state[f]), hs[f])
    assert int(state["lock"]) == hs["lock"], what
    for f in ("alpha", "beta"):
        assert float(state[f]) == hs[f], (what, f)
    d = _costas_differences({k: got[k][:m] for k in got}, {k: ref[k][:m] for k in ref}, state, hs)
    _assert_costas(d, what, capsys)
    return cnt


@pytest.mark.parametrize("name", sorted(sw.CASES))
def test_walk_against_the_restatement(hip, name, capsys):
    """default and started states, a tile full of symbols (sbuf at capacity) and a tile with none: everything the timing chain
    yields bit for bit, the Costas chain within its bounds; the restatement's counters say that the case met its branch"""
    policy, x, st = sw.case(name)
    state, got = dev_walk(hip, policy, x, st)
    cnt = check_walk(policy, x, st, state, got, capsys, name)
    for key in sw.CASES[name]["reaches"]:
        assert cnt[key] > 0, (key, cnt)


@pytest.mark.parametrize("name", FIXTURES)
def test_walk_against_the_reference(hip, name, golden_dir, capsys):
    """the same inputs against the reference's own loop: indices exact, values within the Costas bounds (agc.adjust's magnitude is
    pow there and sqrt here, which the restatement's two modes carry to the same indices)"""
    import os
    g = np.load(os.path.join(golden_dir, "symbolwalk_%s.npz" % name))
    policy, x, st = sw.case(name)
    assert sw.sha256(x) == str(g["sha256"])
    state, got = dev_walk(hip, policy, x, st)
    m = len(g["aidx"])
    assert int(state["ctr"]) == m and int(state["overflow"]) == 0
    assert np.array_equal(got["aidx"][:m], g["aidx"])
    assert np.array_equal(got["bidx"][:m], np.where(g["bidx"] < 0, 0, g["bidx"]))
    ref = dict(sym=g["sym"], ph=got["ph"][:m], pf=np.stack((g["phase"], g["freq"]), axis=1))      # (the reference's phasor is not recorded)
    d = _costas_differences(got, ref, None, None)
    d["sym"] = max(d["sym"], float(np.max(np.abs(got["agc"][:m] - g["agc"]) / np.maximum(np.abs(g["agc"]), 1.0), initial=0.0)))
    _assert_costas(d, name + " (reference)", capsys)


@pytest.mark.parametrize("policy", POLICIES)
def test_walker_class_starts_where_the_reference_does(hip, policy):
    """symbolsync.Walker's own start state and parameters are _symbolwalk.start_state's and params', and a walk through the class
    gives the restatement's indices and agc.adjust outputs"""
    from directdemod_amd import bpsk, qpsk
    _, x, st = sw.case(policy + "_default")
    x = x[:4096]
    w = {"meteor": qpsk.Walker, "funcube": bpsk.Walker}[policy](sw.FS, len(x))
    assert w.state.to_host().tobytes() == sw.state_struct(st, _state_type()).tobytes()
    assert np.array_equal(w.params, sw.params_array(sw.params(policy)))
    w.walk(hip.DevArray.from_host(x))
    hs, ref, _ = sw.walk_host(x, 0, st, sw.params(policy), policy, "sqrt")
    assert w.nsym == hs["ctr"] > 0
    for k in ("bidx", "aidx", "agc"):
        assert np.array_equal(_bits(w.view(k).to_host()), _bits(ref[k])), k


@pytest.mark.parametrize("policy", POLICIES)
def test_walk_lengths(hip, policy, capsys):
    """n around the 64 staging lanes and around one, two and three tiles, from timing 0 and from start timings that put an A event
    and a B event on the last sample of a tile and on the first sample of the next (tests/test_symbolwalk_host.py asserts where
    they fall from the restatement's indices); n = 0 leaves the state's bytes alone"""
    xs = sw.signal(policy, **sw.LENGTH_SIGNAL[policy])
    for n, t0, want in sw.length_runs(policy):
        st = sw.start_state(policy, timing=t0)
        state, got = dev_walk(hip, policy, xs[:n], st)
        check_walk(policy, xs[:n], st, state, got, None, "%s n %d timing %r %r" % (policy, n, t0, want))
        if want is not None and want[0] == "A":
            assert want[1] in got["aidx"][:int(state["ctr"])]
    _report(capsys, "%s lengths: largest of the session so far" % policy, MEASURED)
    st = sw.start_state(policy, timing=12.75, b_im=-3.5, phase=1.25, ctr=0)
    state, got = dev_walk(hip, policy, xs[:0], st, cap=4)
    assert state.tobytes() == sw.state_struct(st, _state_type()).tobytes()
    for k in ARRAYS:
        assert np.array_equal(_bits(got[k]), _bits(np.full(4 + SPARE, SENT_I if k in ("bidx", "aidx") else SENT_C))), k


def _primes(count):
    out, v = [], 2
    while len(out) < count:
        if all(v % p for p in out):
            out.append(v)
        v += 1
    return out


CUTTINGS = {
    "edges": lambda n: (n, [1, 1023, 1, 1024, 2049]),
    "primes": lambda n: (sum(_primes(64)), _primes(64)[:-1]),          # 64 calls: the last takes the 64th prime
    "ones": lambda n: (2000, [1] * 1999),
}


@pytest.mark.parametrize("cutting", sorted(CUTTINGS))
@pytest.mark.parametrize("name", ["meteor_default", "meteor_started", "funcube_default", "funcube_started"])
def test_walk_chunked_is_bit_identical(hip, name, cutting):
    """the same input in one call and cut into calls, `base` running on from a non-zero start: every array and the final state bit
    for bit, the Costas chain's included (the same device code); the B / A indices carry the base"""
    policy, x, st = sw.case(name)
    n, cuts = CUTTINGS[cutting](len(x))
    x = x[:n]
    base = 1000003
    s1, one = dev_walk(hip, policy, x, st, base=base)
    s2, cut = dev_walk(hip, policy, x, st, cuts=cuts, base=base)
    assert s1.tobytes() == s2.tobytes()
    for k in ARRAYS:
        assert np.array_equal(_bits(one[k]), _bits(cut[k])), k
    m = int(s1["ctr"])
    assert m > 0 and one["aidx"][0] >= base and np.all(np.diff(one["aidx"][:m]) > 0)
    _, ref, _ = sw.walk_host(x, base, st, sw.params(policy), policy, "sqrt")
    assert np.array_equal(one["aidx"][:m], ref["aidx"]) and np.array_equal(one["bidx"][:m], ref["bidx"])


@pytest.mark.parametrize("policy", POLICIES)
def test_walk_capacity(hip, policy):
    """cap = nsym, nsym - 1, 1, 0: overflow exactly when cap < nsym, ctr the true count, entries [0, cap) right, and every entry
    from cap on untouched in all six arrays (check_walk looks at each)"""
    _, x, st = sw.case(policy + "_default")
    x = x[:6000]
    hs, _, _ = sw.walk_host(x, 0, st, sw.params(policy), policy, "sqrt")
    nsym = hs["ctr"]
    assert nsym > 2
    for cap in (nsym, nsym - 1, 1, 0):
        state, got = dev_walk(hip, policy, x, st, cap=cap)
        assert int(state["ctr"]) == nsym and int(state["overflow"]) == (1 if cap < nsym else 0), cap
        check_walk(policy, x, st, state, got, None, "%s cap %d of %d" % (policy, cap, nsym), cap=cap)


@pytest.mark.parametrize("policy", POLICIES)
def test_walk_refuses_bad_arguments(hip, policy):
    fn = getattr(hip.lib(), WALK[policy])
    prm = sw.params_array(sw.params(policy))
    st0 = sw.state_struct(sw.start_state(policy), _state_type()).view(np.uint8)
    dstate = hip.DevArray.from_host(st0)
    dx = hip.DevArray.from_host(np.zeros(8, dtype=np.complex128))
    bufs = [hip.DevArray(8 + SPARE, np.int64 if k in ("bidx", "aidx") else np.complex128) for k in ARRAYS]
    ptrs = [b.ptr for b in bufs]
    good = dict(x=dx.ptr, n=8, base=0, state=dstate.ptr, prm=_pd(prm), cap=8)

    def call(ptrs=ptrs, **kw):
        a = dict(good, **kw)
        return fn(a["x"], a["n"], a["base"], a["state"], a["prm"], a["cap"], *ptrs, None)
    for bad in (dict(n=-1), dict(base=-1), dict(cap=-1), dict(state=None), dict(prm=None), dict(x=None),
                dict(n=0, state=None), dict(n=0, prm=None), dict(n=0, cap=-1)):
        assert call(**bad) == hip.DD_ERR_INVALID, bad
    for i in range(len(ptrs)):
        assert call(ptrs=ptrs[:i] + [None] + ptrs[i + 1:]) == hip.DD_ERR_INVALID, ARRAYS[i]
    assert call(n=0, x=None, ptrs=[None] * 6) == hip.DD_OK            # nothing to read or write
    hip.sync()
    assert dstate.to_host().tobytes() == st0.tobytes()                  # no refused call touched the state


# ------------------------------------------------------------------------------------------------------------------ lim
def lim_value(v):
    """lim of the project: NaN gives 0 (the reference's int() raises)"""
    from directdemod_amd.symbolsync import lim
    return 0 if v != v else lim(v)


def lim_expected(policy, x, base, aidx, ph):
    """sample base + j takes the phasor of the last symbol whose A sample lies before it, (1, -0) before any; NumPy's complex
    product component by component; lim of half the real (and imaginary) part"""
    out = []
    for j, v in enumerate(x):
        c = sum(1 for a in aidx if a < base + j)
        o = complex(1.0, -0.0) if c == 0 else ph[c - 1]
        re = np.float64(v.real) * o.real - np.float64(v.imag) * o.imag
        im = np.float64(v.real) * o.imag + np.float64(v.imag) * o.real
        out.append((lim_value(re / 2.0), lim_value(im / 2.0)))
    e = np.array(out, dtype=np.int8).reshape(-1, 2)
    return e.copy().view(np.int16).reshape(-1) if policy == "meteor" else e[:, 0].copy()


def dev_lim(hip, policy, x, base, aidx, ph, out_len, rc_only=False):
    entry, dt = LIM[policy]
    sent = np.full(out_len + SPARE, SENT_8, dtype=np.int8) if dt == np.int8 else np.full(2 * (out_len + SPARE), SENT_8, dtype=np.int8).view(np.int16)
    out = hip.DevArray.from_host(sent)
    dx = hip.DevArray.from_host(np.ascontiguousarray(x, dtype=np.complex128))
    da = hip.DevArray.from_host(np.asarray(aidx, dtype=np.int64)) if len(aidx) else None
    dp = hip.DevArray.from_host(np.asarray(ph, dtype=np.complex128)) if len(aidx) else None
    rc = getattr(hip.lib(), entry)(dx.ptr, len(x), base, da.ptr if da else None, len(aidx), dp.ptr if dp else None, out.ptr, out_len, None)
    hip.sync()
    if rc_only:
        return rc, out.to_host(), sent
    hip.check(rc, entry)
    return out.to_host(), sent


SPECIAL = [0.0, -0.0, 0.5, -0.5, 1.9, -1.9, 2.0, -2.0, 253.9, -253.9, 254.0, -254.0, 256.0, -256.0, 257.0, -257.0, 1e9, -1e9, float("nan")]


@pytest.mark.parametrize("policy", POLICIES)
def test_lim_values_without_symbols(hip, policy):
    """nsym = 0: the phasor is (1, -0), the output lim(v / 2) of the real (and imaginary) part -- the special values on either
    side of every rule of lim against symbolsync.lim, NaN as 0, and a random tail to a length that is no multiple of 256"""
    rng = np.random.Generator(np.random.PCG64(21))
    tail = rng.integers(-4200, 4200, size=(600 - 2 * len(SPECIAL) + 3, 2)) / 8.0
    x = np.concatenate((np.array(SPECIAL) + 1j * 3.0, 3.0 + 1j * np.array(SPECIAL), tail[:, 0] + 1j * tail[:, 1]))
    assert len(x) % 256 and len(x) > 512
    got, _ = dev_lim(hip, policy, x, 0, [], [], len(x))
    assert np.array_equal(got, np.concatenate((lim_expected(policy, x, 0, [], []), got[len(x):])))
    # said plainly: lim of half of each part (a NaN in one part reaches the other through the product with -0)
    re = np.array([lim_value(v.real / 2.0) for v in x], dtype=np.int8)
    im = np.array([lim_value(v.imag / 2.0) for v in x], dtype=np.int8)
    assert list(re[:8]) == [0, 0, 1, -1, 1, -1, 1, -1] and list(re[8:19]) == [126, -126, 127, -127, 127, -128, 127, -128, 127, -128, 0]
    ok = ~np.isnan(x.real) & ~np.isnan(x.imag)
    if policy == "meteor":
        pairs = got[:len(x)].view(np.int8).reshape(-1, 2)
        assert np.array_equal(pairs[ok, 0], re[ok]) and np.array_equal(pairs[ok, 1], im[ok])
        assert np.array_equal(pairs[~ok], np.zeros((2, 2), dtype=np.int8))
    else:
        assert np.array_equal(got[:len(x)][ok], re[ok]) and got[18] == 0


@pytest.mark.parametrize("policy", POLICIES)
def test_lim_takes_the_phasor_of_the_last_symbol_before_the_sample(hip, policy):
    """a hand-made aidx / ph: the sample at aidx[k] still takes ph[k - 1] (the strict <), the next one ph[k]; samples up to
    aidx[0] take (1, -0); a chunk at base != 0 writes out[base : base + n] alone; base + n > out_len is refused"""
    rng = np.random.Generator(np.random.PCG64(22))
    aidx = np.array([5, 6, 300, 301, 555, 700, 701], dtype=np.int64)
    ph = np.array([1j, -1.0, -1j, 0.5 + 0.5j, 2.0, -0.25j, 1.0], dtype=np.complex128)
    n = 777
    v = rng.integers(-800, 800, size=(n, 2)) / 8.0
    x = v[:, 0] + 1j * v[:, 1]
    want = lim_expected(policy, x, 0, aidx, ph)
    got, _ = dev_lim(hip, policy, x, 0, aidx, ph, n)
    assert np.array_equal(got[:n], want)

    def one(s, o):
        return lim_expected(policy, x[s:s + 1], 0, [], []) if o is None else lim_expected(policy, x[s:s + 1], s, [s - 1], [o])
    for s in range(0, 6):
        assert got[s] == one(s, None)[0]                       # up to and including aidx[0]: no symbol before
    for k in range(1, len(aidx)):
        assert got[aidx[k]] == one(int(aidx[k]), ph[k - 1])[0]
    for k in range(len(aidx)):
        assert got[aidx[k] + 1] == one(int(aidx[k]) + 1, ph[k])[0]
    assert not np.array_equal(want, lim_expected(policy, x, 0, aidx + 1, ph))       # the input tells < from <=
    # a chunk in the middle of a longer recording, the symbols before it included
    base, m, total = 290, 300, 900
    got, sent = dev_lim(hip, policy, x[base:base + m], base, aidx, ph, total)
    assert np.array_equal(got[base:base + m], want[base:base + m])
    assert np.array_equal(got[:base], sent[:base]) and np.array_equal(got[base + m:], sent[base + m:])
    rc, got, sent = dev_lim(hip, policy, x[:m], total - m + 1, aidx, ph, total, rc_only=True)
    assert rc == hip.DD_ERR_INVALID and np.array_equal(got, sent)
    rc, got, sent = dev_lim(hip, policy, x[:m], total - m, aidx, ph, total, rc_only=True)
    assert rc == hip.DD_OK and np.array_equal(got[total:], sent[total:])


# ------------------------------------------------------------------------------------------------------------------ MINSYNC
def minsync_patterns(policy):
    """the bit patterns a window is scored against, per symbol: Meteor (re, im) pairs for sync72khz and (re, im) pairs that give
    sync72khz1 read as (im, re); Funcube sync12khz"""
    from directdemod_amd import bpsk, qpsk
    if policy == "meteor":
        s72, s1, _ = qpsk.sync_patterns()
        return [s72.reshape(-1, 2), s1.reshape(-1, 2)[:, ::-1]]
    return [np.stack((bpsk.sync12khz(), bpsk.sync12khz()), axis=1)]


def minsync_symbols(policy, nsym, plants, seed):
    """random symbols with patterns planted: plants = [(first symbol, pattern number, inverted, number of flipped bits)]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    bits = rng.integers(0, 2, size=(nsym, 2))
    width = 2 if policy == "meteor" else 1
    for at, which, inverted, flips in plants:
        p = minsync_patterns(policy)[which].copy()
        if inverted:
            p = 1 - p
        flat = p[:, :width].reshape(-1)
        flat[rng.permutation(len(flat))[:flips]] ^= 1
        p[:, :width] = flat.reshape(-1, width)
        bits[at:at + len(p)] = p
    mag = rng.integers(1, 2000, size=(nsym, 2)) / 8.0
    return np.where(bits == 1, mag, -mag)[:, 0] + 1j * np.where(bits == 1, mag, -mag)[:, 1]


def minsync_expected(policy, sym):
    """(the symbols' bits as the device packs them, the rows of the windows that fire) from limBin, qpsk._scores / _fires, and a
    NumPy count for Funcube"""
    from directdemod_amd import bpsk, qpsk
    from directdemod_amd.symbolsync import limBin
    re = np.array([limBin(v) for v in sym.real], dtype=np.int64)
    im = np.array([limBin(v) for v in sym.imag], dtype=np.int64)
    rows = []
    if policy == "meteor":
        w = qpsk.NSYNC // 2
        for k in range(w - 1, len(sym)):
            m1, m2 = qpsk._scores(np.stack((re[k - w + 1:k + 1], im[k - w + 1:k + 1]), axis=1))
            if qpsk._fires(m1) or qpsk._fires(m2):
                rows.append((k, m1, m2))
        return (re | (im << 1)).astype(np.uint8), rows
    s12 = bpsk.sync12khz()
    for k in range(bpsk.WIN - 1, len(sym)):
        m = int(np.sum(np.abs(re[k - bpsk.WIN + 1:k + 1] - s12)))
        if np.abs(m - (len(s12) / 2)) > 120:
            rows.append((k, m))
    return re.astype(np.uint8), rows


def dev_minsync(hip, policy, sym, cap):
    """-> (count, cand whole: width * (cap + SPARE) words with the sentinel where not written, bits)"""
    from directdemod_amd import bpsk, qpsk
    entry, width = MINSYNC[policy]
    if policy == "meteor":
        s72, s1, _ = qpsk.sync_patterns()
        sb = np.ascontiguousarray(np.concatenate((s72, s1)), dtype=np.uint8)
    else:
        sb = np.ascontiguousarray(bpsk.sync_bits(), dtype=np.uint8)
    n = len(sym)
    dsym = hip.DevArray.from_host(np.ascontiguousarray(sym, dtype=np.complex128))
    bits = hip.DevArray.from_host(np.full(n + SPARE, 0xEE, dtype=np.uint8))
    cand = hip.DevArray.from_host(np.full(width * (cap + SPARE), SENT_I, dtype=np.int64))
    cnt = hip.DevArray.from_host(np.full(1, 12345, dtype=np.uint64))
    hip.check(getattr(hip.lib(), entry)(dsym.ptr, n, sb.ctypes.data, bits.ptr, cap, cand.ptr, cnt.ptr, None), entry)
    hip.sync()
    return int(cnt.to_host()[0]), cand.to_host().reshape(-1, width), bits.to_host()


def check_minsync(hip, policy, sym, want_fired=None):
    bits, rows = minsync_expected(policy, sym)
    count, cand, got_bits = dev_minsync(hip, policy, sym, len(sym))
    assert np.array_equal(got_bits[:len(sym)], bits) and np.all(got_bits[len(sym):] == 0xEE)
    assert count == len(rows)
    got = cand[:count]
    assert sorted(map(tuple, got.tolist())) == rows                 # the order of the compaction is not defined
    assert np.all(cand[count:] == SENT_I)
    if want_fired is not None:
        assert [r[0] for r in rows] == want_fired, rows
    return rows


def _win(policy):
    return 60 if policy == "meteor" else 330


@pytest.mark.parametrize("policy", POLICIES)
def test_minsync_window_edges(hip, policy):
    """nsym one below, at and one above the window, 257 (two workgroups) and 1000: the pattern planted in the first full window,
    and inverted (the other polarity) in the last: that window fires with no bit wrong, or with every bit wrong (a Meteor window
    one symbol off does not fire; a Funcube window does, its sync bits being ten symbols long)"""
    w = _win(policy)
    every = 2 * w if policy == "meteor" else w
    for nsym in sorted({w - 1, w, w + 1, 257, 1000}):
        if nsym < w:
            check_minsync(hip, policy, minsync_symbols(policy, nsym, [], 30), [])
            continue
        for at, inverted in ((0, False), (nsym - w, True)):
            sym = minsync_symbols(policy, nsym, [(at, 0, inverted, 0)], 30 + nsym)
            k = at + w - 1
            rows = check_minsync(hip, policy, sym, [k] if policy == "meteor" else None)
            assert [r for r in rows if r[0] == k][0][1] == (every if inverted else 0)


@pytest.mark.parametrize("policy", POLICIES)
def test_minsync_thresholds(hip, policy):
    """planted windows with a chosen number of flipped bits on both sides of either threshold: |m - 60| > 30 (Meteor: 29 and 91
    fire, 30, 31, 89 and 90 do not; for both scores, the second from the swapped (im, re) pattern), |m - 165| > 120 (Funcube: 44
    and 286 fire, 45 and 285 do not)"""
    w = _win(policy)
    if policy == "meteor":
        cases = [(which, f, f < 30 or f > 90) for which in (0, 1) for f in (29, 30, 31, 89, 90, 91)]
    else:
        cases = [(0, f, f < 45 or f > 285) for f in (44, 45, 285, 286)]
    nsym = 1000
    step = 75 if policy == "meteor" else 335
    per = (nsym - w) // step
    seed = 50
    while cases:
        now, cases = cases[:per], cases[per:]
        plants = [(5 + i * step, which, False, f) for i, (which, f, _) in enumerate(now)]
        sym = minsync_symbols(policy, nsym, plants, seed)
        seed += 1
        bits, rows = minsync_expected(policy, sym)
        by_k = {r[0]: r for r in rows}
        for (at, which, _, f), (_, _, fires) in zip(plants, now):
            k = at + w - 1
            assert (k in by_k) == fires, (which, f)
            if fires:
                assert by_k[k][1 + which] == f
        if policy == "meteor":
            assert len(rows) == sum(1 for c in now if c[2])
        check_minsync(hip, policy, sym)


@pytest.mark.parametrize("policy", POLICIES)
def test_minsync_zero_and_nan_symbols_and_a_small_capacity(hip, policy):
    """0.0, -0.0 (limBin: 0) and NaN (limBin: 1) among the symbols; with cap below the count the count is the total, the first cap
    rows are distinct members of the expected set, and nothing is written after them"""
    w = _win(policy)
    nsym = 1000
    sym = minsync_symbols(policy, nsym, [(0, 0, False, 0), (w + 5, 0, True, 3), (nsym - w, 0, False, 2)], 60)
    sym[2 * w + 6] = complex(0.0, -0.0)
    sym[2 * w + 7] = complex(-0.0, 0.0)
    sym[2 * w + 8] = complex(float("nan"), 1.0)
    sym[2 * w + 9] = complex(-1.0, float("nan"))
    zero_bits = int(np.nonzero(minsync_patterns(policy)[0].sum(axis=1) == 0)[0][0])
    sym[zero_bits] = complex(0.0, -0.0)                             # inside the first planted window, where the pattern's bits are 0
    bits, rows = minsync_expected(policy, sym)
    assert bits[2 * w + 6] == 0 and bits[2 * w + 7] == 0 and bits[2 * w + 8] & 1 == 1 and (policy == "funcube" or bits[2 * w + 9] == 2)
    rows = check_minsync(hip, policy, sym)
    assert rows[0][:2] == (w - 1, 0) and len(rows) >= 3             # the zeros read as 0: the first window has no bit wrong
    for cap in (len(rows) - 1, 1, 0):
        count, cand, _ = dev_minsync(hip, policy, sym, cap)
        assert count == len(rows)
        got = list(map(tuple, cand[:cap].tolist()))
        assert len(set(got)) == cap and set(got) <= set(rows)
        assert np.all(cand[cap:] == SENT_I)


# ------------------------------------------------------------------------------------------------------------------ MAXSYNC
def meteor_templates():
    from directdemod_amd import qpsk
    s72, _, s2 = qpsk.sync_patterns()
    return [np.where(s72 == 1, 127, -128).astype(np.int64), np.where(s2 == 1, 127, -128).astype(np.int64)]


def meteor_maxcorr(hip, items):
    """items = [(buffer entries int8 (re, im interleaved), template number, split)]: each buffer laid into one lim array between
    random samples, as one interval (split None) or two (split = samples in the first) -> the device's (argmax, max) rows, one call"""
    from directdemod_amd import qpsk
    rng = np.random.Generator(np.random.PCG64(70))
    parts, bufs = [], []
    at = 0

    def put(e):
        nonlocal at
        parts.append(np.asarray(e, dtype=np.int8))
        lo = at // 2
        at += len(e)
        return lo
    for e, tm, split in items:
        put(rng.integers(-128, 128, 2 * 7))
        ns = len(e) // 2
        if split is None:
            ivs = [(put(e), ns)]
        else:
            lo0 = put(e[:2 * split])
            put(rng.integers(-128, 128, 2 * 3))
            ivs = [(lo0, split), (put(e[2 * split:]), ns - split)]
        bufs.append((ivs, ivs[0][0], tm))
    put(rng.integers(-128, 128, 2 * 5))
    lim = hip.DevArray.from_host(np.concatenate(parts).view(np.int16))
    return qpsk.maxsync_argmax(lim, bufs), lim


def corr_reference(e, t, rep):
    r = np.abs(np.correlate(np.asarray(e, dtype=np.int64), np.repeat(t, rep), "same"))
    return int(np.argmax(r)), int(r.max())


def test_meteor_maxcorr_against_numpy(hip):
    """|np.correlate(buf, np.repeat(t, 28), 'same')| and its first argmax: the shortest and the longest buffer and lengths between
    (no multiple of the 256 lags a pass takes), both templates, one interval and two with either down to no sample, all in one
    call; all zero (argmax 0), all -128 at the greatest length (the largest block sums), a full match at 127 / -128 (the largest lag
    sum), the peak on lag 0 and on the last
    lag, and two equal peaks 27 * 256 lags apart, which one thread meets both: the lower lag wins"""
    rng = np.random.Generator(np.random.PCG64(71))
    T = meteor_templates()
    rep, half = 28, 1680
    items, names = [], []
    for L in (3360, 3362, 13442, 20162, 20480):
        for tm in (0, 1):
            items.append((rng.integers(-128, 128, L), tm, None))
            names.append("random L %d template %d" % (L, tm))
    e = rng.integers(-128, 128, 13442)
    for split in (0, 1, 3000, 13442 // 2 - 1, 13442 // 2):
        items.append((e, 1, split))
        names.append("two intervals, %d samples in the first" % split)
    items.append((np.zeros(3362, dtype=np.int64), 0, None))
    names.append("all zero")
    items.append((np.full(20480, -128), 1, None))
    names.append("all -128")
    tm0 = np.repeat(T[0], rep)
    first = rng.integers(-3, 4, 5000)
    first[:half] = np.where(tm0[half:] > 0, 127, -128)
    items.append((first, 0, None))
    names.append("peak at lag 0")
    last = rng.integers(-3, 4, 5000)
    last[5000 - 1 - half:] = np.where(tm0[:half + 1] > 0, 127, -128)
    items.append((last, 0, 1234))
    names.append("peak at the last lag")
    full = rng.integers(-3, 4, 5000)
    full[500:500 + len(tm0)] = np.where(tm0 > 0, 127, -128)
    items.append((full, 0, None))
    names.append("full match")
    twin = np.zeros(13442, dtype=np.int64)
    for at in (100, 100 + 27 * 256):
        twin[at:at + len(tm0)] = np.where(tm0 > 0, 100, -100)
    items.append((twin, 0, None))
    names.append("two equal peaks")
    got, _ = meteor_maxcorr(hip, items)
    for (e, tm, _), name, row in zip(items, names, got):
        want = corr_reference(e, T[tm], rep)
        assert (int(row[0]), int(row[1])) == want, name
        if name == "all zero":
            assert want == (0, 0)
        elif name == "all -128":
            assert want[1] > 0
        elif name == "full match":
            assert want == (500 + half, int(np.sum(np.abs(tm0) * np.where(tm0 > 0, 127, 128)))) and want[1] > 54000000
        elif name == "peak at lag 0":
            assert want[0] == 0
        elif name == "peak at the last lag":
            assert want[0] == 4999
        elif name == "two equal peaks":
            r = np.abs(np.correlate(e, tm0, "same"))
            assert want[0] == 100 + half and r[100 + half] == r[100 + half + 27 * 256]


def test_meteor_maxcorr_refuses_bad_buffers(hip):
    from directdemod_amd import qpsk
    lim = hip.DevArray.from_host(np.zeros(10300, dtype=np.int16))
    assert qpsk.maxsync_argmax(lim, [([(0, 1680)], 0, 0)]).shape == (1, 2)
    assert qpsk.maxsync_argmax(lim, [([(60, 10240)], 0, 1)]).shape == (1, 2)
    for ivs in ([(0, 1679)], [(0, 10241)], [(0, 5000), (5000, 5241)], [(10300 - 1679, 1680)], [(0, 1680), (10300, 1)], [(-1, 1680)]):
        with pytest.raises(ValueError):
            qpsk.maxsync_argmax(lim, [([(0, 1680)], 0, 0), (ivs, 0, 0)])


def test_funcube_maxcorr_ties_and_zeros(hip):
    """what test_gpu_funcube.py's correlation test leaves: two equal peaks a multiple of the workgroup's 1024 lags apart (one
    thread meets both; the lower lag wins), at a short template against np.correlate, and an all-zero buffer of the full
    template's length and more (argmax 0)"""
    from directdemod_amd import bpsk
    t = bpsk.template_bits()

    def run(buf, rep):
        lv = hip.DevArray.from_host(np.asarray(buf, dtype=np.int8))
        return tuple(int(v) for v in bpsk.maxsync_argmax(lv, [([(0, len(buf))], 0)], rep)[0])
    rep = 5
    tm = np.repeat(t, rep)
    twin = np.zeros(3000, dtype=np.int64)
    for at in (100, 100 + 2048):
        twin[at:at + len(tm)] = np.where(tm > 0, 100, -100)
    r = np.abs(np.correlate(twin, tm, "same"))
    want = corr_reference(twin, t, rep)
    assert want[0] == 100 + len(tm) // 2 and r[want[0]] == r[want[0] + 2048]
    assert run(twin, rep) == want
    assert run(np.zeros(bpsk.TLEN, dtype=np.int64), bpsk.REP) == (0, 0)
    assert run(np.zeros(57001, dtype=np.int64), bpsk.REP) == (0, 0)
