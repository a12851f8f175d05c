"""The OQPSK walk (dd_oqpsk_walk), the re-stagger (dd_lrpt_restagger), decode_lrpt's stagger keyword and decode_meteorm2x on the device.

The walk is defined so that no operation depends on a library (+ - * / sqrt floor and table reads, each
rounded on its own), so every per-symbol array and every field of the carried state is compared with np.array_equal against
tests/_oqpsk.py's walk_host, a sample-by-sample restatement in Python floats.  The rest is integer work and exact as well."""
import ctypes as C

import numpy as np
import pytest

import _lrpt_modes
import _oqpsk as oq
from directdemod_amd import lrpt

pytestmark = pytest.mark.gpu

SPARE = 16                                     # entries past the capacity, which must keep the sentinel
SENT_I = np.int64(-0x5A5A5A5A5A5A5A5B)
SENT_C = np.complex128(complex(-7.25e300, 3.5e-300))


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.int64)


def _state_type():
    from directdemod_amd.oqpsk import STATE
    return STATE


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def dev_walk(hip, rate, x, st, cuts=(), cap=None, base=0):
    """dd_oqpsk_walk over x from the state st (a dict), cut into calls of the lengths `cuts` and a last call with the rest, `base`
    running on -> (the state record after, the four arrays whole: cap + SPARE entries, sentinel where not written)"""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    n = len(x)
    cap = n if cap is None else cap
    dev = {k: hip.DevArray.from_host(np.full(cap + SPARE, SENT_I if k in ("bidx", "aidx") else SENT_C)) for k in oq.ARRAYS}
    dx = hip.DevArray.from_host(x) if n else hip.DevArray(1, np.complex128)
    dstate = hip.DevArray.from_host(oq.state_struct(st, _state_type()).view(np.uint8))
    dtab = hip.DevArray.from_host(oq.table().ravel())
    prm = oq.params_array(oq.params(rate))
    at = 0
    assert sum(cuts) <= n
    for m in list(cuts) + [n - sum(cuts)]:
        hip.check(hip.lib().dd_oqpsk_walk(dx.ptr + 16 * at, m, base + at, dstate.ptr, _pd(prm), dtab.ptr, cap,
                                          *(dev[k].ptr for k in oq.ARRAYS), None), "dd_oqpsk_walk")
        at += m
    hip.sync()
    return dstate.to_host().view(_state_type())[0], {k: dev[k].to_host() for k in oq.ARRAYS}


def check_walk(rate, x, st, state, got, what, base=0, cap=None):
    """device result (state record, whole arrays) against walk_host over the same samples, bit for bit -> the restatement's counters"""
    cap = len(x) if cap is None else cap
    hs, ref, cnt = oq.walk_host(x, base, st, oq.params(rate))
    nsym = hs["ctr"] - st["ctr"]
    assert st["ctr"] == 0 and int(state["ctr"]) == hs["ctr"], what
    m = min(nsym, cap)
    for k in oq.ARRAYS:
        want = ref[k][:m].view(np.complex128).reshape(-1) if k == "uf" else ref[k][:m]
        assert np.array_equal(_bits(got[k][:m]), _bits(want)), (what, k)
        sent = SENT_I if k in ("bidx", "aidx") else SENT_C
        assert np.array_equal(_bits(got[k][m:]), _bits(np.full(len(got[k]) - m, sent))), (what, k, "written past min(ctr, cap)")
    for f in oq.FLOAT_FIELDS:
        assert np.float64(state[f]).view(np.int64) == np.float64(hs[f]).view(np.int64), (what, f, float(state[f]), hs[f])
    for f in oq.INT_FIELDS:
        assert int(state[f]) == ((1 if nsym > cap else st["overflow"]) if f == "overflow" else hs[f]), (what, f)
    return cnt


# ------------------------------------------------------------------------------------------------------------------ dd_oqpsk_walk
@pytest.mark.parametrize("name", sorted(oq.CASES))
def test_walk_named_cases(hip, name):
    """both symbol rates from the start state, a B before any A, the gain cap on both sides, hyp's three ranges, the error clamp,
    lock and unlock, u wrapping past 1 and more than two tiles of A events only: every array and every state field bit for bit"""
    rate, x, st = oq.case(name)
    state, got = dev_walk(hip, rate, x, st)
    cnt = check_walk(rate, x, st, state, got, name)
    for key in oq.CASES[name]["reaches"]:
        assert cnt[key] > 0, (key, cnt)


@pytest.mark.parametrize("rate", sorted(oq.RATES))
def test_walk_lengths_and_tile_edges(hip, rate):
    """lengths around the 64 staging lanes and around one, two and three tiles, each from timing 0 and from start timings that put
    the first A or B on the last sample of a tile and on the first of the next"""
    x = oq.signal(rate, **oq.LENGTH_SIGNAL)
    for n, timing, event in oq.length_runs(rate):
        st = oq.start_state(rate, timing=timing, seen_a=1 if event else 0)
        state, got = dev_walk(hip, rate, x[:n], st)
        check_walk(rate, x[:n], st, state, got, (rate, n, timing, event))


@pytest.mark.parametrize("rate", sorted(oq.RATES))
def test_walk_cut_between_events(hip, rate):
    """calls cut right after an A (its B comes in the next call: the pending I, its sample and the Q mid sample cross in the
    state), right after a B (the pending Q Gardner term crosses), at a tile edge and one sample in, at base 0 and at a base past
    2^31: what one call gives, and what the restatement gives"""
    x = oq.signal(rate, n=6000, seed=12, amp=3.0, noise=24)
    st = oq.start_state(rate)
    _, ref, _ = oq.walk_host(x, 0, st, oq.params(rate))
    a, b = int(ref["aidx"][40]), int(ref["bidx"][40])
    assert a < b < int(ref["aidx"][41])
    whole_state, whole = dev_walk(hip, rate, x, st)
    check_walk(rate, x, st, whole_state, whole, "one call")
    for cuts in ((a + 1,), (b + 1,), (a + 1, b - a), (1,), (1024, 1), (1023, 2, 2047), (a, 1, b - a - 1, 1)):
        state, got = dev_walk(hip, rate, x, st, cuts=cuts)
        assert state.tobytes() == whole_state.tobytes(), cuts
        for k in oq.ARRAYS:
            assert np.array_equal(_bits(got[k]), _bits(whole[k])), (cuts, k)
    base = (1 << 31) + 12345
    state, got = dev_walk(hip, rate, x[:3000], st, cuts=(a + 1,), base=base)
    check_walk(rate, x[:3000], st, state, got, "large base", base=base)
    assert got["aidx"][0] >= base and got["bidx"][0] > got["aidx"][0]


def test_walk_capacity_overflow(hip):
    """fewer entries than symbols: the first cap are written, the entries past them keep their sentinel, the flag is set and the
    count runs on; a later call keeps the flag"""
    rate, x, st = oq.case("default_72k")
    hs, ref, _ = oq.walk_host(x, 0, st, oq.params(rate))
    assert hs["ctr"] > 100
    for cap in (0, 1, 100):
        state, got = dev_walk(hip, rate, x, st, cap=cap)
        check_walk(rate, x, st, state, got, ("cap", cap), cap=cap)
        assert int(state["overflow"]) == 1 and int(state["ctr"]) == hs["ctr"]
    state, got = dev_walk(hip, rate, x, st, cuts=(4096,), cap=hs["ctr"])
    assert int(state["overflow"]) == 0
    st1 = dict(st, overflow=1)
    state, _ = dev_walk(hip, rate, x[:100], st1)
    assert int(state["overflow"]) == 1


def test_walk_no_samples_and_bad_arguments(hip):
    """n = 0 returns at once and leaves the state (null sample and output buffers allowed); null buffers with n > 0, a null state,
    parameter block or table, and negative sizes are refused with DD_ERR_INVALID and nothing is launched"""
    rate = 72000
    st0 = oq.state_struct(oq.start_state(rate, timing=3.5, u=0.25), _state_type())
    dstate = hip.DevArray.from_host(st0.view(np.uint8))
    dtab = hip.DevArray.from_host(oq.table().ravel())
    prm = oq.params_array(oq.params(rate))
    dx = hip.DevArray.from_host(np.ones(8, dtype=np.complex128))
    out = [hip.DevArray.from_host(np.full(8, SENT_I)) for _ in range(2)] + [hip.DevArray.from_host(np.full(8, SENT_C)) for _ in range(2)]
    fn = hip.lib().dd_oqpsk_walk
    ptrs = [d.ptr for d in out]
    assert fn(None, 0, 0, dstate.ptr, _pd(prm), dtab.ptr, 0, None, None, None, None, None) == hip.DD_OK
    assert fn(dx.ptr, 0, 5, dstate.ptr, _pd(prm), dtab.ptr, 8, *ptrs, None) == hip.DD_OK
    bad = [(None, 8, 0, dstate.ptr, _pd(prm), dtab.ptr, 8, *ptrs),
           (dx.ptr, 8, 0, None, _pd(prm), dtab.ptr, 8, *ptrs),
           (dx.ptr, 8, 0, dstate.ptr, None, dtab.ptr, 8, *ptrs),
           (dx.ptr, 8, 0, dstate.ptr, _pd(prm), None, 8, *ptrs),
           (dx.ptr, -1, 0, dstate.ptr, _pd(prm), dtab.ptr, 8, *ptrs),
           (dx.ptr, 8, -1, dstate.ptr, _pd(prm), dtab.ptr, 8, *ptrs),
           (dx.ptr, 8, 0, dstate.ptr, _pd(prm), dtab.ptr, -1, *ptrs)]
    for i in range(4):
        p = list(ptrs)
        p[i] = None
        bad.append((dx.ptr, 8, 0, dstate.ptr, _pd(prm), dtab.ptr, 8, *p))
    for args in bad:
        assert fn(*args, None) == hip.DD_ERR_INVALID, args
        with pytest.raises(ValueError):
            hip.check(fn(*args, None), "dd_oqpsk_walk")
    hip.sync()
    assert dstate.to_host().tobytes() == st0.tobytes()
    assert all(np.array_equal(_bits(d.to_host()), _bits(np.full(8, SENT_I if i < 2 else SENT_C))) for i, d in enumerate(out))


def test_walker_class_starts_as_the_restatement(hip):
    from directdemod_amd import oqpsk
    for rate in sorted(oq.RATES):
        x = oq.signal(rate, n=5000, seed=13, amp=3.0, noise=24)
        st = oq.start_state(rate)
        w = oqpsk.Walker(oq.FS, len(x), rate)
        assert w.state.to_host().tobytes() == oq.state_struct(st, _state_type()).tobytes()
        assert np.array_equal(w.params, oq.params_array(oq.params(rate))) and np.array_equal(w.table.to_host().reshape(-1, 2), oq.table())
        w.walk(hip.DevArray.from_host(x[:3000]))
        w.walk(hip.DevArray.from_host(x[3000:]))
        hs, ref, _ = oq.walk_host(x, 0, st, oq.params(rate))
        assert w.nsym == hs["ctr"] > 0 and w.fed == len(x)
        for k in ("bidx", "aidx", "sym"):
            assert np.array_equal(_bits(w.view(k).to_host()), _bits(ref[k])), k
        assert np.array_equal(w.view("uf").to_host().view(np.float64).reshape(-1, 2), ref["uf"])
        with pytest.raises(ValueError):
            w.walk(hip.DevArray.from_host(x[:1]))
    with pytest.raises(ValueError):
        oqpsk.Walker(oq.FS, 100, 12000)
    small = oqpsk.Walker(oq.FS, 4096, 72000)
    small.cap = 3
    with pytest.raises(RuntimeError):
        small.walk(hip.DevArray.from_host(oq.signal(72000, n=4096, seed=13, amp=3.0, noise=24)))


# ------------------------------------------------------------------------------------------------------------------ dd_lrpt_restagger
@pytest.mark.parametrize("nsym", [0, 1, 2, 255, 256, 257, 1000])
def test_restagger_against_numpy(hip, nsym):
    rng = np.random.Generator(np.random.PCG64(30 + nsym))
    soft = rng.integers(-128, 128, 2 * nsym + 6, dtype=np.int8)
    if nsym >= 2:
        soft[[0, 1, 2 * nsym - 2, 2 * nsym - 1]] = [-128, 127, 127, -128]
    d = hip.DevArray.from_host(soft)
    for s in (-1, 0, 1):
        got = lrpt.restagger(d, nsym, s)
        assert got.dtype == np.dtype(np.int8) and np.array_equal(got.to_host(), lrpt.restagger_np(soft, nsym, s)), (nsym, s)
    # nothing past the nout pairs is written
    out = hip.DevArray.from_host(np.full(2 * nsym + 8, -77, dtype=np.int8))
    hip.check(hip.lib().dd_lrpt_restagger(d.ptr, nsym, -1, out.ptr, None), "dd_lrpt_restagger")
    assert np.all(out.to_host()[2 * max(nsym - 1, 0):] == -77)


def test_restagger_bad_arguments(hip):
    d = hip.DevArray.from_host(np.zeros(16, dtype=np.int8))
    fn = hip.lib().dd_lrpt_restagger
    for args in ((d.ptr, 8, 2, d.ptr), (d.ptr, 8, -2, d.ptr), (d.ptr, -1, 0, d.ptr), (None, 8, 0, d.ptr), (d.ptr, 8, 1, None)):
        assert fn(*args, None) == hip.DD_ERR_INVALID, args
    assert fn(None, 0, 0, None, None) == hip.DD_OK and fn(None, 1, 1, None, None) == hip.DD_OK
    with pytest.raises(ValueError):
        lrpt.restagger(d, 8, 3)


# ------------------------------------------------------------------------------------------------------------------ decode_lrpt(stagger=)
@pytest.mark.parametrize("differential,interleaved", [(False, False), (True, False), (True, True)])
def test_decode_lrpt_stagger(hip, differential, interleaved):
    """a stream re-staggered on the host by -s decodes with stagger=s and with "auto" to the frames of the unstaggered stream, and
    "auto" says s; the default keyword gives what it gave before there was one (no new timings key either)"""
    from directdemod_amd import decode_lrpt
    bodies = _lrpt_modes.random_bodies(660, 3)
    s0 = _lrpt_modes.stream(bodies, 661, differential=differential, interleaved=interleaved, branches=36, delay=8, prefix=90, hyp=3)
    kw = dict(differential=differential, interleaved=interleaved, branches=36, delay=8)
    plain = decode_lrpt.decode_lrpt(s0["soft"], **kw)
    assert np.array_equal(plain.getFrames, bodies) and plain.stagger == 0 and "lrpt_stagger" not in plain.timings
    assert plain.frameInfo["symbol"].tolist() == s0["starts"]
    auto0 = decode_lrpt.decode_lrpt(s0["soft"], stagger="auto", **kw)
    assert auto0.stagger == 0 and np.array_equal(auto0.getFrames, bodies) and np.array_equal(auto0.frameInfo, plain.frameInfo)
    assert auto0.timings["lrpt_stagger"] >= 0.0
    for s in (-1, 1):
        soft = lrpt.restagger_np(s0["soft"], s0["nsym"], -s)
        for arg in (s, "auto"):
            obj = decode_lrpt.decode_lrpt(hip.DevArray.from_host(soft) if arg == "auto" else soft, stagger=arg, **kw)
            assert obj.stagger == s and obj.locked is True
            frames, info = obj.getFrames, obj.frameInfo
            # a symbol is lost at either end: without the interleaver the last frame no longer fits
            keep = len(bodies) if interleaved else len(bodies) - 1
            assert np.array_equal(frames, bodies[:keep]) and not info["asm_errors"].any(), (s, arg)
            if not interleaved:
                assert info["symbol"].tolist() == [p - 1 for p in s0["starts"][:keep]]
        wrong = decode_lrpt.decode_lrpt(soft, **kw)
        assert wrong.stagger == 0 and len(wrong.getFrames) == 0
    for bad in (2, "both", None, True, 1.5):
        with pytest.raises(ValueError):
            decode_lrpt.decode_lrpt(s0["soft"], stagger=bad)


# ------------------------------------------------------------------------------------------------------------------ decode_meteorm2x
def _decode(name, **kw):
    from directdemod_amd import decode_meteorm2x, source
    c = dict(oq.RECORDINGS[name])
    c.update(kw.pop("recording", {}))
    rec = oq.recording(**c)
    obj = decode_meteorm2x.decode_meteorm2x(source.IQarray(rec["raw"], oq.FS), rec["carrier"], symbol_rate=c["symbol_rate"], **kw)
    return rec, obj


@pytest.fixture(scope="module")
def first_case(hip):
    rec, obj = _decode("72k_s0")
    obj.getFrames
    return rec, obj


def _check_frames(rec, obj):
    w = obj.walker()
    aidx = w.view("aidx").to_host()
    expected = oq.expected_frames(rec, aidx)
    assert len(expected) >= 5
    rows = oq.frames_found(obj.getFrames, obj.frameInfo, rec["bodies"], expected)
    return w, aidx, rows


def test_meteorm2x_72k_lock_at_0_degrees(hip, first_case):
    rec, obj = first_case
    w, aidx, rows = _check_frames(rec, obj)
    assert obj.stagger == 0 and obj.locked is True and len(obj.deintInfo) == 0
    info = obj.frameInfo
    assert np.array_equal(info["sample"], aidx[info["symbol"]]) and np.all(np.diff(info["sample"]) > 0)
    assert list(obj.timings)[:2] == ["front_end", "walk"] and all(obj.timings[k] >= 0.0 for k in ("lrpt_stagger", "lrpt_viterbi"))
    sym = obj.getSymbols
    assert sym.sampRate == 72000 and sym.length == w.nsym
    soft = obj.getSoft
    assert soft.dtype == np.int8 and np.array_equal(soft, lrpt.soft_np(w.view("sym").to_host()))
    assert obj.getVCDUs.shape == (len(info), 892) and obj.getImage.shape[1:] == (1568, 3)
    rot, ok = oq.decisions({k: w.view(k).to_host() for k in ("aidx", "bidx", "sym")}, rec["code"], 72000)
    assert rot % 2 == 0 and ok[oq.ACQ:].all()


def test_meteorm2x_72k_lock_at_90_degrees(hip):
    """the carrier phase at which the walk locks a quarter turn off: its rails come out one symbol apart, "auto" finds -1, and
    frameInfo['sample'] is the A sample of the symbol whose I rail opens the frame"""
    rec, obj = _decode("72k_s1")
    w, aidx, rows = _check_frames(rec, obj)
    assert obj.stagger == -1
    info = obj.frameInfo
    assert np.array_equal(info["sample"], aidx[info["symbol"] + 1])
    rot, ok = oq.decisions({k: w.view(k).to_host() for k in ("aidx", "bidx", "sym")}, rec["code"], 72000)
    assert rot % 2 == 1 and ok[oq.ACQ:].all()


def test_meteorm2x_80k_interleaved(hip):
    rec, obj = _decode("80k_s1", recording=dict(interleaved=True, delay=8), interleaved=True, delay=8)
    _check_frames(rec, obj)
    assert obj.locked is True and obj.stagger == -1 and np.all(obj.frameInfo["sample"] == -1)
    lock = obj.lock
    assert 4 * lock["score"] >= 3 * 8 * lock["markers"] and len(obj.deintInfo) >= 1


@pytest.mark.parametrize("interleaved", [False, True])
def test_meteorm2x_noise_only(hip, interleaved):
    from directdemod_amd import decode_meteorm2x, source
    rng = np.random.Generator(np.random.PCG64(670))
    raw = np.clip(np.rint(127.5 + 20.0 * rng.standard_normal((400000, 2))), 0, 255).astype(np.uint8)
    obj = decode_meteorm2x.decode_meteorm2x(source.IQarray(raw, oq.FS), 300.0, symbol_rate=80000 if interleaved else 72000,
                                            interleaved=interleaved, delay=8)
    assert obj.getFrames.shape == (0, 1020) and len(obj.frameInfo) == 0 and obj.getPackets == []
    assert obj.locked is (not interleaved) and obj.stagger in (0, -1, 1) and obj.walker().nsym > 10000


def test_meteorm2x_chunked_is_the_one_chunk_run(hip, first_case):
    rec, ref = first_case
    from directdemod_amd import decode_meteorm2x, source
    obj = decode_meteorm2x.decode_meteorm2x(source.IQarray(rec["raw"], oq.FS), rec["carrier"], chunk_size=300001)
    assert np.array_equal(obj.getFrames, ref.getFrames) and len(ref.getFrames) >= 5
    assert np.array_equal(obj.frameInfo["sample"], ref.frameInfo["sample"])
    assert obj.stagger == ref.stagger


def test_meteorm2x_bad_arguments(hip):
    from directdemod_amd import decode_meteorm2x, source
    src = source.IQarray(np.full((100, 2), 127, dtype=np.uint8), oq.FS)
    with pytest.raises(ValueError):
        decode_meteorm2x.decode_meteorm2x(src, 0, symbol_rate=64000)
    with pytest.raises(ValueError):
        decode_meteorm2x.decode_meteorm2x(src, 0, interleaved=True, branches=5)
    import directdemod_amd
    assert "decode_meteorm2x" in directdemod_amd.__all__
