"""The G3RUH 9600 baud FSK chain on the device: the timing walk (dd_fsk_walk), the decision / descrambler / NRZI stage (dd_fsk_bits),
fsk.walk and fsk.bit_stream, and decode_fsk9600 end to end.

The walk is defined so that no operation depends on a library (+ - * / abs and comparisons, each rounded
on its own), so every per-symbol array and every field of the carried state is compared with np.array_equal against tests/_fsk.py's
walk_host, a sample-by-sample restatement in Python floats.  The rest is integer work and exact as well: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import _fsk as fk

pytestmark = pytest.mark.gpu

SPARE = 16                                     # entries past the capacity, which must keep the sentinel
SENT_I = np.int64(-0x5A5A5A5A5A5A5A5B)
SENT_F = np.float64(-7.25e300)
SENT = dict(sym=SENT_F, sidx=SENT_I, tmu=SENT_F)


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.int64)


def _state_type():
    from directdemod_amd.fsk import STATE
    return STATE


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def dev_walk(hip, prm, x, st, cuts=(), cap=None, base=0):
    """dd_fsk_walk over x from the state st (a dict), cut into calls of the lengths `cuts` and a last call with the rest, `base`
    running on -> (the state record after, the three arrays whole: cap + SPARE entries, sentinel where not written)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    cap = n if cap is None else cap
    dev = {k: hip.DevArray.from_host(np.full(cap + SPARE, SENT[k])) for k in fk.ARRAYS}
    dx = hip.DevArray.from_host(x) if n else hip.DevArray(1, np.float64)
    dstate = hip.DevArray.from_host(fk.state_struct(st, _state_type()).view(np.uint8))
    p = fk.params_array(prm)
    at = 0
    assert sum(cuts) <= n
    for m in list(cuts) + [n - sum(cuts)]:
        hip.check(hip.lib().dd_fsk_walk(dx.ptr + 8 * at, m, base + at, dstate.ptr, _pd(p), cap, *(dev[k].ptr for k in fk.ARRAYS), None),
                  "dd_fsk_walk")
        at += m
    hip.sync()
    return dstate.to_host().view(_state_type())[0], {k: dev[k].to_host() for k in fk.ARRAYS}


def check_walk(prm, x, st, state, got, what, base=0, cap=None):
    """device result (state record, whole arrays) against walk_host over the same samples, bit for bit -> the restatement's counters"""
    cap = len(x) if cap is None else cap
    hs, ref, cnt = fk.walk_host(x, base, st, prm)
    nsym = hs["ctr"] - st["ctr"]
    assert st["ctr"] == 0 and int(state["ctr"]) == hs["ctr"], what
    m = min(nsym, cap)
    for k in fk.ARRAYS:
        assert np.array_equal(_bits(got[k][:m]), _bits(ref[k][:m])), (what, k)
        assert np.array_equal(_bits(got[k][m:]), _bits(np.full(len(got[k]) - m, SENT[k]))), (what, k, "written past min(ctr, cap)")
    for f in fk.FLOAT_FIELDS:
        assert np.float64(state[f]).view(np.int64) == np.float64(hs[f]).view(np.int64), (what, f, float(state[f]), hs[f])
    assert int(state["overflow"]) == (1 if nsym > cap else st["overflow"]), what
    return cnt


# ------------------------------------------------------------------------------------------------------------------ dd_fsk_walk
@pytest.mark.parametrize("name", sorted(fk.CASES))
def test_walk_named_cases(hip, name):
    """the interpolated mid and eye events at a fractional period, P = 2 and P = 64, the clamp on both sides, a dc offset, an eye
    before any mid, am = 0 under the guard, a subnormal am that stalls above 0, and more than two tiles of eye events only: every
    array and every state field bit for bit"""
    prm, x, st = fk.case(name)
    state, got = dev_walk(hip, prm, x, st)
    cnt = check_walk(prm, x, st, state, got, name)
    for key in fk.CASES[name]["reaches"]:
        assert cnt[key] > 0, (key, cnt)


@pytest.mark.parametrize("P", [2.0, fk.P_FRAC, 64.0])
def test_walk_lengths(hip, P):
    x = fk.signal(P, max(fk.LENGTHS), 10)
    prm = fk.params(P)
    for n in fk.LENGTHS:
        for t in (0.0, P + 0.25 - (n - 1)):               # from the start, and with the first eye event on the last sample
            st = fk.start_state(t=t)
            state, got = dev_walk(hip, prm, x[:n], st)
            check_walk(prm, x[:n], st, state, got, (P, n, t))


@pytest.mark.parametrize("P", [2.0, fk.P_FRAC, 64.0])
def test_walk_cut_into_calls(hip, P):
    """the same input cut at 1, at a tile edge and a sample either side, in the middle of a tile and twice, with base running on,
    at base 0 and past 2^31: what one call gives, and what the restatement gives"""
    x = fk.signal(P, 2051, 11)
    prm, st = fk.params(P), fk.start_state()
    whole_state, whole = dev_walk(hip, prm, x, st)
    check_walk(prm, x, st, whole_state, whole, "one call")
    for cuts in fk.CUTS:
        state, got = dev_walk(hip, prm, x, st, cuts=cuts)
        assert state.tobytes() == whole_state.tobytes(), cuts
        for k in fk.ARRAYS:
            assert np.array_equal(_bits(got[k]), _bits(whole[k])), (cuts, k)
    base = (1 << 31) + 12345
    state, got = dev_walk(hip, prm, x, st, cuts=(1025,), base=base)
    check_walk(prm, x, st, state, got, "large base", base=base)
    assert got["sidx"][0] >= base


def test_walk_capacity_overflow(hip):
    """fewer entries than symbols: the first cap are written, the entries past them keep their sentinel, the flag is set and the
    count runs on; a later call keeps the flag"""
    prm, x, st = fk.case("fractional")
    hs, _, _ = fk.walk_host(x, 0, st, prm)
    assert hs["ctr"] > 100
    for cap in (0, 1, 100):
        state, got = dev_walk(hip, prm, x, st, cap=cap)
        check_walk(prm, x, st, state, got, ("cap", cap), cap=cap)
        assert int(state["overflow"]) == 1 and int(state["ctr"]) == hs["ctr"]
    state, _ = dev_walk(hip, prm, x, st, cuts=(2048,), cap=hs["ctr"])
    assert int(state["overflow"]) == 0
    state, _ = dev_walk(hip, prm, x[:100], dict(st, overflow=1))
    assert int(state["overflow"]) == 1


def test_walk_no_samples_and_bad_arguments(hip):
    """n = 0 returns at once and leaves the state (null sample and output buffers allowed); null buffers with n > 0, a null state or
    parameter block, negative sizes and a period outside 2 .. 64 (a NaN too) are refused with DD_ERR_INVALID, nothing is launched"""
    st0 = fk.state_struct(fk.start_state(t=3.5, dc=0.25), _state_type())
    dstate = hip.DevArray.from_host(st0.view(np.uint8))
    prm = fk.params_array(fk.params(5.0))
    dx = hip.DevArray.from_host(np.ones(8))
    out = [hip.DevArray.from_host(np.full(8, SENT[k])) for k in fk.ARRAYS]
    fn = hip.lib().dd_fsk_walk
    ptrs = [d.ptr for d in out]
    assert fn(None, 0, 0, dstate.ptr, _pd(prm), 0, None, None, None, None) == hip.DD_OK
    assert fn(dx.ptr, 0, 5, dstate.ptr, _pd(prm), 8, *ptrs, None) == hip.DD_OK
    bad = [(None, 8, 0, dstate.ptr, _pd(prm), 8, *ptrs),
           (dx.ptr, 8, 0, None, _pd(prm), 8, *ptrs),
           (dx.ptr, 8, 0, dstate.ptr, None, 8, *ptrs),
           (dx.ptr, -1, 0, dstate.ptr, _pd(prm), 8, *ptrs),
           (dx.ptr, 8, -1, dstate.ptr, _pd(prm), 8, *ptrs),
           (dx.ptr, 8, 0, dstate.ptr, _pd(prm), -1, *ptrs)]
    for i in range(3):
        p = list(ptrs)
        p[i] = None
        bad.append((dx.ptr, 8, 0, dstate.ptr, _pd(prm), 8, *p))
    keep = []
    for P in (1.999, 64.001, float("nan"), float("inf"), -5.0):
        keep.append(fk.params_array(fk.params(P)))
        bad.append((dx.ptr, 8, 0, dstate.ptr, _pd(keep[-1]), 8, *ptrs))
    for args in bad:
        assert fn(*args, None) == hip.DD_ERR_INVALID, args
        with pytest.raises(ValueError):
            hip.check(fn(*args, None), "dd_fsk_walk")
    hip.sync()
    assert dstate.to_host().tobytes() == st0.tobytes()
    assert all(np.array_equal(_bits(d.to_host()), _bits(np.full(8, SENT[k]))) for k, d in zip(fk.ARRAYS, out))


def test_fsk_walk_function_chunked_is_one_call(hip):
    from directdemod_amd import fsk
    rate = 2048000 / 42
    prm, x, st = fk.case("fractional")
    hs, ref, _ = fk.walk_host(x, 0, st, prm)
    d = hip.DevArray.from_host(x)
    sym, sidx, tmu, state = fsk.walk(d, rate)
    for k, a in zip(fk.ARRAYS, (sym, sidx, tmu)):
        assert np.array_equal(_bits(a.to_host()), _bits(ref[k])), k
    assert int(state["ctr"][0]) == hs["ctr"] and state.dtype == fsk.STATE
    s1, i1, _, mid = fsk.walk(d.view(0, 1500), rate)
    s2, i2, _, end = fsk.walk(d.view(1500, len(x) - 1500), rate, state=mid, base=1500)
    assert end.tobytes() == state.tobytes()
    assert np.array_equal(_bits(np.concatenate((s1.to_host(), s2.to_host()))), _bits(ref["sym"]))
    assert np.array_equal(np.concatenate((i1.to_host(), i2.to_host())), ref["sidx"])
    with pytest.raises(ValueError, match="9600"):
        fsk.walk(d, 9600.0)
    with pytest.raises(TypeError):
        fsk.walk(x, rate)
    with pytest.raises(RuntimeError):                      # a start timing that fires at every sample: more symbols than the room
        st = fsk.state0()
        st["t"] = 1e9
        fsk.walk(hip.DevArray.from_host(fk.signal(64.0, 4096, 12)), 64 * 9600.0, state=st)


# ------------------------------------------------------------------------------------------------------------------ dd_fsk_bits
def dev_bits(hip, sym, cap_flags=None):
    n = len(sym)
    cap_flags = max(n, 1) if cap_flags is None else cap_flags
    d = hip.DevArray.from_host(np.ascontiguousarray(sym, dtype=np.float64)) if n else hip.DevArray(1, np.float64)
    outs = [hip.DevArray.from_host(np.full(n + SPARE, -77, dtype=np.int8)) for _ in range(3)]
    flags = hip.DevArray.from_host(np.full(cap_flags + SPARE, SENT_I))
    counts = np.full(2, -1, dtype=np.int64)
    rc = hip.lib().dd_fsk_bits(d.ptr, n, *(o.ptr for o in outs), flags.ptr, cap_flags, counts.ctypes.data_as(C.POINTER(C.c_int64)), None)
    hip.sync()
    return rc, counts, [o.to_host() for o in outs], flags.to_host()


def random_symbols(n, seed):
    """soft symbols with zeros, both signed zeros and a NaN among them (none of them > 0)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    sym = rng.integers(-3, 4, n).astype(np.float64) / 2.0
    if n > 20:
        sym[[3, 7, 11]] = [-0.0, np.nan, 5e-324]
    return sym


@pytest.mark.parametrize("nsym", [0, 1, 12, 13, 17, 18, 255, 256, 257, 273, 773])
def test_bits_against_numpy(hip, nsym):
    """the lengths around the descrambler's taps and around the 256-thread blocks (at 257 and 273 the 12- and 17-symbol look-back
    crosses a block edge; 773 = 3 blocks and 5)"""
    for seed in (nsym, 1000 + nsym):
        sym = random_symbols(nsym, seed)
        rc, counts, (r, bits, marks), flags = dev_bits(hip, sym)
        want = fk.bits_host(sym)
        assert rc == hip.DD_OK and counts.tolist() == [nsym, len(want[3])]
        for got, ref in zip((r, bits, marks), want):
            assert np.array_equal(got[:nsym], ref) and np.all(got[nsym:] == -77)
        assert np.array_equal(flags[:counts[1]], want[3]) and np.all(flags[counts[1]:] == SENT_I)


def _flag_stream(n, seed):
    """bits with the flag at its first (1: bit 0 is 1 by definition) and its last (n - 9) admissible position"""
    rng = np.random.Generator(np.random.PCG64(seed))
    b = rng.integers(0, 2, n).astype(np.int8)
    b[0] = 1
    b[1:9] = b[n - 9:n - 1] = [0, 1, 1, 1, 1, 1, 1, 0]
    return b


def test_bits_flags_at_either_end_and_flag_capacity(hip):
    from directdemod_amd import fsk
    for n in (18, 300, 2049):
        b = _flag_stream(n, n)
        sym = fk.symbols_for(b)
        want = fk.bits_host(sym)
        assert np.array_equal(want[1], b) and want[3][0] == 1 and want[3][-1] == n - 9
        nf = len(want[3])
        rc, counts, (r, bits, marks), flags = dev_bits(hip, sym)
        assert rc == hip.DD_OK and np.array_equal(bits[:n], b) and np.array_equal(flags[:nf], want[3]) and counts[1] == nf
        # a flag in the last eight bits is none: the same stream cut short by one
        rc, counts, _, flags = dev_bits(hip, sym[:n - 1])
        assert rc == hip.DD_OK and counts[1] == nf - 1 and np.array_equal(flags[:nf - 1], want[3][:-1])
        # one entry too few: the entry's error, the list full and nothing past it
        rc, counts, _, flags = dev_bits(hip, sym, cap_flags=nf - 1)
        assert rc == hip.DD_ERR_INVALID and "flag list too small" in hip.last_error() and counts.tolist() == [n, nf]
        assert np.array_equal(flags[:nf - 1], want[3][:-1]) and np.all(flags[nf - 1:] == SENT_I)
        bs = fsk.bit_stream(hip.DevArray.from_host(sym))
        assert len(bs) == n and np.array_equal(bs.flags.to_host(), want[3]) and np.array_equal(bs.marks.to_host(), want[2])
        assert np.array_equal(bs.sgn.to_host(), want[0]) and bs.mean.n == n


def test_bits_bad_arguments(hip):
    d = hip.DevArray.from_host(np.ones(16))
    o = [hip.DevArray.from_host(np.zeros(16, dtype=np.int8)) for _ in range(3)]
    fl = hip.DevArray.from_host(np.zeros(16, dtype=np.int64))
    counts = np.zeros(2, dtype=np.int64)
    pc = counts.ctypes.data_as(C.POINTER(C.c_int64))
    fn = hip.lib().dd_fsk_bits
    good = [d.ptr, 16, o[0].ptr, o[1].ptr, o[2].ptr, fl.ptr, 16, pc]
    assert fn(*good, None) == hip.DD_OK
    assert fn(None, 0, None, None, None, None, 0, pc, None) == hip.DD_OK and counts.tolist() == [0, 0]
    for i, v in ((0, None), (1, -1), (2, None), (3, None), (4, None), (5, None), (6, -1), (7, None)):
        args = list(good)
        args[i] = v
        assert fn(*args, None) == hip.DD_ERR_INVALID, i


# ------------------------------------------------------------------------------------------------------------------ decode_fsk9600
@pytest.fixture(scope="module")
def decoded(hip):
    """name -> (raw, fs, offset, the good frames' bytes, the decoder after its decode), each recording decoded once"""
    from directdemod_amd import decode_fsk9600, source
    cache = {}

    def get(name):
        if name not in cache:
            raw, fs, offset, good = fk.recording(name)
            obj = decode_fsk9600.decode_fsk9600(source.IQarray(raw, fs), offset)
            obj.getFrames
            cache[name] = (raw, fs, offset, good, obj)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(fk.RECORDINGS))
def test_decode_end_to_end(hip, decoded, name):
    """0.45 s, four frames with the third's CRC corrupted, 100 ppm baud error, the second recording inverted and 12.5 kHz off
    centre: exactly the three good frames, in order"""
    from directdemod_amd import decode_afsk1200
    raw, fs, offset, good, obj = decoded(name)
    frames = obj.getFrames
    assert [f["raw"] for f in frames] == good and obj.useful == 1
    for f, g in zip(frames, good):
        dst, src, path, control, pid, text = decode_afsk1200._fields(g)
        assert (f["destination"], f["source"], f["path"], f["control"], f["pid"], f["info"]) == (dst, src, path, control, pid, text)
        assert f["nbytes"] == len(g) + 2 and (control, pid) == ("0x3", "0xf0")
    bits, info = obj.getBits, obj.bitInfo
    flags = [f["start"] for f in frames]
    assert flags == sorted(flags) and all(tuple(bits[s:s + 8]) == (0, 1, 1, 1, 1, 1, 1, 0) for s in flags)
    assert [f["flag"] for f in frames] == sorted(f["flag"] for f in frames) and frames[-1]["flag"] < info["pairs"]
    assert info["symbols"] == len(bits) and info["frames"] == 3 and info["pairs"] == info["flags"] - 1
    P = fs / int(fs / 48000) / 9600
    # the mean period: 100 ppm of baud error, up to a symbol of pull-in and a sample of rounding at either end over the span
    assert obj.audioRate == fs / int(fs / 48000) and abs(info["period"] / P - 1.0) < 1e-4 + (P + 2) / (P * info["symbols"])
    assert list(obj.timings) == ["front_end", "walk", "bits", "frames"] and all(v >= 0.0 for v in obj.timings.values())
    assert obj.getFrames == frames                         # cached: the same dicts, no second decode
    assert list(obj.timings) == ["front_end", "walk", "bits", "frames"]


@pytest.mark.parametrize("name", sorted(fk.RECORDINGS))
def test_stages_agree_with_the_restatement_on_the_device_s_audio(hip, decoded, name):
    raw, fs, offset, good, obj = decoded(name)
    audio = obj.audio().to_host()
    assert audio.dtype == np.float64 and abs(len(audio) - len(raw) / int(fs / 48000)) <= 1
    _, ref, _ = fk.walk_host(audio, 0, fk.start_state(), fk.params(obj.audioRate / 9600))
    sym, sidx = obj.getSymbols
    assert np.array_equal(_bits(sym), _bits(ref["sym"])) and np.array_equal(sidx, ref["sidx"])
    assert np.array_equal(obj.getBits, fk.bits_host(ref["sym"])[1])


@pytest.mark.parametrize("name", sorted(fk.RECORDINGS))
def test_from_audio_gives_the_same_frames(hip, decoded, name):
    from directdemod_amd import decode_fsk9600
    raw, fs, offset, good, obj = decoded(name)
    for audio in (obj.audio(), obj.audio().to_host()):
        again = decode_fsk9600.decode_fsk9600.fromAudio(audio, obj.audioRate)
        assert again.getFrames == obj.getFrames and again.useful == 1 and again.bitInfo == obj.bitInfo
        assert np.array_equal(again.getBits, obj.getBits)


def test_noise_only_and_bad_arguments(hip):
    from directdemod_amd import decode_fsk9600, source
    import directdemod_amd
    obj = decode_fsk9600.decode_fsk9600(source.IQarray(fk.noise_recording(), 960000), 0)
    assert obj.useful == 0 and obj.getFrames == [] and obj.useful == 0
    assert obj.bitInfo["frames"] == 0 and obj.bitInfo["symbols"] > 500
    src = source.IQarray(np.full((100, 2), 127, dtype=np.uint8), 2048000)
    for kw in (dict(bw=9600), dict(bw=1000000), dict(bw=48000, baud=300)):           # P = 1.002, P = 106.7, P = 162.5
        with pytest.raises(ValueError, match="S/s"):
            decode_fsk9600.decode_fsk9600(src, 0, **kw)
    with pytest.raises(ValueError):
        decode_fsk9600.decode_fsk9600.fromAudio(np.zeros(10), 9600.0)
    empty = decode_fsk9600.decode_fsk9600.fromAudio(np.zeros(0), 48000.0)
    assert empty.getFrames == [] and empty.bitInfo["period"] is None and len(empty.getBits) == 0
    assert "decode_fsk9600" in directdemod_amd.__all__ and "fsk" in directdemod_amd.__all__
