"""The OQPSK symbol walk of DESIGN.md section 4.19 (dd_oqpsk.h) restated sample by sample in Python floats, for
tests/test_oqpsk_host.py and tests/test_gpu_oqpsk.py: `walk_host` with its branch counters, the seeded integer-arithmetic `signal`
and the named `CASES`, the length and cut runs, and a recording builder on top of _lrpt / _lrpt_modes (`recording`, `front_end`).
No run skipping, no tiles: `timing += 1` once per sample.  Every operation is one IEEE float64 operation of + - * / sqrt floor, in
the order the design text writes out, so the device is compared with np.array_equal."""
import math

import numpy as np

import _lrpt
from directdemod_amd import lrpt

FS = 2048000
TILE = 1024                       # samples the device stages per step
N = 1024                          # phasor table entries
K = 6.283185307179586 / 1024.0    # 2 pi / N
C3, C4, C5 = 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0
TWO_PI = 6.283185307179586
BW = 0.008727                     # the Costas loop's bandwidth, rad per symbol, unlocked
CAP = 200.0                       # agc.adjust's gain limit (dd_met_agc_cap<200>)
AMEAN0 = 3.0
RATES = {72000: (9, 256), 80000: (5, 128)}        # symbols per sample as a fraction

FLOAT_FIELDS = ("timing", "dc_re", "dc_im", "amean", "u", "freq", "pmean", "alpha", "beta", "i_k", "i_prev", "i_mid", "q_prev",
                "q_mid", "e_q")
INT_FIELDS = ("lock", "ctr", "aidx", "seen_a", "overflow")
ARRAYS = ("bidx", "aidx", "sym", "uf")
COUNTERS = ("b_events", "a_events", "b_before_a", "cap_taken", "cap_not_taken", "hyp_high", "hyp_low", "hyp_table", "err_clamped",
            "locked", "unlocked", "u_wrapped")

# Symbols after which every hard decision of the walk equals the sent bit, in every recording of RECORDINGS (0.9 s, amplitude 40,
# sigma 4, 300 Hz carrier).  Measured with this restatement, the last wrong decision fell at symbol 6 111 (72k_s0), 6 660 (72k_s1),
# 5 971 (80k_s0) and 7 580 (80k_s1; 7 285 with the interleaver's data), and at most there at five more carrier phases per rate;
# the prototype the design was written from needed up to 16 000.  10 000 leaves a third on top of the measured figure: the
# device's front end (fixed-point NCO, block-parallel filter) differs from front_end below in its last bits.
ACQ = 10000


def table():
    """the phasor table: (cos, sin)(2 pi i / N), float64[N, 2], by NumPy"""
    a = 2.0 * np.pi * np.arange(N) / N
    return np.stack((np.cos(a), np.sin(a)), axis=1)


def _alpha_beta(damping, bw):
    denom = (1.0 + 2.0 * damping * bw + bw * bw)
    return (4 * damping * bw) / denom, (4 * bw * bw) / denom


def params(symbol_rate):
    """the walk's constants: P, the loop gains in turns, unlocked (`u`) and locked (`l`, half the bandwidth), the tanh table"""
    P = FS / symbol_rate
    au, bu = _alpha_beta(0.70710678118, BW)
    al, bl = _alpha_beta(0.70710678118, BW / 2.0)
    return dict(P=P, alpha_u=au / TWO_PI, beta_u=bu / TWO_PI, alpha_l=al / TWO_PI, beta_l=bl / TWO_PI,
                hyp=[np.tanh(i - 128) for i in range(256)])


def params_array(p):
    """`params` as the 263 doubles the device entry point takes (DDMeteorParams)"""
    return np.array([p["P"], p["P"] / 2, (p["P"] / 2) + 1, p["alpha_u"], p["beta_u"], p["alpha_l"], p["beta_l"]] + list(p["hyp"]),
                    dtype=np.float64)


def start_state(symbol_rate, **over):
    """the 20 fields of oqpsk.STATE at the start of a recording, with `over` on top; lock = 1 takes the locked gains unless stated"""
    p = params(symbol_rate)
    s = dict.fromkeys(FLOAT_FIELDS, 0.0)
    s.update(dict.fromkeys(INT_FIELDS, 0))
    s.update(amean=AMEAN0, freq=0.001 / TWO_PI, pmean=1.0)
    s.update(over)
    if "alpha" not in over:
        s["alpha"], s["beta"] = (p["alpha_l"], p["beta_l"]) if s["lock"] else (p["alpha_u"], p["beta_u"])
    return s


def state_struct(s, dtype):
    st = np.zeros(1, dtype=dtype)
    for f in FLOAT_FIELDS + INT_FIELDS:
        st[f] = s[f]
    return st


def phasor(u, tab):
    """(cos, sin)(2 pi u) for u in [0, 1): table entry i = int(u N), rotated by d = (u N - i) (2 pi / N) through the two polynomials"""
    t = u * 1024.0
    i = int(min(t, 1023.0)) if t >= 0.0 else 0
    d = (t - i) * K
    d2 = d * d
    pc = 1.0 - d2 * (0.5 - d2 * C4)
    ps = d * (1.0 - d2 * (C3 - d2 * C5))
    tc, ts = tab[i]
    return tc * pc - ts * ps, ts * pc + tc * ps


def frac(t):
    """t - floor(t), 0 where that is not below 1 (a tiny negative t, or no number)"""
    if not math.isfinite(t):
        return 0.0
    f = t - math.floor(t)
    return f if f < 1.0 else 0.0


def walk_host(x, base, state, prm, tab=None):
    """The walk over the samples x (complex128) = samples base .. of the recording, from `state` (not modified) -> (state after,
    per-symbol arrays bidx, aidx (int64), sym (complex128), uf (float64[n, 2] = u, freq after the symbol's step), counters).
    `overflow` is carried as it is: this walk has no capacity."""
    tab = (table() if tab is None else np.asarray(tab)).tolist()
    P, hyp_tab = prm["P"], prm["hyp"]
    halfP, halfP1 = P / 2, (P / 2) + 1
    s = dict(state)
    cnt = dict.fromkeys(COUNTERS, 0)
    cnt["pmean_margin"] = float("inf")
    out = dict(bidx=[], aidx=[], sym=[], uf=[])
    xr, xi = np.asarray(x).real.tolist(), np.asarray(x).imag.tolist()

    def adjust(re, im):
        s["dc_re"] = (s["dc_re"] * 1048575.0 + re) * (1.0 / 1048576.0)
        s["dc_im"] = (s["dc_im"] * 1048575.0 + im) * (1.0 / 1048576.0)
        re, im = re - s["dc_re"], im - s["dc_im"]
        s["amean"] = (s["amean"] * 65535.0 + math.sqrt(re * re + im * im)) / 65536.0
        if 180.0 / s["amean"] > CAP:
            cnt["cap_taken"] += 1
            return re * CAP, im * CAP
        cnt["cap_not_taken"] += 1
        inv = 1.0 / s["amean"]
        return (re * 180.0) * inv, (im * 180.0) * inv

    def hyp(v):
        if v > 127:
            cnt["hyp_high"] += 1
            return 1.0
        if v < -128:
            cnt["hyp_low"] += 1
            return -1.0
        cnt["hyp_table"] += 1
        return hyp_tab[int(v + 128) if v == v else 0]

    def derotated(j):
        ar, ai = adjust(xr[j], xi[j])
        c, sn = phasor(s["u"], tab)
        return ar * c + ai * sn, ai * c - ar * sn              # a * (cos, -sin)

    def wrap(t):
        f = frac(t)
        if math.isfinite(t) and math.floor(t) != 0.0:
            cnt["u_wrapped"] += 1
        return f

    timing = s["timing"]
    for j in range(len(xr)):
        if timing >= halfP and timing < halfP1:
            re, im = derotated(j)
            s["i_mid"] = re
            cnt["b_events"] += 1
            if s["seen_a"]:
                q = im
                s["e_q"] = (q - s["q_prev"]) * s["q_mid"]
                s["q_prev"] = q
                ik = s["i_k"]
                err = (q * hyp(ik) - ik * hyp(q)) / 255.0
                s["pmean"] = (s["pmean"] * 39999.0 + abs(err)) / 40000.0
                if err > 1.0:
                    err = 1.0
                    cnt["err_clamped"] += 1
                elif err < -1.0:
                    err = -1.0
                    cnt["err_clamped"] += 1
                s["u"] = wrap((s["u"] + s["freq"] * 0.5) + s["alpha"] * err)
                s["freq"] = s["freq"] + s["beta"] * err
                if not s["lock"] and s["pmean"] < 0.2:
                    s["alpha"], s["beta"], s["lock"] = prm["alpha_l"], prm["beta_l"], 1
                    cnt["locked"] += 1
                elif s["lock"] and s["pmean"] > 0.5:
                    s["alpha"], s["beta"], s["lock"] = prm["alpha_u"], prm["beta_u"], 0
                    cnt["unlocked"] += 1
                cnt["pmean_margin"] = min(cnt["pmean_margin"], abs(s["pmean"] - 0.2), abs(s["pmean"] - 0.5))
                out["bidx"].append(base + j)
                out["aidx"].append(s["aidx"])
                out["sym"].append(complex(ik, q))
                out["uf"].append((s["u"], s["freq"]))
                s["ctr"] += 1
            else:
                cnt["b_before_a"] += 1
        elif timing >= P:
            re, im = derotated(j)
            s["i_k"], s["q_mid"] = re, im
            e_i = (re - s["i_prev"]) * s["i_mid"]
            s["i_prev"] = re
            timing = (timing - P) + ((e_i + s["e_q"]) * P) / 2000000.0
            s["e_q"] = 0.0
            s["u"] = wrap(s["u"] + s["freq"] * 0.5)
            s["seen_a"], s["aidx"] = 1, base + j
            cnt["a_events"] += 1
        timing += 1
    s["timing"] = timing
    arrays = dict(bidx=np.array(out["bidx"], dtype=np.int64), aidx=np.array(out["aidx"], dtype=np.int64),
                  sym=np.array(out["sym"], dtype=np.complex128), uf=np.array(out["uf"], dtype=np.float64).reshape(-1, 2))
    return s, arrays, cnt


# ---------------------------------------------------------------------------------------------------------------- exact inputs
def rails(t, num, den):
    """the symbol index of the I rail and of the Q rail (half a period late) at the sample times t"""
    t = np.asarray(t, dtype=np.int64)
    return t * num // den, (2 * t * num - den) // (2 * den)


def signal(symbol_rate, n, seed, amp=40.0, noise=8):
    """n samples of rectangular-pulse OQPSK at 2.048 MS/s, complex128, every component a multiple of 1/8: I(t) + j Q(t - T/2) with
    amplitude `amp` per rail and uniform noise of up to `noise` eighths.  PCG64 integers and integer arithmetic up to the final
    division by 8: the same samples on every machine.  (The Q rail's index is -1 during the first half period: the last bit.)"""
    num, den = RATES[symbol_rate]
    rng = np.random.Generator(np.random.PCG64(seed))
    nsym = n * num // den + 2
    bits = rng.integers(0, 2, size=(nsym, 2))
    nz = rng.integers(-noise, noise + 1, size=(n, 2))
    ki, kq = rails(np.arange(n), num, den)
    a8 = int(round(amp * 8))
    assert a8 == amp * 8
    vi = a8 * (2 * bits[ki, 0] - 1) + nz[:, 0]
    vq = a8 * (2 * bits[kq, 1] - 1) + nz[:, 1]
    return (vi / 8.0) + 1j * (vq / 8.0)


# The walk's named cases: symbol rate, `signal` arguments, start state overrides, and the counters each is there for
CASES = {
    "default_72k": dict(rate=72000, signal=dict(n=8192, seed=1, amp=3.0, noise=24),
                        reaches=("b_events", "a_events", "b_before_a", "cap_not_taken", "hyp_high", "hyp_low", "hyp_table",
                                 "err_clamped")),
    "default_80k": dict(rate=80000, signal=dict(n=8192, seed=2, amp=3.0, noise=24),
                        reaches=("b_events", "a_events", "cap_not_taken", "hyp_table")),
    "started": dict(rate=72000, signal=dict(n=8192, seed=3, amp=1.0, noise=3), state=dict(pmean=0.49999, lock=1, amean=0.8995, seen_a=1, u=0.125),
                    reaches=("unlocked", "cap_taken", "cap_not_taken", "err_clamped")),
    "locking": dict(rate=80000, signal=dict(n=8192, seed=5, amp=1.0, noise=2), state=dict(pmean=0.20003, seen_a=1),
                    reaches=("locked", "hyp_table")),
    # a frequency of 0.3 turns per symbol: u passes 1 every few symbols
    "u_wraps": dict(rate=72000, signal=dict(n=4096, seed=6, amp=3.0, noise=24), state=dict(freq=0.3, u=0.9),
                    reaches=("u_wrapped",)),
    # timing far above P: an A event at every sample until it has come down, and no B between them
    "a_run": dict(rate=72000, signal=dict(n=3073, seed=7, amp=3.0, noise=24), state=dict(timing=7.0e4), reaches=("a_events",)),
}


def case(name):
    """(symbol rate, x, start state) of a named case"""
    c = CASES[name]
    return c["rate"], signal(c["rate"], **c["signal"]), start_state(c["rate"], **c.get("state", {}))


LENGTHS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 1)
LENGTH_SIGNAL = dict(n=LENGTHS[-1], seed=10, amp=3.0, noise=24)


def length_runs(symbol_rate):
    """[(n, start timing, None or (event kind "A" / "B", the sample it falls on))]: each length from timing 0 and from start timings
    that put the first A or the first B on the last sample of a tile and on the first sample of the next (a length of one tile or
    less: on its last sample)"""
    P = FS / symbol_rate
    runs = []
    for n in LENGTHS:
        runs.append((n, 0.0, None))
        edge = ((n - 1) // TILE) * TILE
        for j in ([edge - 1, edge] if edge else [n - 1]):
            runs.append((n, P + 0.25 - j, ("A", j)))
            runs.append((n, P / 2 + 0.25 - j, ("B", j)))
    return runs


# ------------------------------------------------------------------------------------------------------------------ recordings
def oqpsk_iq(code, symbol_rate, n, carrier, phase, amp, sigma, rng):
    """code bits uint8[nsym, 2] -> uint8[n, 2] IQ pairs centred on 127.5: rectangular OQPSK pulses, the Q rail half a period late,
    on a carrier, with Gaussian noise"""
    num, den = RATES[symbol_rate]
    ki, kq = rails(np.arange(n), num, den)
    lv = 2.0 * code.astype(np.float64) - 1.0
    x = amp * (lv[ki, 0] + 1j * lv[np.maximum(kq, 0), 1])
    t = np.arange(n, dtype=np.int64)
    x = x * np.exp(1j * (2.0 * np.pi * carrier * t / FS + phase))
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.stack((x.real, x.imag), axis=1) + 127.5
    return np.clip(np.rint(iq), 0, 255).astype(np.uint8)


def recording(seed, symbol_rate, seconds=0.9, carrier=300.0, phase=0.0, amp=40.0, sigma=4.0, interleaved=False, branches=36, delay=8):
    """-> dict(raw uint8[n, 2], code uint8[nsym, 2] = the bits sent per symbol (I rail, Q rail), bodies, starts): frames ->
    NRZ-M -> the convolutional code -> (interleaver and markers) -> OQPSK.  starts[i] = the sent symbol of frame i's marker, counted
    in the deinterleaved stream when interleaved.  The stream begins at a random bit of the first frame."""
    num, den = RATES[symbol_rate]
    n = int(round(seconds * FS))
    nsym = n * num // den + 2
    rng = np.random.Generator(np.random.PCG64(seed))
    span = branches * delay * (branches - 1) if interleaved else 0
    nframes = (nsym * (36 if interleaved else 40) // 40) // lrpt.FRAME_BITS + 2
    bodies = rng.integers(0, 256, size=(nframes, lrpt.BODY_BYTES), dtype=np.uint8)
    start = int(rng.integers(0, lrpt.FRAME_BITS))
    code = lrpt.encode(lrpt.nrzm_encode(_lrpt.frames_bits(bodies)))[2 * start:]
    if interleaved:
        code = lrpt.add_markers_np(lrpt.interleave_np(code, branches, delay))
    assert len(code) >= 2 * nsym, (len(code), nsym)
    code = code[:2 * nsym].reshape(-1, 2)
    raw = oqpsk_iq(code, symbol_rate, n, carrier, phase, amp, sigma, rng)
    return dict(raw=raw, code=code, bodies=bodies, starts=[lrpt.FRAME_BITS * i - start for i in range(nframes)], span=span,
                symbol_rate=symbol_rate, carrier=carrier)


def front_end(raw, offset, symbol_rate):
    """the decoder's front end in NumPy / SciPy float64: mix by exp(-2 pi j offset k / fs), butter(6, 70 kHz * rate / 72000)"""
    import scipy.signal as signal
    x = (raw[:, 0].astype(np.float64) - 127.5) + 1j * (raw[:, 1].astype(np.float64) - 127.5)
    x = x * np.exp(-2.0j * np.pi * offset * np.arange(len(x)) / FS)
    b, a = signal.butter(6, (70000.0 * symbol_rate / 72000.0) / (0.5 * FS), btype="lowpass")
    return signal.lfilter(b, a, x)


DELAY = {72000: 18, 80000: 16}       # the low-pass filter's group delay in samples (scipy.signal.group_delay at 0 Hz: 17.9, 16.1)


def decisions(arr, code, symbol_rate):
    """The walk's hard decisions against the sent bits: the I rail of symbol k was sampled at aidx[k], the Q rail at bidx[k], which
    the filter delays by DELAY samples, and there the sent rails' symbol indices are `rails`.  Under each of the four carrier rotations the received rails are the sent rails with
    signs, exchanged for the odd ones -> (the rotation with the most agreement, bool[nsym, 2] = decision equals sent bit)"""
    num, den = RATES[symbol_rate]
    ai, aq = rails(np.maximum(arr["aidx"] - DELAY[symbol_rate], 0), num, den)
    bi, bq = rails(np.maximum(arr["bidx"] - DELAY[symbol_rate], 0), num, den)
    hi, hq = arr["sym"].real > 0, arr["sym"].imag > 0
    c = code.astype(bool)
    best = None
    for rot, (ri, rq) in enumerate(((c[ai, 0], c[np.maximum(bq, 0), 1]), (~c[np.maximum(aq, 0), 1], c[bi, 0]),
                                    (~c[ai, 0], ~c[np.maximum(bq, 0), 1]), (c[np.maximum(aq, 0), 1], ~c[bi, 0]))):
        ok = np.stack((hi == ri, hq == rq), axis=1)
        if best is None or ok.sum() > best[1].sum():
            best = (rot, ok)
    return best


# 0.9 s recordings: per symbol rate two carrier phases, chosen with this restatement so that both lock outcomes occur (rotation
# 0 / 180 degrees: stagger 0; 90 / 270 degrees: the rails one symbol apart, stagger -1)
RECORDINGS = {
    "72k_s0": dict(seed=41, symbol_rate=72000, phase=0.0),
    "72k_s1": dict(seed=41, symbol_rate=72000, phase=1.6),
    "80k_s0": dict(seed=42, symbol_rate=80000, phase=0.0),
    "80k_s1": dict(seed=42, symbol_rate=80000, phase=1.6),
}


def expected_frames(rec, aidx, acq=None):
    """The sent frames that lie whole in what the walk delivered past symbol `acq` (ACQ), as indices into rec["bodies"].  Walk symbol
    k carries the sent symbol rails(aidx[k] - DELAY) (one more or less at a 90 degree lock); a frame counts when every sent symbol
    that holds one of its bits -- through the interleaver, when there is one -- lies two symbols inside that range."""
    acq = ACQ if acq is None else acq
    num, den = RATES[rec["symbol_rate"]]
    if len(aidx) <= acq:
        return []
    first, last = (int(rails(max(int(aidx[k]) - DELAY[rec["symbol_rate"]], 0), num, den)[0]) for k in (acq, len(aidx) - 1))
    out = []
    for i, st in enumerate(rec["starts"]):
        if rec["span"]:
            lo = (2 * st // 72) * 40
            hi = ((2 * (st + lrpt.FRAME_BITS) + rec["span"]) // 72 + 1) * 40
        else:
            lo, hi = st, st + lrpt.FRAME_BITS
        if st >= 0 and lo >= first + 2 and hi <= last - 2:
            out.append(i)
    return out


def frames_found(frames, info, bodies, expected):
    """every expected body is among the decoded frames, once, in order, with no marker bit in error -> their rows"""
    rows = []
    for i in expected:
        hit = [r for r in range(len(frames)) if np.array_equal(frames[r], bodies[i])]
        assert len(hit) == 1, (i, hit)
        assert int(info["asm_errors"][hit[0]]) == 0, (i, info[hit[0]])
        rows.append(hit[0])
    assert rows == sorted(rows)
    return rows
