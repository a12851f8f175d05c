"""Restatements of the symbol walk (dd_symbol_walk.h) shared by the Meteor-M2 and Funcube tests: the device's run skipping (`skip`), and a
sample-by-sample float64 walk from the design text with its seeded inputs and named cases (`walk_host`, `signal`, `CASES`)."""
import hashlib
import math

import numpy as np


def skip(t, T, room):
    """dd_met_skip (dd_symbol_walk.h): how many plain timing += 1 samples the walk takes at once"""
    _, e = math.frexp(t)
    U2 = math.ldexp(1.0, e + 1)
    est = min(T - t, U2 - 1.0 - t)
    m = 0 if est <= 0 else int(min(math.ceil(est), room))
    while m > 0 and not (t + (m - 1) < T and t + m < U2):
        m -= 1
    while m < room and t + m < T and t + (m + 1) < U2:
        m += 1
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# A sample-by-sample float64 restatement of the walk (the reference's agc.adjust, costas.loop and Gardner
# test), its inputs and its cases, for tests/test_symbolwalk_host.py and tests/test_gpu_symbolwalk.py.  No skip(), no tiles, no
# waves: `timing += 1` once per sample.  NumPy's complex arithmetic, which the reference runs on, is written component by component:
# a complex times a real r is (re * r, im * r), a complex over a real r is Smith's quotient (re * (1 / r), im * (1 / r)).
FS = 2048000
TILE = 1024                       # samples the device stages per step; here only the unit of two branch counters
TWO_PI = 6.283185307179586        # 2 * np.pi

# cap: agc.adjust's gain limit; amean0: agc.mean at start; bw: the Costas loop's bandwidth, unlocked; rate = symbols per sample as a
# fraction; qpsk: the cross-term error (else imag * hyp(real))
POLICIES = {
    "meteor": dict(symbol_rate=72000, rate=(9, 256), cap=200.0, amean0=3.0, bw=0.008727, qpsk=True),
    "funcube": dict(symbol_rate=12000, rate=(3, 512), cap=20.0, amean0=180.0, bw=0.05235833333 * 6, qpsk=False),
}
FLOAT_FIELDS = ("timing", "b_re", "b_im", "c_re", "c_im", "dc_re", "dc_im", "amean", "freq", "phase", "pmean", "alpha", "beta")
INT_FIELDS = ("lock", "ctr", "bidx", "overflow")
TIMING_FIELDS = ("timing", "b_re", "b_im", "c_re", "c_im", "dc_re", "dc_im", "amean", "bidx", "overflow")    # carried by the timing chain
COUNTERS = ("b_events", "a_events", "cap_taken", "cap_not_taken", "locked", "unlocked", "hyp_high", "hyp_low", "hyp_table",
            "err_clamped", "timing_below_1", "tiles_empty", "tiles_full")


def _alpha_beta(damping, bw):
    denom = (1.0 + 2.0 * damping * bw + bw * bw)
    return (4 * damping * bw) / denom, (4 * bw * bw) / denom


def params(policy):
    """the walk's constants: symbolPeriod P, costas.compAlphaBeta(damping, bw) unlocked (`u`) and (damping, bw / 2) locked (`l`),
    costas.hypstore"""
    pol = POLICIES[policy]
    P = FS / pol["symbol_rate"]
    au, bu = _alpha_beta(0.70710678118, pol["bw"])
    al, bl = _alpha_beta(0.70710678118, pol["bw"] / 2.0)
    return dict(P=P, alpha_u=au, beta_u=bu, alpha_l=al, beta_l=bl, hyp=[np.tanh(i - 128) for i in range(256)])


def params_array(p):
    """`params` as the 263 doubles the device entry points take (DDMeteorParams)"""
    return np.array([p["P"], p["P"] / 2, (p["P"] / 2) + 1, p["alpha_u"], p["beta_u"], p["alpha_l"], p["beta_l"]] + list(p["hyp"]),
                    dtype=np.float64)


def start_state(policy, **over):
    """the 17 fields of symbolsync._STATE as the reference's objects start (timing, B, C, dc 0; agc.mean; costas.freq 0.001, mean 1.0,
    unlocked), with `over` on top; lock = 1 takes the locked alpha / beta unless `over` states them"""
    p = params(policy)
    s = dict.fromkeys(FLOAT_FIELDS, 0.0)
    s.update(dict.fromkeys(INT_FIELDS, 0))
    s.update(amean=POLICIES[policy]["amean0"], freq=0.001, pmean=1.0)
    s.update(over)
    if "alpha" not in over:
        s["alpha"], s["beta"] = (p["alpha_l"], p["beta_l"]) if s["lock"] else (p["alpha_u"], p["beta_u"])
    return s


def state_struct(s, dtype):
    """a state dict as one record of `dtype` (symbolsync._STATE)"""
    st = np.zeros(1, dtype=dtype)
    for f in FLOAT_FIELDS + INT_FIELDS:
        st[f] = s[f]
    return st


def state_dict(st):
    r = st.reshape(-1)[0]
    return {**{f: float(r[f]) for f in FLOAT_FIELDS}, **{f: int(r[f]) for f in INT_FIELDS}}


def walk_host(x, base, state, params, policy, magnitude="sqrt"):
    """The walk over the samples x (complex128), which are samples base .. base + len(x) - 1 of the recording, from `state` (the 17
    fields; not modified).  -> (state after, per-symbol arrays bidx, aidx (int64), agc, ph, sym (complex128), pf (float64[n, 2] =
    phase, freq after the step), branch counters).  magnitude: "pow" takes agc.adjust's magnitude as np.float64 ** 0.5 (the
    reference), "sqrt" as math.sqrt (the device).  The counters also carry pmean_margin, the least distance of costas.mean from a
    lock threshold (0.2, 0.5) after any step.  `overflow` is carried as it is: this walk has no capacity."""
    pol = POLICIES[policy]
    cap, qpsk = pol["cap"], pol["qpsk"]
    P, hyp_tab = params["P"], params["hyp"]
    halfP, halfP1 = P / 2, (P / 2) + 1
    s = dict(state)
    cnt = dict.fromkeys(COUNTERS, 0)
    cnt["pmean_margin"] = float("inf")
    out = dict(bidx=[], aidx=[], agc=[], ph=[], sym=[], pf=[])
    per_tile = [0] * ((len(x) + TILE - 1) // TILE)

    def adjust(v):
        # dc: a moving average over 2^20 calls, mean: of the magnitude over 2^16
        s["dc_re"] = (s["dc_re"] * 1048575.0 + v.real) * (1.0 / 1048576.0)
        s["dc_im"] = (s["dc_im"] * 1048575.0 + v.imag) * (1.0 / 1048576.0)
        re, im = v.real - s["dc_re"], v.imag - s["dc_im"]
        sq = re * re + im * im
        mag = math.sqrt(sq) if magnitude == "sqrt" else float(np.float64(sq) ** 0.5)
        s["amean"] = (s["amean"] * 65535.0 + mag) / 65536.0
        if 180.0 / s["amean"] > cap:
            cnt["cap_taken"] += 1
            return re * cap, im * cap
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
        return hyp_tab[int(v + 128)]

    def loop(ar, ai):
        o_re, o_im = math.cos(s["phase"]), -math.sin(s["phase"])           # exp(-1j * phase)
        cr, ci = ar * o_re - ai * o_im, ar * o_im + ai * o_re
        err = (ci * hyp(cr) - cr * hyp(ci)) / 255.0 if qpsk else ci * hyp(cr) / 255.0
        s["pmean"] = (s["pmean"] * 39999.0 + abs(err)) / 40000.0
        if err > 1:
            err = 1.0
            cnt["err_clamped"] += 1
        elif err < -1:
            err = -1.0
            cnt["err_clamped"] += 1
        s["phase"] = math.fmod(s["phase"] + s["freq"] + s["alpha"] * err, TWO_PI)
        s["freq"] = s["freq"] + s["beta"] * err
        if not s["lock"] and s["pmean"] < 0.2:
            s["alpha"], s["beta"], s["lock"] = params["alpha_l"], params["beta_l"], 1
            cnt["locked"] += 1
        elif s["lock"] and s["pmean"] > 0.5:
            s["alpha"], s["beta"], s["lock"] = params["alpha_u"], params["beta_u"], 0
            cnt["unlocked"] += 1
        cnt["pmean_margin"] = min(cnt["pmean_margin"], abs(s["pmean"] - 0.2), abs(s["pmean"] - 0.5))
        return (o_re, o_im), (cr, ci)

    timing = s["timing"]
    for j in range(len(x)):
        event = False
        if timing >= halfP and timing < halfP1:
            s["b_re"], s["b_im"] = adjust(x[j])
            s["bidx"] = base + j
            cnt["b_events"] += 1
            event = True
        elif timing >= P:
            ar, ai = adjust(x[j])
            timing -= P
            resync = (ai - s["c_im"]) * s["b_im"]
            timing += resync * P / 2000000.0
            s["c_re"], s["c_im"] = ar, ai
            o, c = loop(ar, ai)
            out["bidx"].append(s["bidx"])
            out["aidx"].append(base + j)
            out["agc"].append(complex(ar, ai))
            out["ph"].append(complex(*o))
            out["sym"].append(complex(*c))
            out["pf"].append((s["phase"], s["freq"]))
            s["ctr"] += 1
            cnt["a_events"] += 1
            per_tile[j // TILE] += 1
            event = True
        timing += 1
        if event and timing < 1.0:
            cnt["timing_below_1"] += 1
    s["timing"] = timing
    cnt["tiles_empty"] = sum(1 for c in per_tile if c == 0)
    cnt["tiles_full"] = sum(1 for i, c in enumerate(per_tile) if c == TILE)
    arrays = dict(bidx=np.array(out["bidx"], dtype=np.int64), aidx=np.array(out["aidx"], dtype=np.int64),
                  agc=np.array(out["agc"], dtype=np.complex128), ph=np.array(out["ph"], dtype=np.complex128),
                  sym=np.array(out["sym"], dtype=np.complex128), pf=np.array(out["pf"], dtype=np.float64).reshape(-1, 2))
    return s, arrays, cnt


def signal(policy, n, seed, amp=40.0, noise=8, quiet=0, quiet_noise=1):
    """n samples of rectangular-pulse QPSK (Meteor) or BPSK on the diagonal (Funcube: the Gardner error reads the imaginary part) at
    the policy's symbol rate and 2.048 MS/s, complex128, every component a multiple of 1/8: amplitude `amp` per component, uniform
    noise of up to `noise` eighths; the first `quiet` samples carry no symbols and noise of up to `quiet_noise` eighths.  Bits and
    noise are PCG64 integers and the arithmetic is integer up to the final division by 8, so the samples are the same on every
    machine."""
    num, den = POLICIES[policy]["rate"]
    rng = np.random.Generator(np.random.PCG64(seed))
    nsym = n * num // den + 2
    bits = rng.integers(0, 2, size=(nsym, 2))
    nz = rng.integers(-noise, noise + 1, size=(n, 2))
    t = np.arange(n, dtype=np.int64)
    b = bits[t * num // den]
    if not POLICIES[policy]["qpsk"]:
        b = b[:, :1].repeat(2, axis=1)
    a8 = int(round(amp * 8))
    assert a8 == amp * 8
    v = a8 * (2 * b - 1) + nz
    if quiet:
        v[:quiet] = np.clip(nz[:quiet], -quiet_noise, quiet_noise)
    return (v[:, 0] / 8.0) + 1j * (v[:, 1] / 8.0)


def sha256(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype=np.complex128).tobytes()).hexdigest()


# The walk's cases: input (`signal` arguments) and start state (`start_state` overrides), and the branch counters each is there
# for (`reaches`: all of them above zero, checked by tests/test_symbolwalk_host.py).  "default" and "started" of each policy are the
# inputs of tests/golden/symbolwalk_*.npz, the reference's own loop over them (tools/gen_golden.py --symbolwalk).
CASES = {
    "meteor_default": dict(policy="meteor", fixture=True, signal=dict(n=16384, seed=1, amp=3.0, noise=24),
                           reaches=("b_events", "a_events", "cap_not_taken", "hyp_high", "hyp_low", "hyp_table", "err_clamped",
                                    "timing_below_1")),
    "meteor_started": dict(policy="meteor", fixture=True, signal=dict(n=16384, seed=2, amp=40.0),
                           state=dict(pmean=0.4995, lock=1, amean=0.89),
                           reaches=("unlocked", "cap_taken", "cap_not_taken", "err_clamped", "tiles_empty")),
    "meteor_locking": dict(policy="meteor", fixture=True, signal=dict(n=16384, seed=5, amp=1.0, noise=2), state=dict(pmean=0.20003),
                           reaches=("locked", "hyp_table")),
    "funcube_default": dict(policy="funcube", fixture=True, signal=dict(n=49152, seed=3, amp=100.0, noise=200),
                            reaches=("b_events", "a_events", "cap_not_taken", "hyp_high", "hyp_low", "hyp_table", "timing_below_1")),
    # (noise above a weak signal: with amp 100 here the locked loop's gain per step, alpha * |symbol| / 255, is above one, and one
    #  last bit of a cosine grows to a phase difference of 1 rad within the case -- tests/test_symbolwalk_host.py keeps the cases
    #  clear of that regime)
    "funcube_started": dict(policy="funcube", fixture=True, signal=dict(n=49152, seed=12, amp=8.0, noise=100),
                            state=dict(pmean=0.4995, lock=1, amean=8.995),
                            reaches=("unlocked", "cap_taken", "cap_not_taken", "err_clamped", "hyp_high", "hyp_low", "hyp_table")),
    "funcube_locking": dict(policy="funcube", fixture=True, signal=dict(n=49152, seed=6, amp=40.0), state=dict(pmean=0.2003, amean=60.0),
                            reaches=("locked",)),
    # timing far above P: an A event at every sample until it has come down, so more than one whole tile is all symbols
    "meteor_full_tile": dict(policy="meteor", signal=dict(n=3073, seed=7, amp=3.0, noise=24), state=dict(timing=4.0e4),
                             reaches=("tiles_full",)),
    "funcube_full_tile": dict(policy="funcube", signal=dict(n=3073, seed=8, amp=100.0, noise=200), state=dict(timing=2.5e5),
                              reaches=("tiles_full",)),
    # shorter than half a symbol from timing 0: no event at all
    "funcube_empty_tile": dict(policy="funcube", signal=dict(n=80, seed=9, amp=100.0, noise=200), reaches=("tiles_empty",)),
}


def case(name):
    """(policy, x, start state) of a named case"""
    c = CASES[name]
    return c["policy"], signal(c["policy"], **c["signal"]), start_state(c["policy"], **c.get("state", {}))


# The lengths test: around the 64 lanes that stage a tile and around one, two and three tiles.  Each length runs from timing 0 and
# from start timings that put the first A event (timing first reaches P there) or the first B event (timing in [P/2, P/2 + 1)
# there) on the sample before the last tile edge inside the input and on the sample after it -- the last sample of a tile and the
# first of the next; a length of one tile or less has them on its last sample.  Such a start timing is negative for all but the
# shortest: a state the walk reaches after a large negative resync error, single-stepped until it has come back to 1.
LENGTHS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 1)
LENGTH_SIGNAL = {"meteor": dict(n=LENGTHS[-1], seed=10, amp=3.0, noise=24), "funcube": dict(n=LENGTHS[-1], seed=11, amp=100.0, noise=200)}


def length_runs(policy):
    """[(n, start timing, None or (event kind "A" / "B", the sample it falls on))]"""
    P = params(policy)["P"]
    runs = []
    for n in LENGTHS:
        runs.append((n, 0.0, None))
        edge = ((n - 1) // TILE) * TILE
        for j in ([edge - 1, edge] if edge else [n - 1]):
            runs.append((n, P + 0.25 - j, ("A", j)))
            runs.append((n, P / 2 + 0.25 - j, ("B", j)))
    return runs
