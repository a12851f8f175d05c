"""The G3RUH 9600 baud FSK chain of DESIGN.md section 4.20 (dd_fsk.h) restated for tests/test_fsk_host.py and tests/test_gpu_fsk.py:
`walk_host`, the timing walk sample by sample in Python floats with its branch counters; `bits_host`, the hard decision, descrambler
and NRZI in NumPy with the stuffing marks and start flags; the seeded `signal` and the named `CASES` of the walk; and a synthesiser
on top of _ax25 (`line_bits` -> `nrz` -> `audio` or `fm_iq`, chained by `recording`).  Every operation of walk_host is one IEEE
float64 operation of + - * / abs or a comparison, in the order the design text writes out, so the device is compared with
np.array_equal."""
import numpy as np

import _ax25

TILE = 1024                       # samples the device stages per step
BAUD = 9600
G = 0.1                           # the loop gain
AM0 = 1.0

FLOAT_FIELDS = ("t", "dc", "am", "prev", "mid", "last")
INT_FIELDS = ("ctr", "overflow")
ARRAYS = ("sym", "sidx", "tmu")
COUNTERS = ("mid_events", "eye_events", "mid_interpolated", "eye_interpolated", "eye_before_mid", "clamp_high", "clamp_low",
            "am_guard", "am_tiny", "back_to_back")


def params(P, g=G):
    return dict(P=P, g=g)


def params_array(p):
    """`params` as the four doubles the device entry point takes (DDFskParams)"""
    return np.array([p["P"], p["P"] / 2, (p["P"] / 2) + 1, p["g"]], dtype=np.float64)


def start_state(**over):
    s = dict.fromkeys(FLOAT_FIELDS, 0.0)
    s.update(dict.fromkeys(INT_FIELDS, 0))
    s["am"] = AM0
    s.update(over)
    return s


def state_struct(s, dtype):
    st = np.zeros(1, dtype=dtype)
    for f in FLOAT_FIELDS + INT_FIELDS:
        st[f] = s[f]
    return st


def walk_host(x, base, state, prm):
    """The walk over the samples x (float64) = samples base .. of the recording, from `state` (a dict, not modified) -> (state
    after, per-symbol arrays sym (float64), sidx (int64), tmu (float64), counters).  `overflow` is carried as it is: this walk has
    no capacity."""
    P, g = prm["P"], prm["g"]
    halfP, halfP1 = P / 2, (P / 2) + 1
    s = dict(state)
    cnt = dict.fromkeys(COUNTERS, 0)
    sym, sidx, tmu = [], [], []
    t, dc, am, prev, mid, last = (s[f] for f in FLOAT_FIELDS)
    seen_mid = False
    last_eye = None
    for j, v in enumerate(np.asarray(x, dtype=np.float64).tolist()):
        dc = (dc * 4095.0 + v) / 4096.0
        y = v - dc
        am = (am * 1023.0 + abs(y)) / 1024.0
        if am > 0.0:
            a = y / am
            if am < 1e-300:
                cnt["am_tiny"] += 1
        else:
            a = 0.0
            cnt["am_guard"] += 1
        if t >= halfP and t < halfP1:
            mid = a - (t - halfP) * (a - last)
            cnt["mid_events"] += 1
            cnt["mid_interpolated"] += (t - halfP) != 0.0
            seen_mid = True
        elif t >= P:
            mu = t - P
            eye = a - mu * (a - last)
            t = t - P
            e = (eye - prev) * mid
            if e > 1.0:
                e = 1.0
                cnt["clamp_high"] += 1
            elif e < -1.0:
                e = -1.0
                cnt["clamp_low"] += 1
            t = t + g * e
            prev = eye
            sym.append(eye)
            sidx.append(base + j)
            tmu.append(t)
            s["ctr"] += 1
            cnt["eye_events"] += 1
            cnt["eye_interpolated"] += mu != 0.0
            cnt["eye_before_mid"] += not seen_mid
            cnt["back_to_back"] += last_eye == j - 1
            last_eye = j
        last = a
        t = t + 1.0
    s.update(t=t, dc=dc, am=am, prev=prev, mid=mid, last=last)
    arrays = dict(sym=np.array(sym, dtype=np.float64), sidx=np.array(sidx, dtype=np.int64), tmu=np.array(tmu, dtype=np.float64))
    return s, arrays, cnt


def scramble_host(d):
    """the transmitter's scrambler from an all-zero register: out[k] = d[k] ^ out[k-12] ^ out[k-17]"""
    out = [0] * 17
    for b in d:
        out.append(int(b) ^ out[-12] ^ out[-17])
    return out[17:]


def bits_host(sym):
    """soft symbols -> (r, bits, marks, flags): r[k] = sym[k] > 0, d[k] = r[k] ^ r[k-12] ^ r[k-17] with zeros before the start,
    bits[0] = 1, bits[k] = (d[k] == d[k-1]); marks and flags as _ax25.bits_host makes them"""
    r = (np.asarray(sym, dtype=np.float64) > 0).astype(np.int8)
    n = len(r)
    ext = np.concatenate((np.zeros(17, dtype=np.int8), r))
    d = ext[17:] ^ ext[5:5 + n] ^ ext[:n]
    b = np.ones(n, dtype=np.int8)
    if n > 1:
        b[1:] = d[1:] == d[:-1]
    flags = [k for k in range(n - 8) if tuple(b[k:k + 8]) == (0, 1, 1, 1, 1, 1, 1, 0)]
    marks = np.zeros(n, dtype=np.int8)
    run = 0
    for k in range(n):
        if run == 5:
            marks[k] = 2 if b[k] == 1 else 1
        run = run + 1 if b[k] == 1 else 0
    return r, b, marks, np.array(flags, dtype=np.int64)


def symbols_for(bits):
    """soft symbols (+-1) whose bits_host decoding is `bits` (bits[0] must be 1): NRZI levels from level 1, scrambled from zeros"""
    assert bits[0] == 1
    d = [1] + _ax25.nrzi([int(b) for b in bits[1:]], level=1)
    return np.where(np.array(scramble_host(d)) == 1, 1.0, -1.0)


# ---------------------------------------------------------------------------------------------------------------- exact inputs
def signal(P, n, seed, amp=3.0, noise=8, offset=0.0, zeros=0):
    """n samples of rectangular NRZ at P samples per bit, every sample a multiple of 1/8: +-amp, uniform noise of up to `noise`
    eighths and `offset` on top, after `zeros` samples that are exactly 0.  PCG64 integers, exact arithmetic: the same samples on
    every machine."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bits = rng.integers(0, 2, size=int(n / P) + 2)
    nz = rng.integers(-noise, noise + 1, size=n)
    k = (np.arange(n) / P).astype(np.int64)
    a8, o8 = int(round(amp * 8)), int(round(offset * 8))
    assert a8 == amp * 8 and o8 == offset * 8
    x = (a8 * (2 * bits[k] - 1) + nz + o8) / 8.0
    x[:zeros] = 0.0
    return x


P_FRAC = 2048000 / 42 / 9600          # 2.048 MS/s cut to 5 * 9600 S/s: 5.0794 samples per bit

# The walk's named cases: samples per bit, `signal` arguments, start state overrides, and the counters each is there for.
# More than two tiles without an event cannot happen for a finite timing: P <= 64 puts a mid and an eye event into every 66
# samples (a NaN timing fires none at all, and the walk still visits every sample once).
CASES = {
    "fractional": dict(P=P_FRAC, signal=dict(n=4096, seed=1, noise=8),
                       reaches=("mid_events", "eye_events", "mid_interpolated", "eye_interpolated", "clamp_high", "clamp_low")),
    "p2": dict(P=2.0, signal=dict(n=3000, seed=2, noise=4), reaches=("mid_events", "eye_events", "back_to_back")),
    "p64": dict(P=64.0, signal=dict(n=8192, seed=3, noise=4), reaches=("mid_events", "eye_events", "eye_interpolated")),
    # the discriminator's offset under a carrier error: the dc tracker starts far off
    "offset": dict(P=5.0, signal=dict(n=4096, seed=4, noise=8, offset=50.0), reaches=("mid_events", "eye_events", "clamp_high", "clamp_low")),
    # a loud start against am = 1: the error is clamped on both sides until am has caught up
    "clamped": dict(P=P_FRAC, signal=dict(n=3000, seed=5, amp=300.0, noise=64), reaches=("clamp_high", "clamp_low")),
    "eye_first": dict(P=5.0, signal=dict(n=2051, seed=6), state=dict(t=5.3), reaches=("eye_before_mid", "mid_events")),
    # am = 0 and samples that are exactly 0: the guard gives a = 0, and the walk takes up the signal behind them
    "am_zero": dict(P=P_FRAC, signal=dict(n=3000, seed=7, zeros=1500), state=dict(am=0.0), reaches=("am_guard", "eye_events")),
    # the smallest positive am and a long run of zeros: (am * 1023) / 1024 rounds back to am (to 512 units of 2^-1074 from above),
    # so am never decays to 0 and the guard is not taken -- y / am = 0 all the same
    "am_tiny": dict(P=P_FRAC, signal=dict(n=3000, seed=8, zeros=2500), state=dict(am=5e-324), reaches=("am_tiny", "eye_events")),
    # timing far above P: an eye event at every sample until it has come down, with mu in the thousands
    "eye_run": dict(P=5.0, signal=dict(n=3073, seed=9), state=dict(t=1.2e4), reaches=("back_to_back", "eye_interpolated")),
}


def case(name):
    """(parameters, x, start state) of a named case"""
    c = CASES[name]
    return params(c["P"]), signal(c["P"], **c["signal"]), start_state(**c.get("state", {}))


LENGTHS = (0, 1, 1023, 1024, 1025, 2051)
CUTS = ((1,), (1023,), (1024,), (1500,), (1, 1022, 1), (1024, 1024))


# ------------------------------------------------------------------------------------------------------------------ recordings
FRAMES = [(("APRS", 0), ("N0CALL", 7), _ax25.INFO, ()),
          (("APZ001", 0), ("DL1ABC", 9), "=5230.00N/01320.00E>first", (("WIDE1", 1),)),
          (("APRS", 0), ("K1XYZ", 0), _ax25.INFO + " bad", ()),
          (("CQ", 0), ("VK2ZZ", 15), ">status text " + "x" * 20, (("WIDE1", 1), ("WIDE2", 2)))]
BAD = (2,)


def line_bits(frames=FRAMES, bad=BAD, lead_flags=260, tail_flags=60):
    """-> (the scrambled line bits, the frames' bytes): flags, the frames with their stuffing and flags, flags; NRZI (a 0 toggles),
    then the scrambler 1 + x^12 + x^17"""
    flag = [0, 1, 1, 1, 1, 1, 1, 0]
    bits = flag * lead_flags
    fb = []
    for i, (dst, src, info, path) in enumerate(frames):
        f = _ax25.frame_bytes(dst, src, info, path, bad_crc=i in bad)
        fb.append(f)
        bits += _ax25.hdlc_bits(f)
    bits += flag * tail_flags
    return np.array(scramble_host(_ax25.nrzi(bits)), dtype=np.int8), fb


def nrz(line, spb, bt=0.5, invert=False):
    """line bits -> Gaussian-filtered NRZ in [-1, 1] at `spb` (fractional) samples per bit: rectangular pulses, then a Gaussian of
    bandwidth-time product `bt`, its taps normalised to sum 1"""
    n = int(len(line) * spb)
    k = np.minimum((np.arange(n) / spb).astype(np.int64), len(line) - 1)
    lv = 2.0 * np.asarray(line, dtype=np.float64)[k] - 1.0
    sigma = np.sqrt(np.log(2.0)) / (2.0 * np.pi * bt) * spb
    half = int(np.ceil(4 * sigma))
    h = np.exp(-0.5 * (np.arange(-half, half + 1) / sigma) ** 2)
    out = np.convolve(lv, h / h.sum(), mode="same")
    return -out if invert else out


def audio(line, P, seed, ppm=0.0, invert=False, sigma=0.05, offset=0.0, oversample=8):
    """line bits -> FM-demodulated audio as a discriminator would give it, at P samples per nominal bit: the NRZ built `oversample`
    times finer and picked, a baud error of `ppm`, an offset, Gaussian noise"""
    fine = nrz(line, oversample * P / (1.0 + ppm * 1e-6), invert=invert)[::oversample]
    rng = np.random.default_rng(seed)
    return 0.4 * fine + offset + sigma * rng.standard_normal(len(fine))


def fm_iq(line, fs, seed, ppm=0.0, invert=False, dev=3000.0, amp=60.0, sigma=2.0, f_carrier=0.0, baud=BAUD):
    """line bits -> u8 IQ pairs at fs: Gaussian NRZ, FM with +-dev Hz, a carrier offset, Gaussian noise"""
    rng = np.random.default_rng(seed)
    m = nrz(line, fs / (baud * (1.0 + ppm * 1e-6)), invert=invert)
    n = len(m)
    ph = 2 * np.pi * dev * np.cumsum(m) / fs
    if f_carrier:
        ph = ph + 2 * np.pi * ((f_carrier / fs * np.arange(n)) % 1.0)
    s = amp * np.exp(1j * ph) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    raw = np.empty((n, 2), dtype=np.uint8)
    raw[:, 0] = np.clip(np.round(s.real + 127.5), 0, 255).astype(np.uint8)
    raw[:, 1] = np.clip(np.round(s.imag + 127.5), 0, 255).astype(np.uint8)
    return raw


# about 0.45 s each: four frames, the third with a corrupted CRC, 100 ppm baud error, amplitude 60, noise sigma 2
RECORDINGS = {
    "960k": dict(fs=960000, offset=0, seed=31, ppm=100.0, invert=False),             # P = 5
    "1M_inverted": dict(fs=1000000, offset=12500, seed=32, ppm=100.0, invert=True),    # P = 5.2083
}


def recording(name):
    """-> (raw u8 IQ, fs, offset, the three good frames' bytes without FCS)"""
    c = RECORDINGS[name]
    line, fb = line_bits()
    raw = fm_iq(line, c["fs"], c["seed"], ppm=c["ppm"], invert=c["invert"], f_carrier=float(c["offset"]))
    return raw, c["fs"], c["offset"], [f[:-2] for i, f in enumerate(fb) if i not in BAD]


def noise_recording(fs=960000, seconds=0.1, seed=33, sigma=20.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(127.5 + sigma * rng.standard_normal((int(fs * seconds), 2))), 0, 255).astype(np.uint8)
