"""Seeded recordings for the Doppler tests (frequency_shift): a carrier -- or a 1200-baud BPSK signal -- swept along a tanh S-curve
of +-3 kHz around a channel 73.2 kHz above the centre frequency, in Gaussian noise, quantised to u8 I,Q at 2.048 MS/s.
Deterministic from the seed (NumPy PCG64), built at test time; each fixture stores the sha256 of the recording it was made from."""
import hashlib

import numpy as np

FS = 2048000
CENTER = 145865000
CHANNEL = 145938200            # 73.2 kHz above the centre
BANDWIDTH = 20000
SWING = 3000.0
SIGMA = 12.0
POSITIONS = ((0, 10), (1, 10), (5, 10), (9, 10), (10, 10))       # (chunk_number, chunk_length) handed to correct()

# name -> samples, amplitude in LSB, seed, modulation
CASES = {
    "a": dict(n=int(1.3 * FS) + 3000, amp=6.0, seed=21),          # every = 1.30..., 2 slices per row, 326 slices -> 163 rows, the
                                                                   # partial tail closes the last row
    "b": dict(n=2 * FS, amp=3.0, seed=22),                        # every = 2.0 exactly (the >= equality), 500 slices -> 250 rows
    "c": dict(n=int(3.4 * FS) + 1234, amp=3.0, seed=23),          # every = 3.40..., 4 slices per row, 851 slices -> 212 rows, 3 dropped
    "d": dict(n=int(2.2 * FS), amp=8.0, seed=24, baud=1200),      # BPSK: flat spectral top, 3 slices per row, 550 -> 183 rows
}


def synth(n, amp, seed, baud=None):
    """-> uint8[n, 2] IQ pairs centred on 127.5"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n, dtype=np.float64) / FS
    T = n / FS
    tau = T / 6.0
    # f(t) = (CHANNEL - CENTER) + SWING tanh((t - T/2) / tau); the phase is its integral
    u = (t - T / 2) / tau
    cyc = (CHANNEL - CENTER) * t + SWING * tau * (np.logaddexp(u, -u) - np.log(2.0))
    x = amp * np.exp(2j * np.pi * (cyc - np.floor(cyc)))
    if baud:
        bits = rng.integers(0, 2, size=int(n * baud // FS) + 2)
        x = x * (2.0 * bits[(np.arange(n, dtype=np.int64) * baud) // FS] - 1.0)
    x = x + SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.stack((x.real, x.imag), axis=1) + 127.5
    return np.clip(np.rint(iq), 0, 255).astype(np.uint8)


_made = {}


def case(name):
    """the recording of a named case, uint8[n, 2] (made once per process, read-only)"""
    if name not in _made:
        raw = synth(**CASES[name])
        raw.setflags(write=False)
        _made[name] = raw
    return _made[name]


def sha(raw):
    return hashlib.sha256(np.ascontiguousarray(raw).tobytes()).hexdigest()


# ---------------------------------------------------------------- restatements shared by the Doppler test modules (CPU only)
def _row_sums(raw, window, every, mags, dtype):
    """make_fft's row sums before the log: `mags(block[k, window] of complex float64) -> |FFT| per window`, summed in window order
    in `dtype`.  Slices start every `window` samples, a final partial one included; every slice counts towards a row of
    ceil(every), only full windows are added, slices after the last closed row are dropped."""
    raw = np.asarray(raw).reshape(-1)
    n = raw.size // 2
    x = (raw[0::2].astype(np.float64) - 127) + 1j * (raw[1::2].astype(np.float64) - 127)
    row_len = int(np.ceil(every))
    n_full, n_slices = n // window, -(-n // window)
    rows = n_slices // row_len
    m = mags(x[:n_full * window].reshape(n_full, window))
    out = np.zeros((rows, window), dtype=dtype)
    for r in range(rows):
        for w in range(r * row_len, min((r + 1) * row_len, n_full)):
            out[r] = out[r] + m[w]
    return out


def waterfall_f64(raw, window, every):
    """make_fft's rows (log domain, fftshifted) in float64 throughout -> float64 [rows, window]"""
    s = _row_sums(raw, window, every, lambda b: np.abs(np.fft.fft(b, axis=1)), np.float64)
    with np.errstate(divide="ignore"):
        return np.log(np.fft.fftshift(s, axes=1) / window / every)


def waterfall_f32_cpu(raw, window, every):
    """the same rows by a float32 pipeline that shares no code with the device: scipy's complex64 transform, float32 magnitudes,
    a float32 sum over the row's windows in window order, the log in float64, stored as float32"""
    import scipy.fft

    def mags(b):
        X = scipy.fft.fft(b.astype(np.complex64), axis=1)
        assert X.dtype == np.complex64
        return np.abs(X)

    s = _row_sums(raw, window, every, mags, np.float32)
    assert s.dtype == np.float32
    with np.errstate(divide="ignore"):
        return np.log(np.fft.fftshift(s, axes=1).astype(np.float64) / window / every).astype(np.float32)


WATERFALL_FACTOR = 4.0


def waterfall_check(got, raw, window, every, what):
    """`got`: the device's rows [rows, window].  The device must lie within WATERFALL_FACTOR times the float32 CPU pipeline's own
    largest log-domain difference from the float64 statement (both are float32 transforms of one length whose error grows
    alike; the factor allows for another summation and butterfly order).  The bound comes from the CPU alone.
    -> (device figure, CPU figure)"""
    want = waterfall_f64(raw, window, every)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(want).all(), "%s: a compared column is not finite in the float64 statement" % what
    cpu = np.abs(waterfall_f32_cpu(raw, window, every).astype(np.float64) - want).max()
    assert np.isfinite(cpu) and cpu > 0, (what, cpu)
    dev = np.abs(got.astype(np.float64) - want).max()
    print("%s: device %.3g, float32 CPU pipeline %.3g, ratio %.2f" % (what, dev, cpu, dev / cpu))
    assert dev <= WATERFALL_FACTOR * cpu, "%s: device %.3g, float32 CPU pipeline %.3g, ratio %.2f" % (what, dev, cpu, dev / cpu)
    return dev, cpu


def tones(window, bins):
    """whole windows, window r the tone 100 exp(2 pi i bins[r] t / window), quantised like synth -> uint8 [len(bins) * window, 2]"""
    t = np.arange(window, dtype=np.float64)
    ph = np.outer(np.asarray(bins, dtype=np.float64), t) / window
    x = (100.0 * np.exp(2j * np.pi * (ph - np.floor(ph)))).reshape(-1)
    iq = np.stack((x.real, x.imag), axis=1) + 127.5
    return np.clip(np.rint(iq), 0, 255).astype(np.uint8)


def ramp_freqs(f0, delta, target, n):
    """f[i] = f0 + i * delta, a product and a sum each rounded to float64, clipped to the target (from above when it lies above
    f0, from below otherwise)"""
    f = f0 + np.arange(n, dtype=np.float64) * delta
    if target > f0:
        f[f > target] = target
    else:
        f[f < target] = target
    return f


def mixer_expected(x, f, start, fs):
    """x[i] exp(-2 pi i frac(f[i] (start + i) / fs)): the fraction in IEEE float64 in the kernels' operation order (NumPy gives
    the same bits), cos, sin and the product in np.longdouble -> (re, im) as longdouble arrays"""
    idx = (np.int64(start) + np.arange(len(x), dtype=np.int64)).astype(np.float64)
    cyc = np.asarray(f, dtype=np.float64) * idx / np.float64(fs)
    fr = cyc - np.floor(cyc)
    two_pi = 2 * np.arctan2(np.longdouble(0), np.longdouble(-1))        # pi to the longdouble's precision
    ang = two_pi * fr.astype(np.longdouble)
    cs, sn = np.cos(ang), np.sin(ang)
    xr, xi = x.real.astype(np.longdouble), x.imag.astype(np.longdouble)
    return xr * cs + xi * sn, xi * cs - xr * sn


def ulp32(v):
    """the spacing of float32 at |v| (of the float32 nearest to it), as float64"""
    return np.spacing(np.abs(np.asarray(v)).astype(np.float32)).astype(np.float64)
