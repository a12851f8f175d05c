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
