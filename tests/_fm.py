"""Seeded FM voice-like recordings for the decode_fm tests: two tones (1000 Hz and 2700 Hz, half the deviation each) frequency-modulated
on a carrier at the offset the decoder is told, amplitude 0.7 of full scale, Gaussian noise of 0.05 of full scale per component,
quantised to u8 I,Q pairs.  Deterministic from the seed (NumPy PCG64), built at test time; each fixture stores the sha256 of the
recording it was made from.  Every case is decoded in chunks of CHUNK samples."""
import hashlib

import numpy as np

CHUNK = 1 << 16
TONES = (1000.0, 2700.0)
FULL_SCALE = 127.5

# name -> rate, samples, what the decoder is told (offset, bw, audioFreq; None = its default) and the deviation
CASES = {
    "a": dict(fs=2048000, n=3 * CHUNK + 12345, offset=25000.0, bw=None, audioFreq=None, dev=5000.0, seed=31),     # /68, ragged tail
    "b": dict(fs=2048000, n=2 * CHUNK + 777, offset=-300000.0, bw=60000, audioFreq=20800, dev=10000.0, seed=32),  # /34: the block-sum kernel
    "c": dict(fs=2400000, n=3 * CHUNK, offset=0.0, bw=30000, audioFreq=15000, dev=3000.0, seed=33),               # /80, whole chunks only
}


def synth(fs, n, offset, dev, seed, **_):
    """-> uint8[n, 2] IQ pairs centred on 127.5"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n, dtype=np.float64) / fs
    cyc = offset * t                                   # the phase in cycles: the carrier plus the integral of the two tones
    for f in TONES:
        cyc = cyc - 0.5 * dev / (2.0 * np.pi * f) * np.cos(2.0 * np.pi * f * t)
    x = 0.7 * FULL_SCALE * np.exp(2j * np.pi * (cyc - np.floor(cyc)))
    x = x + 0.05 * FULL_SCALE * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
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


def told(name):
    """(fs, offset, bw, audioFreq) as handed to decode_fm"""
    p = CASES[name]
    return p["fs"], p["offset"], p["bw"], p["audioFreq"]


def sha(raw):
    return hashlib.sha256(np.ascontiguousarray(raw).tobytes()).hexdigest()
