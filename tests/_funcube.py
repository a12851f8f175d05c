"""Seeded Funcube-like BPSK recordings for the decode_funcube tests: 1200 bit/s rectangular-pulse BPSK at 2.048 MS/s carrying the
reference's 33-bit sync (decode_funcube.py:170) at given times, on a carrier, with Gaussian noise, as u8 IQ pairs.
Deterministic from the seed (NumPy PCG64); each fixture stores the sha256 of the recording it was made from."""
import hashlib

import numpy as np

FS = 2048000
BIT_RATE = 1200
SYMBOL_RATE = 12000
SYNC = "101000110001000000000001010111100"
CENTER = 145000000                  # what a corrfreq decode is told: the recording's centre and the channel's frequency
CHANNEL = 145025000

# name -> synthesis parameters; `offset` and `corrfreq` are what the decoder is told
CASES = {
    "a": dict(seed=21, seconds=0.6, carrier=300.0, syncs=(0.2, 0.35)),                                  # clean
    "b": dict(seed=22, seconds=0.6, carrier=30000.0 + 300.0, syncs=(0.2, 0.35), offset=30000),          # +30 kHz, told
    "c": dict(seed=23, seconds=0.6, carrier=300.0, phase=np.pi, syncs=(0.2, 0.35)),                     # inverted: score below 165
    "d": dict(seed=24, seconds=0.3, carrier=300.0, amp=0.0, syncs=()),                                  # noise only
    "e": dict(seed=25, seconds=0.4, carrier=300.0, syncs=(0.15,)),                                      # one MAXSYNC: the reference raises
    "f": dict(seed=26, seconds=10.5, carrier=-20000.0 + 150.0, syncs=(0.3, 5.28, 10.26), offset=-20000),    # two chunks
    "g": dict(seed=27, seconds=10.5, carrier=25000.0, drift=(300.0, -300.0), syncs=(0.3, 5.28, 10.26), offset=25000,
              corrfreq=True),                                                                            # Doppler track + ramp
}


def sync_bits():
    return np.array([int(i) for i in SYNC], dtype=np.int64)


def synth(seed, seconds, carrier=0.0, phase=0.0, amp=60.0, sigma=4.0, syncs=(), drift=None):
    """-> uint8[n, 2] IQ pairs (I, Q) centred on 127.5.  `syncs`: the times (s) at which a sync word starts (moved to the bit grid);
    `drift` = (f0, f1): the carrier moves linearly from carrier + f0 to carrier + f1 Hz over the recording"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(round(seconds * FS))
    nbit = n * 3 // 5120 + 2                          # 1200 / 2048000 = 3 / 5120
    bits = rng.integers(0, 2, size=nbit)
    pat = sync_bits()
    for t0 in syncs:
        p = int(round(t0 * BIT_RATE))
        bits[p:p + len(pat)] = pat
    t = np.arange(n, dtype=np.int64)
    x = amp * (2.0 * bits[t * 3 // 5120] - 1.0)
    if drift is None:
        ph = 2.0 * np.pi * carrier * t / FS + phase
    else:
        f0, f1 = drift
        tt = t / FS
        ph = 2.0 * np.pi * ((carrier + f0) * tt + 0.5 * (f1 - f0) / seconds * tt * tt) + phase
    x = x * np.exp(1j * ph)
    del ph
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.stack((x.real, x.imag), axis=1) + 127.5
    return np.clip(np.rint(iq), 0, 255).astype(np.uint8)


def case(name):
    """(raw, offset, corrfreq) of a named case"""
    p = dict(CASES[name])
    off = p.pop("offset", 0)
    corr = p.pop("corrfreq", False)
    return synth(**p), off, corr


def sha256(raw):
    return hashlib.sha256(np.ascontiguousarray(raw).tobytes()).hexdigest()
