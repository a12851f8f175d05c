"""Seeded Meteor-M2-like QPSK recordings for the decode_meteorm2 tests: 72 ksym/s rectangular-pulse QPSK at 2.048 MS/s carrying the
reference's 120-bit sync (decode_meteorm2.py:163) every 8192 symbols, on a carrier, with Gaussian noise, as u8 IQ pairs.
Deterministic from the seed (NumPy PCG64); each fixture stores the sha256 of the recording it was made from."""
import hashlib

import numpy as np

FS = 2048000
SYMBOL_RATE = 72000
SYNC = "0, 13, 13, 12, 13, 13, 13, 0, 0, 0, 13, 13, 0, 13, 13, 0, 13, 0, 0, 0, 13, 13, 13, 0, 0, 13, 0, 13, 0, 13, 0, 13, 13, 0, 0, 0, " \
       "13, 13, 0, 0, 0, 0, 13, 0, 13, 13, 0, 0, 0, 0, 0, 13, 1, 13, 0, 13, 13, 13, 13, 12, 0, 13, 0, 13, 0, 0, 13, 0, 13, 0, 13, " \
       "13, 0, 13, 13, 13, 0, 0, 0, 0, 13, 0, 13, 0, 13, 13, 13, 13, 13, 0, 13, 13, 13, 0, 0, 0, 0, 13, 13, 13, 0, 13, 0, 0, 0, 13, " \
       "0, 13, 13, 0, 13, 0, 13, 13, 0, 0, 0, 13, 13, 13"

# name -> synthesis parameters; `offset` is what the decoder is told
CASES = {
    "a": dict(seed=11, seconds=1.0, carrier=300.0, phase=0.0),                          # clean
    "b": dict(seed=12, seconds=0.8, carrier=30000.0 + 300.0, phase=0.0, offset=30000),  # +30 kHz, told
    "c": dict(seed=13, seconds=0.8, carrier=0.0, phase=np.pi / 2),                      # 90 degree ambiguity: buff4corr, sync2mhz2
    "d": dict(seed=14, seconds=2.3, carrier=300.0, phase=0.0, bursts=((0.0, 0.5), (1.65, 2.3))),   # fade of 1.15 s
    "e": dict(seed=15, seconds=0.4, carrier=0.0, phase=0.0, amp=0.0),                   # noise only
    "f": dict(seed=16, seconds=10.5, carrier=-20000.0 + 300.0, phase=0.0, offset=-20000),   # two chunks, mixer restart
    "g": dict(seed=17, seconds=0.24, carrier=300.0, phase=0.0),                         # one MAXSYNC: the reference raises
}


def sync_bits():
    s = np.array([int(i) for i in SYNC.split(",")])
    return (s >= 7).astype(np.int64)


def synth(seed, seconds, carrier=0.0, phase=0.0, amp=40.0, sigma=4.0, bursts=None, sync_every=8192, first_sync=1500):
    """-> uint8[n, 2] IQ pairs (I, Q) centred on 127.5"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(round(seconds * FS))
    nsym = n * 9 // 256 + 2                           # 72000 / 2048000 = 9 / 256
    bits = rng.integers(0, 2, size=(nsym, 2))
    pat = sync_bits().reshape(-1, 2)
    for p in range(first_sync, nsym - len(pat), sync_every):
        bits[p:p + len(pat)] = pat
    sym = (2.0 * bits[:, 0] - 1.0) + 1j * (2.0 * bits[:, 1] - 1.0)
    t = np.arange(n, dtype=np.int64)
    x = amp * sym[t * 9 // 256]
    if bursts is not None:
        on = np.zeros(n, dtype=bool)
        for a, b in bursts:
            on[int(a * FS):int(b * FS)] = True
        x = np.where(on, x, 0.0)
    x = x * np.exp(1j * (2.0 * np.pi * carrier * t / FS + phase))
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.stack((x.real, x.imag), axis=1) + 127.5
    return np.clip(np.rint(iq), 0, 255).astype(np.uint8)


def case(name):
    """(raw, offset) of a named case"""
    p = dict(CASES[name])
    off = p.pop("offset", 0)
    return synth(**p), off


def sha256(raw):
    return hashlib.sha256(np.ascontiguousarray(raw).tobytes()).hexdigest()
