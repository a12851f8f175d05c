"""Seeded inputs for the Funcube frame decoder's tests (funcube_fec.py): symbol-level int8 arrays carrying
frames of funcube_fec.encode_frame, and one recording in the style of tests/_funcube.synth whose bits are the differentially
encoded channel bits.  Deterministic from the seed (NumPy PCG64)."""
import numpy as np

import _funcube
from directdemod_amd import funcube_fec as fec

AMP = 90                              # symbol amplitude of the symbol-level arrays
FS = _funcube.FS


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def payload(seed):
    return rng(seed).integers(0, 256, fec.FRAME_BYTES, dtype=np.uint8)


def position(lead, bit):
    """the position p in D of a frame whose first channel bit is bit `bit` of a stream that starts after `lead` symbols: ten symbols
    (the bit before, the differential reference) ahead of the frame's first symbol"""
    return lead + fec.SYMBOLS_PER_BIT * (bit - 1)


def symbols(seed, nbits, frames, lead=0, sigma=0.0, amp=AMP):
    """-> int8[lead + 10 nbits]: random idle bits with, for every (bit, data, inverted) of `frames`, the 5200 channel bits of `data`
    from bit `bit` >= 1 on (complemented when inverted), differentially encoded, ten symbols of +-amp per bit behind `lead` symbols
    of the first level, plus Gaussian noise, rounded and clipped to int8"""
    g = rng(seed)
    bits = g.integers(0, 2, nbits).astype(np.uint8)
    for bit, data, inverted in frames:
        assert 1 <= bit and bit + fec.CHANNEL_BITS <= nbits
        bits[bit:bit + fec.CHANNEL_BITS] = fec.encode_frame(data) ^ np.uint8(1 if inverted else 0)
    lev = np.repeat(fec.differential(bits), fec.SYMBOLS_PER_BIT)
    lev = np.concatenate((np.full(lead, lev[0], dtype=np.uint8), lev))
    x = amp * (2.0 * lev - 1.0) + sigma * g.standard_normal(len(lev))
    return np.clip(np.rint(x), -128, 127).astype(np.int8)


def pairs(r, seed=0):
    """int8 soft symbols -> the int8 (re, im) pairs the device reads, the imaginary parts random"""
    out = rng(1000 + seed).integers(-128, 128, 2 * len(r)).astype(np.int8)
    out[0::2] = r
    return out


def recording(seed, data, lead_bits=600, tail_bits=360, carrier=300.0, amp=60.0, sigma=4.0):
    """-> (uint8[n, 2] IQ pairs at 2.048 MS/s, the sample at which the frame's first channel bit starts): 1200 bit/s rectangular
    BPSK of the differentially encoded stream random bits, the frame of `data`, random bits; on a carrier, with Gaussian noise"""
    g = rng(seed)
    bits = np.concatenate((g.integers(0, 2, lead_bits), fec.encode_frame(data), g.integers(0, 2, tail_bits))).astype(np.uint8)
    lev = fec.differential(bits)
    n = len(bits) * 5120 // 3                       # 2048000 / 1200 = 5120 / 3 samples per bit
    t = np.arange(n, dtype=np.int64)
    x = amp * (2.0 * lev[t * 3 // 5120] - 1.0) * np.exp(2.0j * np.pi * carrier * t / FS)
    del t
    x += sigma * (g.standard_normal(n) + 1j * g.standard_normal(n))
    iq = np.stack((x.real, x.imag), axis=1) + 127.5
    return np.clip(np.rint(iq), 0, 255).astype(np.uint8), -(-lead_bits * 5120 // 3)
