"""Seeded Meteor-M2 LRPT recordings for the frame decoding tests: channel frames (attached sync marker, 1020 random body bytes XOR
the CCSDS pseudo-noise sequence) through the rate-1/2, K = 7 encoder, one QPSK symbol per code bit pair, with _meteor.synth's
waveform: 72 ksym/s rectangular pulses at 2.048 MS/s on a carrier, with Gaussian noise, as u8 IQ pairs.  The recording starts at a
random bit inside a frame.  Deterministic from the seed (NumPy PCG64); the fixture stores the sha256 of the recording it was made from."""
import numpy as np

from _meteor import FS, sha256  # noqa: F401

from directdemod_amd import lrpt

FIRST, HYP = 9159, 3          # case a: the frames past loop acquisition start at symbol FIRST + 8192 i under hypothesis HYP

CASES = {
    "a": dict(seed=31, seconds=1.3, carrier=300.0, phase=0.7, amp=40.0, sigma=4.0),
}


def frames_bits(bodies):
    """uint8[n, 1020] bodies -> the n channel frames' bits, uint8[n * 8192]"""
    bodies = np.asarray(bodies, dtype=np.uint8)
    cadu = np.concatenate((np.tile(lrpt.ASM, (len(bodies), 1)), bodies ^ lrpt.pn_sequence()[None, :]), axis=1)
    return np.unpackbits(cadu.ravel())


def stream(seed, nsym, rng=None):
    """-> (bodies uint8[n, 1020], start, code bits uint8[nsym, 2]): nsym // 8192 + 2 frames, enough to cover nsym symbols from
    bit `start` of the first; the encoder runs from state 0 at the first frame's first bit"""
    rng = np.random.Generator(np.random.PCG64(seed)) if rng is None else rng
    bodies = rng.integers(0, 256, size=(nsym // lrpt.FRAME_BITS + 2, lrpt.BODY_BYTES), dtype=np.uint8)
    start = int(rng.integers(0, lrpt.FRAME_BITS))
    code = lrpt.encode(frames_bits(bodies)).reshape(-1, 2)
    return bodies, start, code[start:start + nsym]


def synth(seed, seconds, carrier=0.0, phase=0.0, amp=40.0, sigma=4.0):
    """-> (uint8[n, 2] IQ pairs (I, Q) centred on 127.5, bodies, start)"""
    n = int(round(seconds * FS))
    nsym = n * 9 // 256 + 2                           # 72000 / 2048000 = 9 / 256
    rng = np.random.Generator(np.random.PCG64(seed))
    bodies, start, code = stream(seed, nsym, rng)
    sym = (2.0 * code[:, 0] - 1.0) + 1j * (2.0 * code[:, 1] - 1.0)
    t = np.arange(n, dtype=np.int64)
    x = amp * sym[t * 9 // 256]
    x = x * np.exp(1j * (2.0 * np.pi * carrier * t / FS + phase))
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.stack((x.real, x.imag), axis=1) + 127.5
    return np.clip(np.rint(iq), 0, 255).astype(np.uint8), bodies, start


def case(name):
    """(raw, bodies, start) of a named case"""
    return synth(**CASES[name])


def noisy_soft(code, amp, sigma, seed):
    """code bits uint8[n, 2] -> int8[2 n] soft pairs: +-amp plus Gaussian noise, truncated and clipped to int8"""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = amp * (2.0 * code.ravel() - 1.0) + sigma * rng.standard_normal(code.size)
    return np.clip(np.trunc(v), -128, 127).astype(np.int8)


def aligned(soft, nsym, code, at=40000, width=512, reach=400):
    """(lag, h) with received symbol q = sent symbol q + lag under h, from the hard bits of symbols at .. at + width"""
    hits = []
    for h in range(8):
        a, b = lrpt.hypothesis(soft[2 * at:2 * (at + width):2], soft[2 * at + 1:2 * (at + width):2], h)
        hard = np.stack((a > 0, b > 0), axis=1).astype(np.uint8)
        for d in range(-reach, reach + 1):
            agree = np.mean(hard == code[at + d:at + d + width])
            if agree > 0.95:
                hits.append((d, h))
    assert len(hits) == 1, hits
    return hits[0]
