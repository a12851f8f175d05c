"""Seeded soft-symbol streams in the Meteor-M N2-x modes of DESIGN.md section 4.18, built directly -- no waveform, no symbol walk:
frame bodies -> _lrpt.frames_bits -> NRZ-M (differential) -> lrpt.encode -> the convolutional interleaver and its 0x27 markers
(interleaved) -> a prefix of random symbols -> _lrpt.noisy_soft (amplitude 64, sigma 16) -> the inverse of a chosen hypothesis, so
that the decoder must find that hypothesis.  Deterministic from the seed (NumPy PCG64)."""
import numpy as np

import _jpeg
import _lrpt
from directdemod_amd import lrpt

INVERSE = {h: next(g for g in range(8) if all(int(v) == w for v, w in zip(lrpt.hypothesis(*lrpt.hypothesis(3, 5, h), g), (3, 5))))
           for h in range(8)}


def distort(soft, h):
    """int8 soft pairs as the channel delivers them when the receiver must apply hypothesis h to get them back (values within
    -127..127, so that the negations are exact)"""
    a, b = lrpt.hypothesis(soft[0::2], soft[1::2], INVERSE[h])
    return np.stack((a, b), axis=1).ravel().astype(np.int8)


def stream(bodies, seed, differential=False, interleaved=False, branches=36, delay=8, start=0, prefix=0, hyp=0, amp=64.0, sigma=16.0):
    """-> dict(soft int8[2 nsym], nsym, starts): the bodies' frames from bit `start` of the first, behind `prefix` random symbols.
    starts[i] = the symbol of frame i's marker (negative for the cut first frame): in the received stream, or with `interleaved`
    in the deinterleaved stream, which begins at the first code bit sent.  An interleaved stream is followed by B M (B - 1)
    random filler bits and the interleaver's own run-out, so that every frame's last bit leaves the deinterleaver."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bits = _lrpt.frames_bits(bodies)
    if differential:
        bits = lrpt.nrzm_encode(bits)
    code = lrpt.encode(bits)[2 * start:]
    if interleaved:
        span = branches * delay * (branches - 1)
        code = np.concatenate((code, rng.integers(0, 2, span + span % 2, dtype=np.uint8)))
        code = lrpt.add_markers_np(lrpt.interleave_np(code, branches, delay))
    code = np.concatenate((rng.integers(0, 2, 2 * prefix, dtype=np.uint8), code)).reshape(-1, 2)
    soft = np.clip(_lrpt.noisy_soft(code, amp, sigma, seed + 1), -127, 127).astype(np.int8)
    first = 36 * (prefix // 40) - start if interleaved else prefix - start      # a whole period of prefix passes as 36 symbols
    return dict(soft=distort(soft, hyp), nsym=len(code), starts=[first + lrpt.FRAME_BITS * i for i in range(len(bodies))])


def random_bodies(seed, n):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(n, lrpt.BODY_BYTES), dtype=np.uint8)


def picture_frames(seed, strips=2, q=60):
    """A picture of `strips` strip cycles laid into as many frames as its packets fill -> (_jpeg.build's dict, the packets that are
    completed inside those frames, in order)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pkts = _jpeg.cycles(rng, _jpeg.picture(rng, strips), q)
    nframes = sum(len(p["data"]) for p in pkts) // _jpeg.ZONE
    built = _jpeg.build(pkts, nframes)
    return built, [p["data"] for p in built["packets"] if p["last"] is not None]
