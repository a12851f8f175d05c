"""
FM stereo audio from the multiplex of a broadcast station: the 19 kHz pilot, L - R on the suppressed 38 kHz subcarrier and the
de-emphasis (beyond the reference; DESIGN.md section 4.29 defines every stage; device side: dd_fmstereo.h): the constants, the taps,
a NumPy restatement `pilot_host` / `carrier_host` / `mix_host` / `fir_host` of the kernels, the device wrappers over the C entries,
`decode`, the chain behind decode_fmstereo, which runs over either set of stages (`DeviceOps`, `HostOps`), and `multiplex` /
`encode_mpx` / `encode`, a synthesiser.

The multiplex is the FM discriminator's output in radians per sample at R S/s, quantised as for RDS (rds.quantise).  Blocks of 256
samples are correlated with a 19 kHz table phasor (P); the sum S of the 17 blocks around a block gives the pilot's phase delta against
the table, and u = -S^2 / |S|^2 = exp(2 i delta) in Q14 turns the table's 38 kHz phasor into the transmitter's subcarrier sin 2 phi.
Every sample is multiplied by 1 + 2 g sin 2 phi and by 1 - 2 g sin 2 phi, and one decimating FIR (a 15 kHz low-pass convolved with the
de-emphasis) over each product gives left and right at about 48 kS/s.  A block whose pilot is below `pilotMin` has u = 0: mono.

Met in synthesised recordings only; INTEGRATION.md lists the limits.
"""
import functools
import math

import numpy as np

from . import rds
from ._burst import Laps, need
from ._hip import DevArray, check, lib
from .rds import DEVIATION, PILOT, RATE_MAX, RATE_MIN

B = 256                               # DD_FMS_B
W = 8                                 # DD_FMS_W
PILOT_SHIFT, CARRIER_SHIFT = 10, 8    # |P| <= 2^27, |S| <= 17 * 2^19
Q = 14                                # u, the table and the mixer's factor are Q14
GAIN_SHIFT, G_MAX = 12, 12288         # G = rint(2 g 4096), g <= 1.5
MIX_SHIFT, OUT_SHIFT = 8, 15
TAPS_MAX, D_MAX = 1024, 12
THR_MAX = 1 << 48
AB_MAX = (1 << 23) + 1536             # |a|, |b| at most: 2^15 (2^16 + 12) >> 8
TAPS_SUM_MAX = 1 << 17                # the sum of |taps| at most, so that the FIR's sums stay below 2^41
OUT_MAX = 1 << 26
AUDIO_RATE = 48000.0
PASSBAND, CUTOFF = 15000.0, 16750.0   # the low-pass passes 15 kHz; its -6 dB point, between 15 kHz and the pilot
KAISER_BETA = 7.0
DEEMPHASIS = (None, 50e-6, 75e-6)
DE_REACH = 8.0                        # the de-emphasis' impulse response is cut at 8 tau
GAIN_MIN, GAIN_MAX = 0.5, 1.5
RDS_LEVEL = 0.04

_F64 = np.dtype(np.float64)
_I32 = np.dtype(np.int32)


def check_options(deemphasis=50e-6, pilotMin=0.03, diffGain=None):
    if deemphasis not in DEEMPHASIS:
        raise ValueError("fmstereo: deemphasis must be 50e-6, 75e-6 or None, got %r" % (deemphasis,))
    if not 0.0 < pilotMin <= 0.5:
        raise ValueError("fmstereo: pilotMin must be a fraction of the peak deviation in (0, 0.5], got %r" % (pilotMin,))
    if diffGain is not None and not GAIN_MIN <= diffGain <= GAIN_MAX:
        raise ValueError("fmstereo: diffGain must be None or from %g to %g, got %r" % (GAIN_MIN, GAIN_MAX, diffGain))


def params(rate):
    """(D, step19, step38) for a multiplex rate R: D = max(1, rint(R / 48000)) samples per audio sample, step19 = rint(19000 * 2^32
    / R), step38 = 2 step19 mod 2^32, so the 38 kHz phase is exactly twice the pilot's.  ValueError unless 125 000 <= R <= 500 000."""
    rate = float(rate) if rate and rate > 0 else float("nan")
    if not RATE_MIN <= rate <= RATE_MAX:
        raise ValueError("fmstereo: a multiplex rate of %r S/s is not supported; %g to %g are" % (rate, RATE_MIN, RATE_MAX))
    step19 = int(round(PILOT * 4294967296.0 / rate))
    return max(1, int(round(rate / AUDIO_RATE))), step19, (2 * step19) & 0xFFFFFFFF


def pilot_unit(rate):
    """|S| / cnt of a pilot at the peak deviation: its amplitude in q, 2 * 75000 / R * 2^15, times 256 / 2 * 2^14 >> 10 >> 8 * 256"""
    return 2.0 * DEVIATION / float(rate) * 32768.0 * 8.0


def threshold(pilotMin, rate):
    """thr of the lock decision |S|^2 >= thr cnt^2 for a pilot of `pilotMin` of the peak deviation"""
    thr = int(round((pilotMin * pilot_unit(rate)) ** 2))
    if not 0 <= thr <= THR_MAX:
        raise ValueError("fmstereo: pilotMin %r gives a threshold beyond 2^48" % (pilotMin,))
    return thr


def gain_word(g):
    """G = rint(2 g 4096)"""
    G = int(round(2.0 * float(g) * (1 << GAIN_SHIFT)))
    if not 0 <= G <= G_MAX:
        raise ValueError("fmstereo: a difference gain of %r is not supported; up to %g is" % (g, GAIN_MAX))
    return G


def lowpass(rate):
    """float64: the 15 kHz low-pass, a Kaiser(7) windowed sinc of the odd length nearest 255 R / 240 000 with its -6 dB point at
    16.75 kHz: at that length the window's transition is some 4 kHz wide, so 15 kHz passes and the 19 kHz pilot is rejected"""
    n = 2 * int(round((255.0 * rate / 240000.0 - 1.0) / 2.0)) + 1
    m = np.arange(n) - (n - 1) / 2.0
    h = np.sinc(2.0 * CUTOFF / rate * m) * np.kaiser(n, KAISER_BETA)
    return h / h.sum()


def deemphasis_taps(rate, tau):
    """float64: the one-pole de-emphasis alpha exp(-i / (tau R)) cut at 8 tau, its sum 1; [1] for None"""
    if tau is None:
        return np.ones(1)
    d = np.exp(-np.arange(int(math.ceil(DE_REACH * tau * rate))) / (tau * rate))
    return d / d.sum()


@functools.lru_cache(maxsize=None)
def taps(rate, deemphasis=50e-6):
    """(h, d0): h = rint(2^15 (lowpass * de-emphasis)) as int32, at most 1024 long, and the low-pass' centre d0, so that output o
    sits at input time o D"""
    lp = lowpass(float(rate))
    h = np.rint(32768.0 * np.convolve(lp, deemphasis_taps(float(rate), deemphasis))).astype(np.int32)
    if len(h) > TAPS_MAX or int(np.abs(h.astype(np.int64)).sum()) > TAPS_SUM_MAX:
        raise ValueError("fmstereo: %d taps at %r S/s are beyond the budget" % (len(h), rate))
    h.setflags(write=False)
    return h, (len(lp) - 1) // 2


def diff_gain(fs, rate):
    """the difference channel's gain g for a recording at fs S/s cut to `rate`: 1 / (|Hw(38 kHz)| / |Hw(0)| * sinc(38000 / R)), Hw the
    front end's Blackman-Harris window of rds.window_taps(fs) taps at fs, the sinc the discriminator's first difference: what the
    front end takes from the 38 kHz band against the audio band"""
    from . import filters
    w = filters._cosine_sum(rds.window_taps(fs), [0.35875, 0.48829, 0.14128, 0.01168])
    hw = abs(np.sum(w * np.exp(-2j * np.pi * 2.0 * PILOT / float(fs) * np.arange(len(w))))) / abs(np.sum(w))
    return float(1.0 / (hw * np.sinc(2.0 * PILOT / float(rate))))


def audio_scale(rate):
    """the float value of one unit of the int32 output: mpx = 1 (the peak deviation) is q = 2 * 75000 / R * 2^15, and the chain's
    gain from q to the output is 2^14 >> 8 = 2^6"""
    return float(rate) / (2.0 * DEVIATION * 32768.0 * 64.0)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def pilot_host(mpx, step19):
    """int64[n // 256, 2]: P, the block sums of q times the 19 kHz table phasor, shifted down (|P| <= 2^27)"""
    q = rds.quantise(mpx)
    nb = len(q) // B
    w = rds.table()[rds.phases(0, nb * B, step19)].astype(np.int64)
    return (q[:nb * B, None] * w).reshape(nb, B, 2).sum(axis=1) >> PILOT_SHIFT


def carrier_host(P, thr):
    """(S int64[nb, 2], u int64[nb, 2], lock uint8[nb]) of the pilot blocks: S = (the sum of the 17 blocks around each that exist)
    >> 8; locked iff |S|^2 > 0 and |S|^2 >= thr cnt^2; u = -S^2 / |S|^2 in Q14 by floor divisions when locked, else 0"""
    P = np.asarray(P, dtype=np.int64).reshape(-1, 2)
    nb = len(P)
    cum = np.concatenate((np.zeros((1, 2), np.int64), np.cumsum(P, axis=0)))
    k = np.arange(nb)
    lo, hi = np.maximum(k - W, 0), np.minimum(k + W, nb - 1)
    S = (cum[hi + 1] - cum[lo]) >> CARRIER_SHIFT
    cnt = (hi - lo + 1).astype(np.int64)
    sr, si = S[:, 0], S[:, 1]
    mag = sr * sr + si * si
    lock = (mag > 0) & (mag >= int(thr) * cnt * cnt)
    den = np.where(mag > 0, mag, 1)
    u = np.stack(((-((sr * sr - si * si) << Q)) // den, (-((2 * sr * si) << Q)) // den), axis=1)
    return S, np.where(lock[:, None], u, 0), lock.astype(np.uint8)


def mix_host(mpx, step38, u, G):
    """int64[n, 2]: a = q (2^14 + c2) >> 8 and b = q (2^14 - c2) >> 8, c = (tr ui + ti ur) >> 14 with (tr, ti) = conj(table[phase38]),
    c2 = c G >> 12, u of the block min(n // 256, nb - 1); without a block u = 0"""
    q = rds.quantise(mpx)
    u = np.asarray(u, dtype=np.int64).reshape(-1, 2)
    c2 = np.zeros(len(q), np.int64)
    if len(u) and len(q):
        k = np.minimum(np.arange(len(q)) // B, len(u) - 1)
        t = rds.table()[rds.phases(0, len(q), step38)].astype(np.int64)
        c2 = (((t[:, 0] * u[k, 1] - t[:, 1] * u[k, 0]) >> Q) * int(G)) >> GAIN_SHIFT
    return np.stack(((q * ((1 << Q) + c2)) >> MIX_SHIFT, (q * ((1 << Q) - c2)) >> MIX_SHIFT), axis=1)


def fir_host(ab, h, D, d0, chunk=4096):
    """int64[ceil(n / D), 2]: (the sum over i of h[i] ab[o D + d0 - i]) >> 15 per column, samples outside the data 0.  The products
    are summed in float64 where every sum stays below 2^53 (exact, as on the device), else in int64."""
    ab = np.asarray(ab, dtype=np.int64).reshape(-1, 2)
    h = np.asarray(h, dtype=np.int64).ravel()
    n, L = len(ab), len(h)
    nout = (n + D - 1) // D
    out = np.zeros((nout, 2), np.int64)
    if nout == 0:
        return out
    right = max(0, (nout - 1) * D + d0 - (n - 1))
    exact = n == 0 or int(np.abs(ab).max()) * int(np.abs(h).sum()) < 1 << 53
    kind = np.float64 if exact else np.int64
    p = np.concatenate((np.zeros((L - 1 - d0, 2), kind), ab.astype(kind), np.zeros((right, 2), kind)))
    hr = h[::-1].astype(kind)
    for c in range(2):
        win = np.lib.stride_tricks.sliding_window_view(p[:, c], L)[::D]
        for a in range(0, nout, chunk):
            out[a:a + chunk, c] = (win[a:min(nout, a + chunk)] @ hr).astype(np.int64)
    return out >> OUT_SHIFT


def audio_host(mpx, step38, u, G, h, D, d0):
    """int32[ceil(n / D), 2]: left and right as the device stores them"""
    return fir_host(mix_host(mpx, step38, u, G).astype(np.int32), h, D, d0).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ the device stages
def _taps_device(h):
    h = np.ascontiguousarray(h, dtype=np.int32).ravel()
    if not 1 <= len(h) <= TAPS_MAX or int(np.abs(h.astype(np.int64)).sum()) > TAPS_SUM_MAX:
        raise ValueError("fmstereo: 1 to %d taps whose magnitudes sum to at most 2^17 expected" % TAPS_MAX)
    return DevArray.from_host(h)


def pilot(mpx, step19):
    """float64 device multiplex -> (P as a device int32 array of n // 256 pairs, the blocks) (dd_fms_pilot)"""
    need(mpx, _F64, "fmstereo.pilot")
    nb = mpx.n // B
    P = DevArray(max(2 * nb, 2), np.int32)
    check(lib().dd_fms_pilot(mpx.ptr, mpx.n, int(step19), rds.table_device().ptr, P.ptr, None), "dd_fms_pilot")
    return P.view(0, 2 * nb), nb


def carrier(P, nb, thr):
    """device P of nb pairs -> (S int32[nb, 2] on the host, u as a device int32 array of nb pairs, lock uint8[nb] on the host)
    (dd_fms_carrier)"""
    need(P, _I32, "fmstereo.carrier")
    S, u, lock = DevArray(max(2 * nb, 2), np.int32), DevArray(max(2 * nb, 2), np.int32), DevArray(max(nb, 1), np.uint8)
    check(lib().dd_fms_carrier(P.ptr, int(nb), int(thr), S.ptr, u.ptr, lock.ptr, None), "dd_fms_carrier")
    return S.to_host()[:2 * nb].reshape(nb, 2), u.view(0, 2 * nb), lock.to_host()[:nb]


def audio(mpx, step38, u, nb, G, h, D, d0, route=None):
    """float64 device multiplex, device u of nb pairs -> left and right as a device int32 array of ceil(n / D) pairs (dd_fms_audio;
    route 0 or 1: dd_debug_fms_audio_route, the filter's sums in int64 or in float64)"""
    need(mpx, _F64, "fmstereo.audio")
    if nb:
        need(u, _I32, "fmstereo.audio")
    nout = (mpx.n + D - 1) // D
    out, hd = DevArray(max(2 * nout, 2), np.int32), _taps_device(h)
    args = (mpx.ptr, mpx.n, int(step38), rds.table_device().ptr, u.ptr if nb else None, int(nb), int(G), hd.ptr, hd.n, int(D), int(d0))
    if route is None:
        check(lib().dd_fms_audio(*args, out.ptr, None), "dd_fms_audio")
    else:
        check(lib().dd_debug_fms_audio_route(*args, int(route), out.ptr, None), "dd_debug_fms_audio_route")
    return out.view(0, 2 * nout)


def mix_device(mpx, step38, u, nb, G):
    """a and b of every sample as int32[n, 2] on the host (dd_debug_fms_mix, a diagnostic)"""
    need(mpx, _F64, "fmstereo.mix_device")
    ab = DevArray(max(2 * mpx.n, 2), np.int32)
    check(lib().dd_debug_fms_mix(mpx.ptr, mpx.n, int(step38), rds.table_device().ptr, u.ptr if nb else None, int(nb), int(G), ab.ptr, None),
          "dd_debug_fms_mix")
    return ab.to_host()[:2 * mpx.n].reshape(mpx.n, 2)


class HostOps(Laps):
    """the stages of `decode` in NumPy"""

    def pilot(self, mpx, step19):
        P = pilot_host(mpx, step19)
        return P, len(P)

    def carrier(self, P, nb, thr):
        return carrier_host(P, thr)

    def audio(self, mpx, step38, u, nb, G, h, D, d0):
        return audio_host(mpx, step38, u, G, h, D, d0)


class DeviceOps(Laps):
    """the stages of `decode` on the device; `laps` collects seconds per stage, with a synchronisation after each"""

    def pilot(self, mpx, step19):
        out = pilot(mpx, step19)
        self.lap("pilot")
        return out

    def carrier(self, P, nb, thr):
        out = carrier(P, nb, thr)
        self.lap("carrier")
        return out

    def audio(self, mpx, step38, u, nb, G, h, D, d0):
        out = audio(mpx, step38, u, nb, G, h, D, d0)
        self.lap("audio")
        out = out.to_host().reshape(-1, 2)
        self.lap("download")
        return out


# ------------------------------------------------------------------------------------------------------------------ the host logic
def pilot_info(S, lock, rate, step19):
    """pilotInfo: blocks, locked, level (the median |S| / cnt as a fraction of the peak deviation) and freqError in Hz (the table's
    frequency less 19 kHz plus the median phase step per block of S, taken between locked blocks 17 apart, whose sums share no block:
    the receiver's clock error at 19 kHz, unambiguous to R / (2 * 256 * 17) Hz either way)"""
    S = np.asarray(S, dtype=np.int64).reshape(-1, 2)
    nb = len(S)
    info = {"blocks": nb, "locked": int(np.count_nonzero(lock)), "level": 0.0, "freqError": 0.0}
    if nb:
        k = np.arange(nb)
        cnt = np.minimum(k + W, nb - 1) - np.maximum(k - W, 0) + 1
        info["level"] = float(np.median(np.hypot(S[:, 0], S[:, 1]) / cnt)) / pilot_unit(rate)
        z = S[:, 0] + 1j * S[:, 1]
        lag = min(2 * W + 1, nb - 1)                                       # sums that share no block where the data allow it
        lock = np.asarray(lock) != 0
        both = lock[lag:] & lock[:nb - lag] if lag else np.zeros(0, bool)
        if both.any():
            step = float(np.median(np.angle(z[lag:][both] * np.conj(z[:nb - lag][both])))) / lag
            info["freqError"] = step19 * float(rate) / 4294967296.0 - PILOT + step * float(rate) / (2.0 * np.pi * B)
    return info


def decode(mpx, rate, deemphasis=50e-6, pilotMin=0.03, gain=1.0, ops=None):
    """The chain behind decode_fmstereo over the multiplex (a float64 device array for DeviceOps, NumPy for HostOps) at `rate` S/s ->
    (int32[n_out, 2] left and right at rate / D on the host, pilotInfo, lock uint8[blocks])"""
    ops = HostOps() if ops is None else ops
    check_options(deemphasis, pilotMin, gain)
    D, step19, step38 = params(rate)
    h, d0 = taps(float(rate), deemphasis)
    P, nb = ops.pilot(mpx, step19)
    S, u, lock = ops.carrier(P, nb, threshold(pilotMin, rate))
    out = ops.audio(mpx, step38, u, nb, gain_word(gain), h, D, d0)
    info = pilot_info(S, lock, rate, step19)
    ops.lap("host")
    return out, info, lock


def to_float(out, rate):
    """getAudio of the int32 output: float32, +-1 the peak deviation"""
    return (np.asarray(out, dtype=np.float64) * audio_scale(rate)).astype(np.float32)


def to_pcm(out, rate):
    """getPCM of the int32 output: int16, rint(32767 * the float value), clipped"""
    return np.clip(np.rint(np.asarray(out, dtype=np.float64) * (audio_scale(rate) * 32767.0)), -32768, 32767).astype(np.int16)


def is_stereo(info):
    """1 if more than half of pilotInfo's blocks are locked, else 0"""
    return 1 if 2 * info["locked"] > info["blocks"] else 0


class StereoSignal:
    """what sink.wavFile reads: ``sampRate`` and ``signal``, the int16[n, 2] of to_pcm"""

    def __init__(self, sampRate, signal):
        self.sampRate = int(round(sampRate))
        self.signal = signal


# ------------------------------------------------------------------------------------------------------------------ the synthesiser
def times(n, rate, clock_ppm=0.0):
    """the transmitter's time of the receiver's samples 0 .. n - 1, its clock `clock_ppm` fast"""
    return np.arange(int(n)) / (float(rate) * (1.0 + clock_ppm * 1e-6))


def tone(freq, amp, n, rate, clock_ppm=0.0, phase=0.0):
    """float64[n]: a programme tone as the receiver samples it"""
    return amp * np.sin(2.0 * np.pi * freq * times(n, rate, clock_ppm) + phase)


def preemphasise(x, rate, tau):
    """the inverse of deemphasis_taps' one pole: (x[n] - p x[n - 1]) / (1 - p), p = exp(-1 / (tau R))"""
    p = math.exp(-1.0 / (tau * rate))
    x = np.asarray(x, dtype=np.float64)
    return (x - p * np.concatenate(([x[0] if len(x) else 0.0], x[:-1]))) / (1.0 - p)


def multiplex(left, right, rate, pilot=0.09, level=0.9, pilot_phase=0.0, preemphasis=None, rds_bits=None, clock_ppm=0.0):
    """float64[n]: the stereo multiplex as a fraction of the peak deviation: level ((L + R) / 2 + (L - R) / 2 sin 2 phi) + pilot sin
    phi, phi = 2 pi 19000 t + pilot_phase, and with rds_bits (uint8) the RDS signal at 0.04 on 3 phi.  left and right: the programme
    at `rate` as the receiver samples it (`tone`).  preemphasis: the time constant applied to both.  clock_ppm: the receiver's sample
    clock error, which moves the pilot and the subcarriers."""
    left, right = np.asarray(left, dtype=np.float64).ravel(), np.asarray(right, dtype=np.float64).ravel()
    if len(left) != len(right):
        raise ValueError("fmstereo: left and right must be equally long")
    n = len(left)
    if preemphasis is not None:
        left, right = preemphasise(left, rate, preemphasis), preemphasise(right, rate, preemphasis)
    phi = 2.0 * np.pi * PILOT * times(n, rate, clock_ppm) + pilot_phase
    x = level * (0.5 * (left + right) + 0.5 * (left - right) * np.sin(2.0 * phi)) + pilot * np.sin(phi)
    if rds_bits is not None:
        x = x + RDS_LEVEL * rds.symbols(rds_bits, rate, n, 0.0, clock_ppm) * np.sin(3.0 * phi)
    return x


def encode_mpx(left, right, rate, sigma=0.0, seed=0, deviation=DEVIATION, **kw):
    """The discriminator's view of a station: float64[n] in radians per sample, 2 pi deviation * multiplex / rate, plus Gaussian
    noise of `sigma` radians; the keywords of `multiplex`"""
    x = 2.0 * np.pi * deviation / rate * multiplex(left, right, rate, **kw)
    if sigma:
        x = x + np.random.default_rng(seed).normal(0.0, sigma, len(x))
    return x


def encode(left, right, rate, offset=0.0, amplitude=60.0, sigma=0.0, seed=0, deviation=DEVIATION, **kw):
    """A recording uint8[n, 2] at `rate` S/s with the station `offset` Hz from the centre, frequency modulated at 75 kHz deviation by
    `multiplex` (its keywords); Gaussian noise of `sigma` per rail; the u8 value is clip(rint(z + 127.5), 0, 255), as rds.encode"""
    mpx = multiplex(left, right, rate, **kw)
    rng = np.random.default_rng(seed)
    phase = rng.uniform(0.0, 2.0 * np.pi) + 2.0 * np.pi * np.cumsum(deviation * mpx + offset) / rate
    z = amplitude * np.exp(1j * phase)
    v = np.stack((z.real, z.imag), axis=1) + 127.5
    if sigma:
        v = v + rng.normal(0.0, 1.0, v.shape) * sigma
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)
