"""
Slow-scan television, PD modes (beyond the reference; DESIGN.md section 4.21 defines the chain operation by operation; device side:
dd_sstv.h): the mode table, `encode` (a continuous-phase tone synthesiser), the tap design, a NumPy restatement `*_host` of every
kernel, the VIS parser, the sync-grid fit, the device wrappers over the C entries, and `decode`, the chain behind decode_sstv, which
runs over either set of stages (`DeviceOps`, `HostOps`): the host logic is one piece of code for both.

The mode figures come from public descriptions of the PD modes and have not been checked against a recording or another decoder.
"""
import ctypes as C
import logging
import math
from collections import namedtuple

import numpy as np

from . import _hip
from ._burst import Laps
from ._hip import DevArray, check, lib

Mode = namedtuple("Mode", "name vis width height pixel")           # pixel time in seconds
MODES = {m.name: m for m in (
    Mode("PD50", 93, 320, 256, 0.286e-3), Mode("PD90", 99, 320, 256, 0.532e-3), Mode("PD120", 95, 640, 496, 0.190e-3),
    Mode("PD160", 98, 512, 400, 0.382e-3), Mode("PD180", 96, 640, 496, 0.286e-3), Mode("PD240", 97, 640, 496, 0.382e-3),
    Mode("PD290", 94, 800, 616, 0.286e-3))}
BY_VIS = {m.vis: m for m in MODES.values()}

SYNC_S, PORCH_S = 20e-3, 2.08e-3
F_SYNC, F_PORCH, F_BLACK, F_WHITE = 1200.0, 1500.0, 1500.0, 2300.0
F_LEADER, F_ONE, F_ZERO = 1900.0, 1100.0, 1300.0
LEADER_S, BREAK_S, BIT_S = 300e-3, 10e-3, 30e-3
VIS_S = 2 * LEADER_S + BREAK_S + 10 * BIT_S                         # 0.91 s

CLS_NONE, CLS_1100, CLS_1200, CLS_1300, CLS_LEADER = range(5)
EDGES_HZ = (1000.0, 1150.0, 1250.0, 1400.0, 1800.0, 2000.0)        # the class bands' edges
F_CENTRE, F_CUT = 1700.0, 900.0                                     # the band-pass: middle of 1100..2300 Hz, low-pass cut-off
MAX_K = 511
RATE_MIN, RATE_MAX = 6000.0, 255000.0                               # audio rates the chain accepts (K = 2 int(rate / 1000) + 1 <= 511)
LAG_TILE = 256                                                      # DD_SSTV_TILE
SYNC_FRACTION, LEADER_FRACTION = 0.7, 0.8                           # window-count thresholds of the two run searches
GRID_TOLERANCE = 0.1                                                # a sync is accepted within this fraction of a period of its prediction

_F64, _I8, _U8, _C128 = np.dtype(np.float64), np.dtype(np.int8), np.dtype(np.uint8), np.dtype(np.complex128)


def mode_of(mode):
    """a Mode, a name or None -> Mode or None"""
    if mode is None or isinstance(mode, Mode):
        return mode
    if mode not in MODES:
        raise ValueError("sstv: unknown mode %r; known: %s" % (mode, ", ".join(sorted(MODES))))
    return MODES[mode]


def line_time(mode):
    """seconds per line pair"""
    return SYNC_S + PORCH_S + 4 * mode.width * mode.pixel


def check_rate(rate, mode=None):
    """ValueError unless the chain accepts the audio rate, and the mode's pixel lasts at least two samples"""
    if not RATE_MIN <= rate <= RATE_MAX:
        raise ValueError("sstv: an audio rate of %r S/s is outside %g to %g S/s" % (rate, RATE_MIN, RATE_MAX))
    if mode is not None and rate * mode.pixel < 2:
        raise ValueError("sstv: at %r S/s a %s pixel of %g ms is %.3f samples; at least 2 are needed"
                         % (rate, mode.name, mode.pixel * 1e3, rate * mode.pixel))


# ------------------------------------------------------------------------------------------------------------------ the transmitter
def rgb_to_levels(image_rgb):
    """uint8[H, W, 3], H even -> (y uint8[H, W], cr, cb uint8[H / 2, W]): the levels a PD transmitter sends, the colour differences
    averaged over the two rows of a pair"""
    a = np.asarray(image_rgb, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] % 2:
        raise ValueError("sstv: an RGB image with an even number of rows expected, got shape %r" % (a.shape,))
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    y = 16.0 + (65.738 * r + 129.057 * g + 25.064 * b) / 256.0
    cr = 128.0 + (112.439 * r - 94.154 * g - 18.285 * b) / 256.0
    cb = 128.0 + (-37.945 * r - 74.494 * g + 112.439 * b) / 256.0
    q = lambda v: np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return q(y), q((cr[0::2] + cr[1::2]) / 2), q((cb[0::2] + cb[1::2]) / 2)


def vis_tones(code):
    """[(Hz, seconds)] of the VIS header for a seven-bit code, even parity"""
    bits = [(code >> j) & 1 for j in range(7)]
    bits.append(sum(bits) & 1)
    return ([(F_LEADER, LEADER_S), (F_SYNC, BREAK_S), (F_LEADER, LEADER_S), (F_SYNC, BIT_S)]
            + [(F_ONE if b else F_ZERO, BIT_S) for b in bits] + [(F_SYNC, BIT_S)])


def tones(y, cr, cb, mode, vis=True):
    """(freqs, durations) of a transmission: the VIS header, then per line pair sync, porch, Y odd, R-Y, B-Y, Y even.  Fewer rows than
    the mode's height give a transmission that ends early."""
    mode = mode_of(mode)
    y, cr, cb = (np.asarray(v, dtype=np.float64) for v in (y, cr, cb))
    pairs, W = cr.shape
    if W != mode.width or y.shape != (2 * pairs, W) or cb.shape != cr.shape or 2 * pairs > mode.height:
        raise ValueError("sstv: %s sends %d x %d pixels; got Y %r, R-Y %r, B-Y %r" % (mode.name, mode.width, mode.height, y.shape,
                                                                                      cr.shape, cb.shape))
    head = vis_tones(mode.vis) if vis else []
    f = np.empty((pairs, 2 + 4 * W))
    f[:, 0], f[:, 1] = F_SYNC, F_PORCH
    lv = np.concatenate((y[0::2], cr, cb, y[1::2]), axis=1)
    f[:, 2:] = F_BLACK + lv * ((F_WHITE - F_BLACK) / 255.0)
    t = np.empty_like(f)
    t[:, 0], t[:, 1], t[:, 2:] = SYNC_S, PORCH_S, mode.pixel
    return (np.concatenate(([h[0] for h in head], f.ravel())), np.concatenate(([h[1] for h in head], t.ravel())))


def synth(freqs, durations, rate, clock_error=0.0, phase=0.0):
    """cos of the continuous phase of a tone sequence, sampled at `rate`: the transmitter's clock runs slow by clock_error (every
    duration is (1 + clock_error) times its nominal)"""
    freqs = np.asarray(freqs, dtype=np.float64)
    ends = np.cumsum(np.asarray(durations, dtype=np.float64) * (1.0 + clock_error))
    starts = np.concatenate(([0.0], ends[:-1]))
    cycles = np.concatenate(([0.0], np.cumsum(freqs * (ends - starts))))[:-1]
    t = np.arange(int(math.floor(ends[-1] * rate + 1e-9))) / float(rate)
    j = np.minimum(np.searchsorted(ends, t, side="right"), len(freqs) - 1)
    return np.cos(phase + 2 * np.pi * ((cycles[j] + freqs[j] * (t - starts[j])) % 1.0))


def card(mode, pairs):
    """(y, cr, cb) levels of a picture of `pairs` line pairs for tests and benchmarks: smooth gradients and slow sinusoids whose
    three channels differ (a swapped channel, row or pixel offset shows), and eight flat bars on the second row of every fourth pair"""
    mode = mode_of(mode)
    W = mode.width
    u = np.arange(W) / W
    r = np.arange(2 * pairs).reshape(-1, 1)
    y = 128 + 90 * np.sin(2 * np.pi * (1.5 * u + 0.11 * r)) + 20 * (u - 0.5)
    q = np.arange(pairs).reshape(-1, 1)
    cr = 128 + 100 * (u - 0.5) + 30 * np.cos(2 * np.pi * (u + 0.2 * q))
    cb = 128 - 80 * (u - 0.5) + 40 * np.sin(2 * np.pi * (2 * u + 0.3 * q))
    y[1::8] = np.array([16, 235, 60, 200, 100, 160, 30, 128])[np.minimum((u * 8).astype(int), 7)]
    f = lambda v: np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return f(y), f(cr), f(cb)


def encode(image_rgb, mode, rate, vis=True, clock_error=0.0):
    """RGB image (uint8[H, W, 3], W the mode's width, H even and at most the mode's height) -> float64 audio at `rate` S/s"""
    y, cr, cb = rgb_to_levels(image_rgb)
    return synth(*tones(y, cr, cb, mode, vis), rate, clock_error)


# ------------------------------------------------------------------------------------------------------------------ the design
def tap_count(rate):
    return 2 * int(rate / 1000.0) + 1


def design(rate):
    """the complex band-pass for `rate`: (K real parts, K imaginary parts), a Hamming-windowed sinc low-pass of cut-off F_CUT and unit
    sum, shifted to F_CENTRE; K = 2 int(rate / 1000) + 1 (about 2 ms)"""
    check_rate(rate)
    K = tap_count(rate)
    m = np.arange(K) - (K - 1) // 2
    lp = np.sinc(2 * F_CUT / rate * m) * (0.54 + 0.46 * np.cos(2 * np.pi * m / max(K - 1, 1)))
    lp = lp / lp.sum()
    w = 2 * np.pi * F_CENTRE / rate * m
    return np.ascontiguousarray(lp * np.cos(w)), np.ascontiguousarray(lp * np.sin(w))


def edges(rate):
    """six cosines then six sines of 2 pi f / rate over EDGES_HZ"""
    w = 2 * np.pi * np.array(EDGES_HZ) / rate
    return np.concatenate((np.cos(w), np.sin(w)))


def delay(K):
    """d[n] belongs to the instant n - delay(K) of the audio"""
    return (K - 1) / 2 + 0.5


_EDGE_CACHE = {}


def sync_edge(rate):
    """How far a run search's position lies before the start of a 1200 Hz tone as long as its window, in lag-product samples: the
    window count stops growing where the class 1200 ends, which is a little before the tone does; the distance depends on the
    filter alone, and is measured on a synthesised 1200 -> 1500 Hz step (mean over eight phases)."""
    if rate not in _EDGE_CACHE:
        hr, hi = design(rate)
        K = len(hr)
        n0 = 3 * K
        total = 0.0
        for j in range(8):
            x = synth([F_SYNC, F_PORCH], [n0 / rate, 3 * K / rate], rate, phase=2 * np.pi * j / 8)
            cls = classes_host(*lag_host(x, hr, hi), edges(rate))
            last = int(np.nonzero(cls == CLS_1200)[0][-1])
            total += n0 + delay(K) - (last + 1)
        _EDGE_CACHE[rate] = total / 8
    return _EDGE_CACHE[rate]


# ------------------------------------------------------------------------------------------------------------------ the restatement
def lag_host(x, hr, hi):
    """dd_sstv_lag -> (re, im) of d"""
    x = np.asarray(x, dtype=np.float64)
    n, K = len(x), len(hr)
    xp = np.concatenate((np.zeros(K - 1), x))
    zr, zi = np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for k in range(K):
            seg = xp[K - 1 - k:K - 1 - k + n]
            zr = zr + hr[k] * seg
            zi = zi + hi[k] * seg
        pr, pi = np.concatenate(([0.0], zr[:-1]))[:n], np.concatenate(([0.0], zi[:-1]))[:n]
        return zr * pr + zi * pi, zi * pr - zr * pi


def classes_host(dr, di, e):
    """dd_sstv_classes"""
    with np.errstate(all="ignore"):
        ge = [e[j] * di >= e[6 + j] * dr for j in range(6)]
        c = np.zeros(len(dr), dtype=np.int8)
        for j, k in ((4, CLS_LEADER), (2, CLS_1300), (1, CLS_1200), (0, CLS_1100)):
            c[ge[j] & ~ge[j + 1]] = k
        c[~(di > 0.0)] = 0
    return c


def runs_host(cls, target, window, thresh):
    """dd_sstv_runs -> int64 positions"""
    n = len(cls)
    if n < window:
        return np.zeros(0, dtype=np.int64)
    P = np.concatenate(([0], np.cumsum(np.asarray(cls) == target)))
    cnt = P[window:] - P[:n - window + 1]
    above = np.concatenate(([False], cnt >= thresh, [False]))
    starts = np.nonzero(above[1:] & ~above[:-1])[0]
    ends = np.nonzero(~above[1:] & above[:-1])[0]
    return np.array([s + int(np.argmax(cnt[s:e])) for s, e in zip(starts, ends)], dtype=np.int64)


ATAN_COEF = (1.0 / 17.0, -1.0 / 15.0, 1.0 / 13.0, -1.0 / 11.0, 1.0 / 9.0, -1.0 / 7.0, 1.0 / 5.0, -1.0 / 3.0, 1.0)
TAN_PI_8 = 0.41421356237309503


def atan_host(x, y):
    """The angle of (x, y) for y >= 0, not both zero, in [0, pi], as dd_sstv_angle forms it: t = min / max of |x| and y, above
    tan(pi / 8) u = (t - 1) / (t + 1), the arctangent's odd series to u^17 by Horner in u * u, then the three reflections."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        ax = np.where(x < 0.0, -x, x)
        swap = y > ax
        t = np.where(swap, ax, y) / np.where(swap, y, ax)
        big = t > TAN_PI_8
        u = np.where(big, (t - 1.0) / (t + 1.0), t)
        w = u * u
        p = np.full(np.shape(u), ATAN_COEF[0])
        for c in ATAN_COEF[1:]:
            p = p * w + c
        r = u * p
        r = np.where(big, 0.78539816339744828 + r, r)
        r = np.where(swap, 1.5707963267948966 - r, r)
        return np.where(x < 0.0, 3.1415926535897931 - r, r)


def _edge_host(v, n):
    with np.errstate(all="ignore"):
        c = np.ceil(v)
        return np.where(c >= 0.0, np.minimum(c, float(n)), 0.0).astype(np.int64)


def pixels_host(dr, di, t0, W, step, c1):
    """dd_sstv_pixels -> (uint8[nseg, W], empty count)"""
    n = len(dr)
    t0 = np.asarray(t0, dtype=np.float64).reshape(-1, 1)
    p = np.arange(W, dtype=np.float64).reshape(1, -1)
    a = _edge_host(t0 + p * step, n)
    b = _edge_host(t0 + (p + 1.0) * step, n)
    sr, si = np.zeros(a.shape), np.zeros(a.shape)
    with np.errstate(all="ignore"):
        for j in range(int((b - a).max()) if a.size else 0):
            m = a + j < b
            at = (a + j)[m]
            sr[m] = sr[m] + dr[at]
            si[m] = si[m] + di[at]
        none = (b <= a) | ((sr == 0.0) & (si == 0.0))
        ang = np.where(si < 0.0, 0.0, atan_host(sr, si))
        v = np.rint((ang * c1 - 1500.0) * 255.0 / 800.0)
        lv = np.where(v >= 255.0, 255.0, np.where(v > 0.0, v, 0.0))
        lv = np.where(none, 0.0, lv)
    return lv.astype(np.uint8), int(none.sum())


def color_host(levels):
    """dd_sstv_color: uint8[pairs, 4, W] -> uint8[2 pairs, W, 3]"""
    lv = np.asarray(levels).astype(np.int64)
    pairs, _, W = lv.shape
    y = np.stack((lv[:, 0], lv[:, 3]), axis=1).reshape(2 * pairs, W)
    cr, cb = np.repeat(lv[:, 1], 2, axis=0), np.repeat(lv[:, 2], 2, axis=0)
    rgb = np.stack(((100 * y + 140 * cr - 17850) // 100, (100 * y - 71 * cr - 33 * cb + 13260) // 100,
                    (100 * y + 178 * cb - 22695) // 100), axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ the host logic
def parse_vis(cls, rate):
    """Tone classes from somewhere inside a header's leader on -> None, or a dict: code, parity_ok, start_bit (index in `cls` of the
    start bit's window position).  The start bit is the first 30 ms window that is four fifths class 1200 (the 10 ms break cannot
    be) behind a window that is half leader; each of the seven data bits and the parity bit is the majority of classes 1100 and
    1300 over its middle half, which must fill half of it; the stop bit's middle half must be half class 1200.  A header that the
    end of `cls` cuts off gives None."""
    cls = np.asarray(cls)
    bit = BIT_S * rate
    wb = int(round(bit))
    if len(cls) < wb + 1:
        return None
    P = np.concatenate(([0], np.cumsum(cls == CLS_1200)))
    L = np.concatenate(([0], np.cumsum(cls == CLS_LEADER)))
    cnt = P[wb:] - P[:len(cls) - wb + 1]
    hit = np.nonzero(cnt >= math.ceil(0.8 * wb))[0]
    hit = hit[hit >= wb]
    hit = hit[2 * (L[hit] - L[hit - wb]) >= wb]
    if not len(hit):
        return None
    first = int(hit[0])
    at = first + int(np.argmax(cnt[first:first + wb]))
    bits = []
    for j in range(9):
        lo, hi = at + int((1.25 + j) * bit), at + int((1.75 + j) * bit)
        if hi > len(cls):
            return None
        seg = cls[lo:hi]
        if j == 8:
            if 2 * int((seg == CLS_1200).sum()) < hi - lo:
                return None
            break
        n1, n0 = int((seg == CLS_1100).sum()), int((seg == CLS_1300).sum())
        if 2 * max(n1, n0) < hi - lo:
            return None
        bits.append(1 if n1 > n0 else 0)
    return {"code": sum(b << j for j, b in enumerate(bits[:7])), "parity_ok": sum(bits) % 2 == 0, "start_bit": at}


def fit_grid(ks, ps, start0, period0):
    """least squares start and period of positions ps at line indices ks, in closed form; one position moves the start alone"""
    m = len(ks)
    if m == 0:
        return float(start0), float(period0)
    k, p = np.asarray(ks, dtype=np.float64), np.asarray(ps, dtype=np.float64)
    if m == 1:
        return float(p[0] - k[0] * period0), float(period0)
    km, pm = k.mean(), p.mean()
    period = float(((k - km) * (p - pm)).sum() / ((k - km) ** 2).sum())
    return float(pm - period * km), period


def match_grid(cands, start0, period0, k0, k1, tol=GRID_TOLERANCE):
    """Sync candidates (ascending) -> (ks, ps, start, period): for line k0, k0 + 1, .. k1 - 1 in turn the candidate nearest the
    prediction of the fit so far is accepted within tol * period0 of it."""
    c = [float(v) for v in np.asarray(cands, dtype=np.float64)]
    ks, ps = [], []
    start, period = float(start0), float(period0)
    m = sk = skk = sp = skp = 0.0                        # running sums of the fit, positions taken relative to start0
    j = 0
    for k in range(k0, k1):
        if not c:
            break
        pred = start + k * period
        while j < len(c) and c[j] < pred:                # c[j] becomes the first candidate at or behind the prediction
            j += 1
        while j > 0 and c[j - 1] >= pred:
            j -= 1
        near = [i for i in (j - 1, j) if 0 <= i < len(c)]
        i = min(near, key=lambda q: abs(c[q] - pred))
        if abs(c[i] - pred) <= tol * period0:
            ks.append(k)
            ps.append(c[i])
            q = c[i] - start0
            m, sk, skk, sp, skp = m + 1, sk + k, skk + k * k, sp + q, skp + k * q
            if m == 1:
                start = c[i] - k * period0
            else:
                period = (m * skp - sk * sp) / (m * skk - sk * sk)
                start = start0 + (sp - period * sk) / m
    start, period = fit_grid(ks, ps, start0, period0)
    return ks, ps, start, period


class HostOps(Laps):
    """the stages of `decode` in NumPy"""

    def lag(self, audio, hr, hi):
        return lag_host(audio, hr, hi)

    def classes(self, d, e):
        return classes_host(d[0], d[1], e)

    def runs(self, cls, target, window, thresh):
        return runs_host(cls, target, window, thresh)

    def cls_slice(self, cls, a, b):
        return cls[a:b]

    def pixels(self, d, t0, W, step, c1):
        return pixels_host(d[0], d[1], t0, W, step, c1)

    def color(self, levels, pairs, W):
        return color_host(np.asarray(levels).reshape(pairs, 4, W))


class DeviceOps(Laps):
    """the stages of `decode` on the device; `laps` collects seconds per stage, with a synchronisation after each"""

    def lag(self, audio, hr, hi):
        return lag(audio, hr, hi)

    def classes(self, d, e):
        return classes(d, e)

    def runs(self, cls, target, window, thresh):
        return runs(cls, target, window, thresh)

    def cls_slice(self, cls, a, b):
        return cls.view(a, b - a).to_host()

    def pixels(self, d, t0, W, step, c1):
        return pixels(d, t0, W, step, c1)

    def color(self, levels, pairs, W):
        return color(levels, pairs, W)


def decode(audio, rate, mode=None, ops=None):
    """The chain behind decode_sstv over `audio` (a float64 device array for DeviceOps, NumPy for HostOps) -> (images, infos): one
    uint8[rows, W, 3] and one dict per image, in stream order.  All positions below are lag-product samples; delay(K) takes them
    back to audio samples in one place, where `start` is reported."""
    ops = HostOps() if ops is None else ops
    forced = mode_of(mode)
    check_rate(rate, forced)
    n = len(audio)
    hr, hi = design(rate)
    K = len(hr)
    e = edges(rate)
    edge = sync_edge(rate)
    d = ops.lag(audio, hr, hi)
    ops.lap("lag")
    cls = ops.classes(d, e)
    ops.lap("classes")
    ws, wl = int(round(SYNC_S * rate)), int(round(LEADER_S * rate))
    syncs = ops.runs(cls, CLS_1200, ws, math.ceil(SYNC_FRACTION * ws)).astype(np.float64) + edge
    leaders = ops.runs(cls, CLS_LEADER, wl, math.ceil(LEADER_FRACTION * wl))
    ops.lap("runs")
    # headers: one parse per leader candidate over about 1 s of classes, one header per start bit
    heads = []
    for p in leaders:
        a = int(p)
        h = parse_vis(ops.cls_slice(cls, a, min(n, a + int(1.05 * rate))), rate)
        if h is None:
            continue
        h["first_sync"] = a + h["start_bit"] + edge + 10 * BIT_S * rate
        h["begin"] = h["first_sync"] - VIS_S * rate
        if not heads or h["first_sync"] - heads[-1]["first_sync"] > BIT_S * rate:
            heads.append(h)
    plans = []
    for h in heads:
        m = forced
        if m is None:
            m = BY_VIS.get(h["code"]) if h["parity_ok"] else None
            if m is None:
                logging.info("SSTV header at sample %d skipped: code %d, parity %s", int(h["begin"]), h["code"],
                             "ok" if h["parity_ok"] else "bad")
                continue
            if rate * m.pixel < 2:
                logging.info("SSTV %s image at sample %d skipped: at %r S/s its pixel of %g ms is %.3f samples, below 2",
                             m.name, int(h["first_sync"]), rate, m.pixel * 1e3, rate * m.pixel)
                continue
        # the stop bit runs into the first sync at the same tone, so line 0's sync is never matched: the header places it
        plans.append((h["first_sync"], m, h, 1))
    if forced is not None and not heads and len(syncs):
        plans.append((float(syncs[0]), forced, None, 0))
    ops.lap("headers")
    images, infos = [], []
    for start0, m, h, k0 in plans:
        later = [g["begin"] for g in heads if g["begin"] > start0]
        limit = min([n + K] + later)                  # the last K samples of the audio have no lag product: those pixels count as empty
        period0 = line_time(m) * rate
        kmax = min(m.height // 2, int((limit - start0) / period0) + 1)
        ks, ps, start, period = match_grid(syncs, start0, period0, k0, kmax)
        pairs = int(min(m.height // 2, max(0, math.floor((limit - start) / period))))
        ops.lap("grid")
        if pairs == 0:
            continue
        scale = period / period0
        offs = (SYNC_S + PORCH_S + np.arange(4) * (m.width * m.pixel)) * rate * scale
        t0 = (start + np.arange(pairs).reshape(-1, 1) * period + offs.reshape(1, -1)).ravel()
        levels, empty = ops.pixels(d, t0, m.width, m.pixel * rate * scale, rate / (2 * np.pi))
        ops.lap("pixels")
        images.append(ops.color(levels, pairs, m.width))
        ops.lap("color")
        infos.append({"mode": m.name, "vis": None if h is None else h["code"], "parity_ok": None if h is None else h["parity_ok"],
                      "start": int(np.rint(start - delay(K))), "rows": 2 * pairs, "syncs_matched": sum(1 for k in ks if k < pairs),
                      "syncs_expected": pairs, "period": period, "slant_ppm": (period / period0 - 1.0) * 1e6,
                      "empty_pixels": int(empty)})
    return images, infos


def decode_host(audio, rate, mode=None):
    """`decode` over the NumPy restatement of every stage"""
    return decode(np.ascontiguousarray(audio, dtype=np.float64).ravel(), rate, mode, HostOps())


# ------------------------------------------------------------------------------------------------------------------ the device stages
def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _need(a, dtype, what):
    if not isinstance(a, DevArray) or a.dtype != dtype:
        raise TypeError("%s: %s device array expected" % (what, dtype))


def lag(audio, hr, hi):
    """float64 device audio -> d as a complex128 device array (dd_sstv_lag)"""
    _hip.require_gpu()
    _need(audio, _F64, "sstv.lag")
    taps = np.ascontiguousarray(np.concatenate((hr, hi)), dtype=np.float64)
    d = DevArray(audio.n, _C128)
    check(lib().dd_sstv_lag(audio.ptr, audio.n, _pd(taps), len(hr), d.ptr, None), "dd_sstv_lag")
    return d


def classes(d, e):
    """d -> int8 tone classes (dd_sstv_classes)"""
    _need(d, _C128, "sstv.classes")
    e = np.ascontiguousarray(e, dtype=np.float64)
    cls = DevArray(d.n, _I8)
    check(lib().dd_sstv_classes(d.ptr, d.n, _pd(e), cls.ptr, None), "dd_sstv_classes")
    return cls


def runs(cls, target, window, thresh, cap=1024):
    """the run positions as a NumPy int64 array (dd_sstv_runs); a list that proves too small is asked for again at the true count"""
    _need(cls, _I8, "sstv.runs")
    count = C.c_int64(0)
    while True:
        pos = DevArray(max(cap, 1), np.int64)
        rc = lib().dd_sstv_runs(cls.ptr, cls.n, int(target), int(window), int(thresh), pos.ptr, cap, C.byref(count), None)
        if rc == _hip.DD_ERR_INVALID and count.value > cap:
            cap = count.value
            continue
        check(rc, "dd_sstv_runs")
        return pos.view(0, count.value).to_host()


def pixels(d, t0, W, step, c1):
    """-> (uint8 device levels [len(t0) * W], empty count) (dd_sstv_pixels)"""
    _need(d, _C128, "sstv.pixels")
    t0 = np.ascontiguousarray(t0, dtype=np.float64)
    dt0 = DevArray.from_host(t0)
    levels = DevArray(max(len(t0) * W, 1), _U8)
    empty = C.c_int64(0)
    check(lib().dd_sstv_pixels(d.ptr, d.n, dt0.ptr, len(t0), int(W), float(step), float(c1), levels.ptr, C.byref(empty), None),
          "dd_sstv_pixels")
    return levels.view(0, len(t0) * W), int(empty.value)


def color(levels, pairs, W):
    """device levels -> uint8[2 pairs, W, 3] on the host (dd_sstv_color)"""
    _need(levels, _U8, "sstv.color")
    rgb = DevArray(max(pairs * 2 * W * 3, 1), _U8)
    check(lib().dd_sstv_color(levels.ptr, int(pairs), int(W), rgb.ptr, None), "dd_sstv_color")
    return rgb.view(0, pairs * 2 * W * 3).to_host().reshape(2 * pairs, W, 3)
