"""
Funcube BPSK sync detection stages -- the reference's decode_funcube.getSyncs (decode_funcube.py:148-306), a Python loop over every
IQ sample there.  Device stages (dd_funcube.h; what the Meteor-M2 decoder shares is in symbolsync.py and dd_symbol_walk.h): the
Gardner / agc / costas walk (`Walker`, configured here), the per-sample lim values (`Walker.lim`),
the MINSYNC list (`minsync_list`), the MAXSYNC correlations (`maxsync_argmax`), the mixer with the Doppler ramp (`mix_ramp`) and
the low-pass in scipy.signal.lfilter's own operation order (`Lowpass`).
Host stages: the correlation-buffer bookkeeping (`maxsync_buffers`), O(syncs); NumPy restatements of the device arithmetic (`lim`,
`limBin`, `correlate_same_blocks`) for the tests.
"""
import ctypes as C
import math

import numpy as np

from . import symbolsync
from ._hip import DevArray, check, lib
from .symbolsync import hyp_table, lim, limBin, mix  # noqa: F401  (the names this module has always offered; mix is offsetFreq)
from .symbolsync import interval_descriptors, iq_pointers, maxcorr, minsync_fired

SYMBOL_RATE = 12000
SYNC = "101000110001000000000001010111100"
NSYNC = len(SYNC)
SYMS = 10                               # symbols per sync bit (np.repeat(sync, 10), decode_funcube.py:172)
WIN = NSYNC * SYMS                      # len(sync12khz)
REP = int(2048000 / 1200)               # np.repeat count of the 2 MHz template (decode_funcube.py:176), whatever the rate
TLEN = NSYNC * REP                      # len(sync2mhz) = 56298
RETAIN = 2 * TLEN                       # the countdown every MINSYNC starts, and the length the idle buffer slides at
COSTAS_BW = 0.05235833333 * 6


def sync_bits():
    """the 33 sync bits as an int64 0/1 array (decode_funcube.py:170)"""
    return np.array([int(i) for i in SYNC], dtype=np.int64)


def sync12khz():
    return np.repeat(sync_bits(), SYMS)


def template_bits():
    """sync2mhz before np.repeat: 127 / -128 per bit (decode_funcube.py:174-175)"""
    return np.where(sync_bits() == 1, 127, -128).astype(np.int64)


def correlate_same_blocks(buf, t, rep=REP):
    """np.correlate(buf, np.repeat(t, rep), 'same') for len(buf) >= len(t) * rep through a prefix sum of the buffer: len(t) block
    sums per lag (what dd_funcube_maxcorr computes, in NumPy integers)"""
    buf = np.asarray(buf, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    L, left = len(buf), (len(t) * rep) // 2
    S = np.concatenate(([0], np.cumsum(buf)))
    e = np.arange(L)[:, None] - left + rep * np.arange(len(t) + 1)[None, :]
    W = S[np.clip(e, 0, L)]
    return (W[:, 1:] - W[:, :-1]) @ t


def costas_coefficients():
    """costas.compAlphaBeta for bw and bw / 2: (alpha, beta, alpha_locked, beta_locked)"""
    return symbolsync.costas_coefficients(COSTAS_BW)


class Lowpass:
    """sig.filter(filters.butter(fs, bw)) of decode_funcube.py:160,230 on complex64 device samples, complex128 out, the state carried
    from call to call: scipy.signal.lfilter's recurrence sample by sample in its operation order (dd_funcube_lowpass), so the output
    is lfilter's bit for bit.  filters.butter's own device path (dd_iir_c64) is block-parallel and 5.6e-6 off lfilter at the default
    7 kHz / 2.048 MS/s, which moves Gardner decisions."""

    def __init__(self, fs, bw):
        import scipy.signal as signal     # coefficient design and lfilter_zi only
        from . import filters
        f = filters.butter(fs, bw)
        self.b = np.ascontiguousarray(f.getB, dtype=np.float64)
        self.a = np.ascontiguousarray(f.getA, dtype=np.float64)
        zi = signal.lfilter_zi(self.b, self.a)          # used unscaled by the reference (filters.py:45); a real zi seeds the real parts
        self.zi = np.concatenate((zi, np.zeros(len(zi))))
        self.state = None

    def apply(self, x):
        if x.dtype != np.dtype(np.complex64):
            raise TypeError("complex64 device array expected, got %s" % x.dtype)
        if self.state is None:
            self.state = DevArray.from_host(self.zi)
        out = DevArray(x.n, np.complex128)
        dp = C.POINTER(C.c_double)
        check(lib().dd_funcube_lowpass(x.ptr, out.ptr, x.n, self.b.ctypes.data_as(dp), self.a.ctypes.data_as(dp), len(self.b),
                                       self.state.ptr, None), "dd_funcube_lowpass")
        return out


class Walker(symbolsync.Walker):
    """symbolsync.Walker for decode_funcube: `lim_values` = the int8 real part of every sample fed.  Device memory: about 1.4 GB of
    symbols and 1.2 GB of lim values for a 10-minute pass at 2.048 MS/s."""
    SYMBOL_RATE = SYMBOL_RATE
    COSTAS_BW = COSTAS_BW
    AMEAN0 = 180.0
    LIM_DTYPE = np.int8
    WALK, LIM = "dd_funcube_walk", "dd_funcube_lim"
    LABEL = "funcube"


def mix_ramp(x, fs, rmp):
    """commSignal.offsetFreq(doppCorrect_freqs) with the reference's arithmetic, the frequencies formed in the kernel from a
    frequency_shift.ramp (dd_funcube_mix_ramp): raw u8 pairs (_hip.IQ8) or complex64 in, complex64 out, k counting from 0"""
    raw, c64 = iq_pointers(x)
    if rmp.n != x.n:
        raise ValueError("a ramp of %d samples for a chunk of %d" % (rmp.n, x.n))
    out = DevArray(x.n, np.complex64)
    w = -1.0j * 2.0 * np.pi                              # comm.py:77's operation order: (-2 pi) * f[k], then * k, then / fs
    check(lib().dd_funcube_mix_ramp(raw, c64, x.n, float(w.imag), float(rmp.start), float(rmp.delta), float(rmp.target), 1.0 / fs,
                                    out.ptr, None), "dd_funcube_mix_ramp")
    return out


def minsync_list(w, cap=1 << 20):
    """symbols k >= 329 whose 330-symbol window fires: int64[m, 2] = (k, mismatches), sorted by k (the reference's ctr is k + 1)"""
    return minsync_fired("dd_funcube_minsync", w, sync_bits(), 2, cap, "funcube MINSYNC: %d firing windows")[0]


def maxsync_buffers(ks, total, a_at, nsym):
    """The MAXSYNC buffer bookkeeping (decode_funcube.py:240-261) for the MINSYNC symbols `ks` (ascending; the reference's ctr is
    k + 1): a_at(k) = the sample of symbol k's A (k < nsym).  -> per correlation that runs: (intervals [(lo, n), ...], maxBuffStart).

    A sample s sees ctr = #{k : a_at(k) < s}.  The MINSYNC at sample s = a_at(k) re-arms lastMin = k + 1 and the countdown, so the
    samples s + 1 .. s + RETAIN + 1 are appended untrimmed and the last of them runs the correlation, unless a further MINSYNC
    falls on one of the first RETAIN of them and starts the count again.  With no countdown running, samples with
    lastMin + 4.9 * 12000 - 660 < ctr <= lastMin + 5.2 * 12000 are collected, trimmed to the last RETAIN; when that span passes
    without a MINSYNC the stale window stays, with its start, and the next MINSYNC's samples are appended to it."""
    out = []
    prev_m = None
    i = 0
    ks = [int(k) for k in ks]
    while i < len(ks):
        s_first = int(a_at(ks[i]))
        s_last = s_first
        while i + 1 < len(ks) and int(a_at(ks[i + 1])) <= s_last + RETAIN:
            i += 1
            s_last = int(a_at(ks[i]))
        pre = []
        if prev_m is not None:
            cmin = math.floor(prev_m + (4.9 * 12000) - (2 * WIN)) + 1        # the first ctr above the collect threshold
            cmax = math.floor(prev_m + (5.2 * 12000))                        # the last ctr not above the span's end
            if cmin - 1 < nsym:
                j0 = int(a_at(cmin - 1)) + 1
                ce = min(s_first, int(a_at(cmax))) if cmax < nsym else s_first
                lo = max(j0, ce - RETAIN + 1)
                if ce >= lo:
                    pre = [(lo, ce - lo + 1)]
        e = s_last + RETAIN + 1                                             # the sample where maxBuffRetain reads 0
        if e >= total:
            break
        ivs = pre + [(s_first + 1, e - s_first)]
        if len(ivs) == 2 and ivs[0][0] + ivs[0][1] == ivs[1][0]:
            ivs = [(ivs[0][0], ivs[0][1] + ivs[1][1])]
        out.append((ivs, ivs[0][0]))
        prev_m = ks[i] + 1
        i += 1
    return out


def maxsync_argmax(lim_values, bufs, rep=REP):
    """[(intervals, start)] -> int64[n, 2] = (argmax, max) of |np.correlate(buffer, np.repeat(template, rep), 'same')| on the
    device; the buffers' int32 prefix sums live in one scratch device array for the call (4 B per buffer entry)"""
    off = 0

    def scratch_offset(_, length):
        nonlocal off
        if length < NSYNC * rep:
            raise ValueError("a correlation buffer of %d samples is shorter than the template (%d)" % (length, NSYNC * rep))
        at, off = off, off + length + 1
        return at
    desc = interval_descriptors(bufs, scratch_offset)
    sb = np.ascontiguousarray(sync_bits(), dtype=np.uint8)
    scratch = DevArray(max(off, 1), np.int32)
    return maxcorr("dd_funcube_maxcorr", lim_values, desc, sb.ctypes.data, int(rep), scratch.ptr, off)
