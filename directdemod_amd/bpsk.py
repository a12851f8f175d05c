"""
Funcube BPSK sync detection stages -- the reference's decode_funcube.getSyncs (decode_funcube.py:148-306), a Python loop over every
IQ sample there.  Device stages (dd_funcube.h): the Gardner / agc / costas walk (`Walker`), the per-sample lim values (`Walker.lim`),
the MINSYNC list (`minsync_list`), the MAXSYNC correlations (`maxsync_argmax`), the mixer with the Doppler ramp (`mix_ramp`) and
the low-pass in scipy.signal.lfilter's own operation order (`Lowpass`).
Host stages: the correlation-buffer bookkeeping (`maxsync_buffers`), O(syncs); NumPy restatements of the device arithmetic (`lim`,
`limBin`, `correlate_same_blocks`) for the tests.
"""
import ctypes as C
import math

import numpy as np

from . import _hip, qpsk
from ._hip import DevArray, check, lib
from .qpsk import hyp_table, lim, limBin, mix  # noqa: F401  (the reference's two decoders define these alike; mix is offsetFreq)

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
    return qpsk.costas_coefficients(bw=COSTAS_BW)


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


class Walker:
    """The symbol walk over a recording of `total` samples at `fs`, fed chunk by chunk in order (`walk`, then `lim`).  Per symbol k (device
    arrays, `nsym` long once fed): bidx, aidx (sample indices of the B and A samples), agc (agc.adjust of A, gardnerC), ph (the
    costas phasor the symbol was corrected with: pllObj.output after the step), sym (the corrected symbol, gardnerA after
    pllObj.loop), pf ((phase, freq) after the step); `lim_values` = the int8 of every sample fed.

    Device memory: room for total / (P / 2) symbols -- twice the nominal count -- at 96 B each, plus 1 B per sample of lim values:
    about 1.4 GB and 1.2 GB for a 10-minute pass at 2.048 MS/s.  A recording whose timing runs faster than one symbol per P / 2
    samples (the reference would keep decoding) raises RuntimeError."""

    def __init__(self, fs, total):
        _hip.require_gpu()
        P = fs / 12000
        a0, b0, a1, b1 = costas_coefficients()
        self.params = np.ascontiguousarray(np.concatenate(([P, P / 2, (P / 2) + 1, a0, b0, a1, b1], hyp_table())), dtype=np.float64)
        st = np.zeros(1, dtype=qpsk._STATE)
        st["amean"], st["freq"], st["pmean"], st["alpha"], st["beta"] = 180.0, 0.001, 1.0, a0, b0
        self.state = DevArray.from_host(st.view(np.uint8))
        self.total = int(total)
        self.cap = int(total / (P / 2)) + 64             # a symbol takes at least P/2 samples unless timing is thrown far
        cap = max(self.cap, 1)
        self.bidx, self.aidx = DevArray(cap, np.int64), DevArray(cap, np.int64)
        self.agc, self.ph, self.sym, self.pf = (DevArray(cap, np.complex128) for _ in range(4))
        self.lim_values = DevArray(max(self.total, 1), np.int8)
        self.fed = 0
        self.nsym = 0

    def _state(self):
        return self.state.to_host().view(qpsk._STATE)[0]

    def walk(self, x):
        """the symbol walk over the next chunk"""
        if x.dtype != np.dtype(np.complex128):
            raise TypeError("complex128 device array expected, got %s" % x.dtype)
        if self.fed + x.n > self.total:
            raise ValueError("more samples than the recording holds")
        dp = C.POINTER(C.c_double)
        check(lib().dd_funcube_walk(x.ptr, x.n, self.fed, self.state.ptr, self.params.ctypes.data_as(dp), self.cap,
                                    self.bidx.ptr, self.aidx.ptr, self.agc.ptr, self.ph.ptr, self.sym.ptr, self.pf.ptr, None),
              "dd_funcube_walk")
        st = self._state()
        if st["overflow"]:
            raise RuntimeError("funcube walk: more symbols than %d (timing thrown by the input)" % self.cap)
        self.nsym = int(st["ctr"])

    def lim(self, x):
        """the lim values of the chunk just walked (its samples take the phasors of the symbols walked so far)"""
        check(lib().dd_funcube_lim(x.ptr, x.n, self.fed, self.aidx.ptr, self.nsym, self.ph.ptr, self.lim_values.ptr, self.total, None),
              "dd_funcube_lim")
        self.fed += x.n

    def view(self, name):
        return getattr(self, name).view(0, self.nsym)


def mix_ramp(x, fs, rmp):
    """commSignal.offsetFreq(doppCorrect_freqs) with the reference's arithmetic, the frequencies formed in the kernel from a
    frequency_shift.ramp (dd_funcube_mix_ramp): raw u8 pairs (_hip.IQ8) or complex64 in, complex64 out, k counting from 0"""
    if x.dtype == _hip.IQ8:
        raw, c64 = x.ptr, None
    elif x.dtype == np.dtype(np.complex64):
        raw, c64 = None, x.ptr
    else:
        raise TypeError("raw u8 pairs or complex64 expected, got %s" % x.dtype)
    if rmp.n != x.n:
        raise ValueError("a ramp of %d samples for a chunk of %d" % (rmp.n, x.n))
    out = DevArray(x.n, np.complex64)
    w = -1.0j * 2.0 * np.pi                              # comm.py:77's operation order: (-2 pi) * f[k], then * k, then / fs
    check(lib().dd_funcube_mix_ramp(raw, c64, x.n, float(w.imag), float(rmp.start), float(rmp.delta), float(rmp.target), 1.0 / fs,
                                    out.ptr, None), "dd_funcube_mix_ramp")
    return out


def minsync_list(w, cap=1 << 20):
    """symbols k >= 329 whose 330-symbol window fires: int64[m, 2] = (k, mismatches), sorted by k (the reference's ctr is k + 1)"""
    nsym = w.nsym
    if nsym == 0:
        return np.zeros((0, 2), dtype=np.int64)
    bits = DevArray(nsym, np.uint8)
    sb = np.ascontiguousarray(sync_bits(), dtype=np.uint8)
    cand = DevArray(2 * cap, np.int64)
    cnt = DevArray(1, np.uint64)
    check(lib().dd_funcube_minsync(w.sym.ptr, nsym, sb.ctypes.data, bits.ptr, cap, cand.ptr, cnt.ptr, None), "dd_funcube_minsync")
    m = int(cnt.to_host()[0])
    if m > cap:
        raise RuntimeError("funcube MINSYNC: %d firing windows, more than %d" % (m, cap))
    c = cand.view(0, 2 * m).to_host().reshape(m, 2) if m else np.zeros((0, 2), dtype=np.int64)
    return c[np.argsort(c[:, 0], kind="stable")]


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
    n = len(bufs)
    out = np.zeros((n, 2), dtype=np.int64)
    if n == 0:
        return out
    desc = np.zeros((n, 5), dtype=np.int64)
    off = 0
    for i, (ivs, _) in enumerate(bufs):
        if len(ivs) > 2:
            raise ValueError("a correlation buffer spans at most two sample intervals")
        (lo0, n0), (lo1, n1) = (list(ivs) + [(0, 0)])[:2]
        if n0 + n1 < NSYNC * rep:
            raise ValueError("a correlation buffer of %d samples is shorter than the template (%d)" % (n0 + n1, NSYNC * rep))
        desc[i] = (lo0, n0, lo1, n1, off)
        off += n0 + n1 + 1
    sb = np.ascontiguousarray(sync_bits(), dtype=np.uint8)
    scratch = DevArray(off, np.int32)
    d = DevArray(2 * n, np.int64)
    check(lib().dd_funcube_maxcorr(lim_values.ptr, lim_values.n, desc.ctypes.data, n, sb.ctypes.data, int(rep), scratch.ptr, off,
                                   d.ptr, None), "dd_funcube_maxcorr")
    return d.to_host().reshape(n, 2)
