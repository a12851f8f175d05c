"""
What the Meteor-M2 QPSK and the Funcube BPSK sync detectors share (the reference's decode_meteorm2.py and decode_funcube.py define
lim, limBin, agc, costas and the Gardner loop alike; device side: dd_symbol_walk.h): the reference's helpers restated, the symbol
walk (`Walker`, which qpsk.Walker and bpsk.Walker configure), offsetFreq in the reference's arithmetic (`mix`), the plumbing of the
two modules' MINSYNC and MAXSYNC stages, and the decode pass of the two decoder classes (`SyncDecoder`).
"""
import ctypes as C
import logging

import numpy as np

from . import _hip, chunker, comm
from ._burst import Laps
from ._hip import DevArray, check, lib


def lim(x):
    """decode_meteorm2.lim / decode_funcube.lim: clamp to [-128, 127], (0, 1) -> 1, (-1, 0) -> -1, else int(x)"""
    if x < -128.0:
        return -128
    if x > 127.0:
        return 127
    if x > 0 and x < 1:
        return 1
    if x > -1 and x < 0:
        return -1
    return int(x)


def limBin(x):
    """decode_meteorm2.limBin / decode_funcube.limBin: 0 for x <= 0, else 1"""
    if x <= 0:
        return 0
    else:
        return 1


def costas_coefficients(bw, damping=0.70710678118):
    """costas.compAlphaBeta for bw and bw / 2: (alpha, beta, alpha_locked, beta_locked)"""
    def ab(d, b):
        denom = (1.0 + 2.0 * d * b + b * b)
        return (4 * d * b) / denom, (4 * b * b) / denom
    return ab(damping, bw) + ab(damping, bw / 2.0)


def hyp_table():
    """costas.hypstore: np.tanh(i - 128) for i in 0..255"""
    return np.array([np.tanh(i - 128) for i in range(256)], dtype=np.float64)


# DDMeteorState (dd_symbol_walk.h)
_STATE = np.dtype([(f, np.float64) for f in ("timing", "b_re", "b_im", "c_re", "c_im", "dc_re", "dc_im", "amean", "freq", "phase",
                                             "pmean", "alpha", "beta")] + [(f, np.int64) for f in ("lock", "ctr", "bidx", "overflow")])


class Walker:
    """The symbol walk over a recording of `total` samples at `fs`, fed chunk by chunk in order (`walk`, then `lim`).  Per symbol k (device
    arrays, `nsym` long once fed): bidx, aidx (sample indices of the B and A samples), agc (agc.adjust of A, gardnerC), ph (the
    costas phasor the symbol was corrected with: pllObj.output after the step), sym (the corrected symbol, gardnerA after
    pllObj.loop), pf ((phase, freq) after the step); `lim_values` = one LIM_DTYPE entry for every sample fed.

    Device memory: room for total / (P / 2) symbols -- twice the nominal count -- at 96 B each, plus the lim values.  A recording
    whose timing runs faster than one symbol per P / 2 samples (the reference would keep decoding) raises RuntimeError.

    A subclass states the modulation: SYMBOL_RATE, COSTAS_BW (the loop's bandwidth, unlocked), AMEAN0 (agc's initial mean),
    LIM_DTYPE (int16 = an int8 (re, im) pair per sample, int8 = re alone), WALK and LIM (its C entry points' names), LABEL (for
    error messages)."""

    @classmethod
    def leading_params(cls, fs):
        """the seven doubles DDMeteorParams starts with: symbolPeriod P, P / 2, P / 2 + 1, then costas_coefficients"""
        P = fs / cls.SYMBOL_RATE
        return [P, P / 2, (P / 2) + 1] + list(costas_coefficients(cls.COSTAS_BW))

    def __init__(self, fs, total):
        _hip.require_gpu()
        lead = self.leading_params(fs)
        halfP, a0, b0 = lead[1], lead[3], lead[4]
        self.params = np.ascontiguousarray(np.concatenate((lead, hyp_table())), dtype=np.float64)
        st = np.zeros(1, dtype=_STATE)
        st["amean"], st["freq"], st["pmean"], st["alpha"], st["beta"] = self.AMEAN0, 0.001, 1.0, a0, b0
        self.state = DevArray.from_host(st.view(np.uint8))
        self.total = int(total)
        self.cap = int(total / halfP) + 64               # a symbol takes at least P/2 samples unless timing is thrown far
        cap = max(self.cap, 1)
        self.bidx, self.aidx = DevArray(cap, np.int64), DevArray(cap, np.int64)
        self.agc, self.ph, self.sym, self.pf = (DevArray(cap, np.complex128) for _ in range(4))
        self.lim_values = DevArray(max(self.total, 1), self.LIM_DTYPE)
        self.fed = self.nsym = 0

    def walk(self, x):
        """the symbol walk over the next chunk"""
        if x.dtype != np.dtype(np.complex128):
            raise TypeError("complex128 device array expected, got %s" % x.dtype)
        if self.fed + x.n > self.total:
            raise ValueError("more samples than the recording holds")
        check(getattr(lib(), self.WALK)(x.ptr, x.n, self.fed, self.state.ptr, self.params.ctypes.data_as(C.POINTER(C.c_double)),
                                        self.cap, self.bidx.ptr, self.aidx.ptr, self.agc.ptr, self.ph.ptr, self.sym.ptr, self.pf.ptr,
                                        None), self.WALK)
        st = self.state.to_host().view(_STATE)[0]
        if st["overflow"]:
            raise RuntimeError("%s walk: more symbols than %d (timing thrown by the input)" % (self.LABEL, self.cap))
        self.nsym = int(st["ctr"])

    def lim(self, x):
        """the lim values of the chunk just walked (its samples take the phasors of the symbols walked so far)"""
        check(getattr(lib(), self.LIM)(x.ptr, x.n, self.fed, self.aidx.ptr, self.nsym, self.ph.ptr, self.lim_values.ptr, self.total,
                                       None), self.LIM)
        self.fed += x.n

    def view(self, name):
        return getattr(self, name).view(0, self.nsym)


def iq_pointers(x):
    """(raw_u8, c64) arguments of a mixer entry point for a device array of raw u8 pairs (_hip.IQ8) or complex64"""
    if x.dtype == _hip.IQ8:
        return x.ptr, None
    if x.dtype == np.dtype(np.complex64):
        return None, x.ptr
    raise TypeError("raw u8 pairs or complex64 expected, got %s" % x.dtype)


def mix(x, fs, offset):
    """commSignal.offsetFreq(offset) with the reference's arithmetic (dd_meteor_mix): raw u8 pairs (_hip.IQ8) or complex64 in,
    complex64 out.  The reference restarts the mixer phase in every chunk (no chunker reaches the signal), so k counts from 0."""
    raw, c64 = iq_pointers(x)
    out = DevArray(x.n, np.complex64)
    w = -1.0j * 2.0 * np.pi * offset                     # comm.py:77's operation order: the imaginary part is -2 pi f
    check(lib().dd_meteor_mix(raw, c64, x.n, float(w.imag), 1.0 / fs, out.ptr, None), "dd_meteor_mix")
    return out


def minsync_fired(entry, w, sync, width, cap, what):
    """One MINSYNC entry point over the walker's symbols -> (the firing windows as int64[m, width] sorted by their first column, the
    symbol index; the device array of the symbols' bits).  More than `cap` of them raise, named by `what` (a format of the count)."""
    bits = DevArray(max(w.nsym, 1), np.uint8)
    if w.nsym == 0:
        return np.zeros((0, width), dtype=np.int64), bits
    sb = np.ascontiguousarray(sync, dtype=np.uint8)
    cand = DevArray(width * cap, np.int64)
    cnt = DevArray(1, np.uint64)
    check(getattr(lib(), entry)(w.sym.ptr, w.nsym, sb.ctypes.data, bits.ptr, cap, cand.ptr, cnt.ptr, None), entry)
    m = int(cnt.to_host()[0])
    if m > cap:
        raise RuntimeError("%s, more than %d" % (what % m, cap))
    c = cand.view(0, width * m).to_host().reshape(m, width) if m else np.zeros((0, width), dtype=np.int64)
    return c[np.argsort(c[:, 0], kind="stable")], bits


def interval_descriptors(bufs, fifth):
    """correlation buffers [(intervals [(lo, n), ...], ...)] -> int64[n, 5] = (lo0, n0, lo1, n1, fifth(buffer, n0 + n1)), the
    device's DDMeteorBuf / DDFuncubeBuf"""
    desc = np.zeros((len(bufs), 5), dtype=np.int64)
    for i, buf in enumerate(bufs):
        ivs = list(buf[0])
        if len(ivs) > 2:
            raise ValueError("a correlation buffer spans at most two sample intervals")
        (lo0, n0), (lo1, n1) = (ivs + [(0, 0)])[:2]
        desc[i] = (lo0, n0, lo1, n1, fifth(buf, n0 + n1))
    return desc


def maxcorr(entry, lim_values, desc, *args):
    """One MAXSYNC entry point over the buffer descriptors (and its own arguments): int64[n, 2] = each buffer's (argmax, max)"""
    n = len(desc)
    if n == 0:
        return np.zeros((0, 2), dtype=np.int64)
    d = DevArray(2 * n, np.int64)
    check(getattr(lib(), entry)(lim_values.ptr, lim_values.n, desc.ctypes.data, n, *args, d.ptr, None), entry)
    return d.to_host().reshape(n, 2)


class SyncDecoder:
    """One decode pass, cached, behind `useful`, `getSyncs`, `getSymbols` and `walker`: per chunk of the recording (the reference's
    chunker) the subclass's front end, then the symbol walk and the per-sample lim values; after the last chunk its sync search.
    Left on the object: timings (seconds per stage of the last decode: STAGES, walk and lim summed over chunks, minsync, maxsync),
    minsyncs, buffers (per MAXSYNC correlation: (intervals [(first sample, count)], maxBuffStart, ...)), argmax (of each |correlation|).

    A subclass states WALKER (its Walker class), STAGES (its front end's timer names) and SPACING (two MAXSYNCs' nominal distance and
    its tolerance, in seconds) and supplies _front_end(src, ck, lap), once before the chunks, -> f(number, a, b, d): chunk `number` =
    samples [a, b), read as the device array d (raw u8 pairs or complex64), to the walk's complex128 input, lapping STAGES;
    _sync_search(w, total, a_at, lap), once after them (a_at(k) = the sample of symbol k's A), -> (minsyncs, buffers, int64[n, 2] =
    each buffer's (argmax, max)), lapping minsync and maxsync; _position(start, arg) -> a MAXSYNC's sample position."""

    def __init__(self, sigsrc, use_device_raw):
        self._sigsrc = sigsrc
        self._use_raw = use_device_raw
        self._useful = 0
        self._result = None
        self.timings, self.minsyncs, self.buffers, self.argmax = {}, [], [], []

    @property
    def useful(self):
        """1 if two MAXSYNCs lie SPACING[0] +- SPACING[1] seconds apart, else 0 (0 until getSyncs has run)"""
        return self._useful

    @property
    def getSyncs(self):
        """The MAXSYNC sample positions but the first"""
        return list(self._decode()[0])

    @property
    def getSymbols(self):
        """The PLL-corrected soft symbols as a device-resident commSignal at the symbol rate"""
        return comm.commSignal(self.WALKER.SYMBOL_RATE, self._decode()[1])

    def walker(self):
        """the symbol walk of the last decode (per-symbol device arrays)"""
        return self._decode()[2]

    def _decode(self):
        if self._result is not None:
            return self._result
        _hip.require_gpu()
        src = self._sigsrc
        t = dict.fromkeys(tuple(self.STAGES) + ("walk", "lim"), 0.0)
        lap = Laps(t).lap
        ck = chunker.chunker(src)
        read = src.read
        if self._use_raw and hasattr(src, "read_device_raw") and src.length > 0 and src.read_device_raw(0, 1) is not None:
            read = src.read_device_raw
        front = self._front_end(src, ck, lap)
        w = self.WALKER(src.sampFreq, src.length)
        for number, (a, b) in enumerate(ck.getChunks):
            if b <= a:
                continue
            d = read(a, b)
            if not isinstance(d, _hip.DevArray):
                d = _hip.DevArray.from_host(np.asarray(d), dtype=np.complex64)
            x = front(number, a, b, d)
            w.walk(x)
            lap("walk")
            w.lim(x)
            lap("lim")
        aidx = w.aidx

        def a_at(k):
            return int(aidx.view(k, 1).to_host()[0])
        minsyncs, bufs, am = self._sync_search(w, src.length, a_at, lap)
        self.timings = t
        maxSyncs = []
        for buf, (arg, _) in zip(bufs, am):
            v = self._position(buf[1], arg)
            logging.info("MAXSYNC %d", v)
            maxSyncs.append(v)
        self.minsyncs = minsyncs
        self.buffers = bufs
        self.argmax = [int(a) for a in am[:, 0]]
        syncs = []
        if len(maxSyncs) > 1:
            if np.min(np.abs(np.diff(maxSyncs) - (self.SPACING[0] * 2048000))) < (self.SPACING[1] * 2048000):
                self._useful = 1
            syncs = list(maxSyncs)[1:]
        self._result = (syncs, w.view("sym"), w)
        return self._result
