"""
OQPSK symbol recovery from IQ samples for the Meteor-M N2-x satellites (where the loop is defined operation
by operation; device side: dd_oqpsk.h).  The transmitter sends I(t) + j Q(t - T/2); the walk reads the I rail at its A events and the
Q rail at the B events half a period later, runs the Gardner detector on both rails of the derotated samples and a Costas loop whose
phase is kept in turns, all in one serial chain that calls no libm function: the phasor comes from `phasor_table` and two short
polynomials.  Here: the table, its NumPy restatement (`phasor_np`), the walk's parameters and state, and `Walker`.
"""
import ctypes as C

import numpy as np

from . import _hip
from ._hip import DevArray, check, lib
from .symbolsync import costas_coefficients, hyp_table

TABLE_N = 1024
COSTAS_BW = 0.008727                # rad per symbol, unlocked; halved when locked
AMEAN0 = 3.0                        # agc.adjust's mean at the start
FREQ0 = 0.001 / (2.0 * np.pi)       # the carrier loop's frequency at the start, turns per symbol
SYMBOL_RATES = (72000, 80000)

# DDOqpskState (dd_oqpsk.h)
STATE = np.dtype([(f, np.float64) for f in ("timing", "dc_re", "dc_im", "amean", "u", "freq", "pmean", "alpha", "beta", "i_k", "i_prev",
                                            "i_mid", "q_prev", "q_mid", "e_q")]
                 + [(f, np.int64) for f in ("lock", "ctr", "aidx", "seen_a", "overflow")])


def phasor_table():
    """(cos, sin)(2 pi i / 1024), float64[1024, 2]"""
    a = 2.0 * np.pi * np.arange(TABLE_N) / TABLE_N
    return np.stack((np.cos(a), np.sin(a)), axis=1)


def phasor_np(u, table=None):
    """The walk's phasor of the phases u (turns, in [0, 1)) -> complex128 (cos + j sin)(2 pi u): entry i = int(u N) of the table
    rotated by d = (u N - i) (2 pi / N) through 1 - d^2/2 + d^4/24 and d - d^3/6 + d^5/120, in the device's operation order"""
    tab = phasor_table() if table is None else np.asarray(table, dtype=np.float64)
    t = np.asarray(u, dtype=np.float64) * 1024.0
    i = np.where(t >= 0.0, np.minimum(t, 1023.0), 0.0).astype(np.int64)
    d = (t - i) * (6.283185307179586 / 1024.0)
    d2 = d * d
    pc = 1.0 - d2 * (0.5 - d2 * (1.0 / 24.0))
    ps = d * (1.0 - d2 * ((1.0 / 6.0) - d2 * (1.0 / 120.0)))
    tc, ts = tab[i, 0], tab[i, 1]
    return (tc * pc - ts * ps) + 1j * (ts * pc + tc * ps)


def leading_params(fs, symbol_rate):
    """the seven doubles DDMeteorParams starts with: P, P / 2, P / 2 + 1, then the loop gains (unlocked, locked) in turns"""
    P = fs / symbol_rate
    return [P, P / 2, (P / 2) + 1] + [v / 6.283185307179586 for v in costas_coefficients(COSTAS_BW)]


class Walker:
    """The OQPSK walk over a recording of `total` samples at `fs`, fed chunk by chunk in order (`walk`).  Per symbol k (device arrays,
    `nsym` long once fed): bidx, aidx (the samples its Q rail and its I rail were read at), sym (complex128 I + jQ), uf ((phase in
    turns, frequency in turns per symbol) after its step).  Room for total / (P / 2) symbols, 48 B each; a recording whose timing
    runs faster than that raises RuntimeError."""

    def __init__(self, fs, total, symbol_rate=72000):
        _hip.require_gpu()
        if symbol_rate not in SYMBOL_RATES:
            raise ValueError("oqpsk.Walker: a symbol rate of %s expected, got %r" % (" or ".join(map(str, SYMBOL_RATES)), symbol_rate))
        self.symbol_rate = symbol_rate
        lead = leading_params(fs, symbol_rate)
        self.params = np.ascontiguousarray(np.concatenate((lead, hyp_table())), dtype=np.float64)
        st = np.zeros(1, dtype=STATE)
        st["amean"], st["freq"], st["pmean"], st["alpha"], st["beta"] = AMEAN0, FREQ0, 1.0, lead[3], lead[4]
        self.state = DevArray.from_host(st.view(np.uint8))
        self.table = DevArray.from_host(np.ascontiguousarray(phasor_table()).ravel())
        self.total = int(total)
        self.cap = int(total / lead[1]) + 64
        cap = max(self.cap, 1)
        self.bidx, self.aidx = DevArray(cap, np.int64), DevArray(cap, np.int64)
        self.sym, self.uf = DevArray(cap, np.complex128), DevArray(cap, np.complex128)
        self.fed = self.nsym = 0

    def walk(self, x):
        """the walk over the next chunk (complex128 device array)"""
        if x.dtype != np.dtype(np.complex128):
            raise TypeError("complex128 device array expected, got %s" % x.dtype)
        if self.fed + x.n > self.total:
            raise ValueError("more samples than the recording holds")
        check(lib().dd_oqpsk_walk(x.ptr, x.n, self.fed, self.state.ptr, self.params.ctypes.data_as(C.POINTER(C.c_double)),
                                  self.table.ptr, self.cap, self.bidx.ptr, self.aidx.ptr, self.sym.ptr, self.uf.ptr, None),
              "dd_oqpsk_walk")
        st = self.host_state()
        if st["overflow"]:
            raise RuntimeError("oqpsk walk: more symbols than %d (timing thrown by the input)" % self.cap)
        self.nsym = int(st["ctr"])
        self.fed += x.n

    def host_state(self):
        """the carried state as one STATE record"""
        return self.state.to_host().view(STATE)[0]

    def view(self, name):
        return getattr(self, name).view(0, self.nsym)
