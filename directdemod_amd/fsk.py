"""
G3RUH 9600 baud FSK on the device (where the loop is defined operation by operation; device side:
dd_fsk.h): the bit-timing walk over FM-demodulated audio (`walk`), and the hard decision, the descrambler 1 + x^12 + x^17 and the
NRZI decoding behind it (`bit_stream`), which hands afsk.frames the same BitStream the AFSK1200 slicer does.  `scramble` and
`descramble` are the line code in NumPy, for users and tests.
"""
import ctypes as C

import numpy as np

from . import _hip, afsk
from ._hip import DevArray, check, lib

BAUDRATE = 9600
GAIN = 0.1                          # the timing loop's gain g
AM0 = 1.0                           # the mean |y| at the start
P_MIN, P_MAX = 2.0, 64.0            # samples per symbol the walk accepts
TAPS = (12, 17)                     # the scrambler polynomial 1 + x^12 + x^17

# DDFskState (dd_fsk.h)
STATE = np.dtype([(f, np.float64) for f in ("t", "dc", "am", "prev", "mid", "last")] + [(f, np.int64) for f in ("ctr", "overflow")])

_F64 = np.dtype(np.float64)
_I8 = np.dtype(np.int8)


def params(rate, baud=BAUDRATE):
    """the four doubles DDFskParams holds: P = rate / baud, P / 2, P / 2 + 1, g"""
    P = rate / baud
    if not P_MIN <= P <= P_MAX:         # (also false for a NaN)
        raise ValueError("fsk: an audio rate of %r S/s at %r baud is %r samples per symbol; %g to %g are supported"
                         % (rate, baud, P, P_MIN, P_MAX))
    return np.array([P, P / 2, (P / 2) + 1, GAIN], dtype=np.float64)


def state0():
    """the walk's state at the start of a recording, one STATE record in an array of one"""
    st = np.zeros(1, dtype=STATE)
    st["am"] = AM0
    return st


def walk(audio, rate, baud=BAUDRATE, state=None, base=0):
    """The timing walk over `audio` (float64 device array, samples base .. of the recording) from `state` (a STATE array of one;
    None: state0()) -> (sym, sidx, tmu, state after): per symbol the eye sample, the sample index it was read at and the timing
    after its update, as device arrays of the exact length.  Cut a recording anywhere and hand the state on: the pieces' results
    are the whole's."""
    _hip.require_gpu()
    if not isinstance(audio, DevArray) or audio.dtype != _F64:
        raise TypeError("float64 device array expected")
    prm = params(rate, baud)
    st = state0() if state is None else np.array(state, dtype=STATE).reshape(1)
    ctr0 = int(st["ctr"][0])
    st["ctr"] = 0                                           # the outputs of this call start at entry 0
    dstate = DevArray.from_host(st.view(np.uint8))
    # an eye event takes the timing back by P and the loop adds at least -g: once the timing is below P + 1, events are at least
    # max(1, P - 1 - g) >= P / 4 samples apart; a start state further up is the caller's, and shows as overflow
    cap = int(4 * audio.n / prm[0]) + 64
    sym, sidx, tmu = DevArray(cap, _F64), DevArray(cap, np.int64), DevArray(cap, _F64)
    check(lib().dd_fsk_walk(audio.ptr, audio.n, int(base), dstate.ptr, prm.ctypes.data_as(C.POINTER(C.c_double)), cap, sym.ptr,
                            sidx.ptr, tmu.ptr, None), "dd_fsk_walk")
    out = dstate.to_host().view(STATE).copy()
    if out["overflow"][0] and not st["overflow"][0]:
        raise RuntimeError("fsk walk: more symbols than %d (timing thrown by the start state)" % cap)
    n = int(out["ctr"][0])
    out["ctr"] = ctr0 + n
    return sym.view(0, n), sidx.view(0, n), tmu.view(0, n), out


def bit_stream(sym):
    """soft symbols (float64 device array) -> afsk.BitStream: mean = sym, sgn = the hard decisions r (1 where sym > 0), bits = NRZI
    of the descrambled r, marks and flags as afsk.bit_stream gives them"""
    _hip.require_gpu()
    if not isinstance(sym, DevArray) or sym.dtype != _F64:
        raise TypeError("float64 device array expected")
    n = sym.n
    cap = max(n, 1)
    r, bits, marks, flags = DevArray(cap, _I8), DevArray(cap, _I8), DevArray(cap, _I8), DevArray(cap, np.int64)
    counts = np.zeros(2, dtype=np.int64)
    check(lib().dd_fsk_bits(sym.ptr, n, r.ptr, bits.ptr, marks.ptr, flags.ptr, cap, counts.ctypes.data_as(C.POINTER(C.c_int64)), None),
          "dd_fsk_bits")
    nf = int(counts[1])
    return afsk.BitStream(sym, r.view(0, n), bits.view(0, n), marks.view(0, n), flags.view(0, nf))


def scramble(bits, state=0):
    """the transmitter's scrambler: out[k] = bits[k] ^ out[k-12] ^ out[k-17]; `state` holds the 17 line bits sent before, bit j - 1
    = the one j bits back (0: none)"""
    b = np.asarray(bits, dtype=np.uint8) & 1
    out = np.zeros(len(b) + 17, dtype=np.uint8)
    out[:17] = [(int(state) >> (16 - i)) & 1 for i in range(17)]
    for k in range(len(b)):
        out[k + 17] = b[k] ^ out[k + 17 - TAPS[0]] ^ out[k + 17 - TAPS[1]]
    return out[17:]


def descramble(line, state=0):
    """the receiver's descrambler: out[k] = line[k] ^ line[k-12] ^ line[k-17], the line bits before the start taken from `state` as
    in `scramble`.  Self-synchronising: whatever the state, the output is right from bit 17 on."""
    r = np.asarray(line, dtype=np.uint8) & 1
    ext = np.concatenate((np.array([(int(state) >> (16 - i)) & 1 for i in range(17)], dtype=np.uint8), r))
    return ext[17:] ^ ext[17 - TAPS[0]:len(ext) - TAPS[0]] ^ ext[:len(ext) - TAPS[1]]
