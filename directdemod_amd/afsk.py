"""
AFSK1200 correlator front end on the device -- the part of the reference's
decode_afsk1200.getMsg (decode_afsk1200.py:99-158) that is a pure-Python double
loop there: quadrature correlation against the mark (1200 Hz) and space (2200 Hz)
tones over one baud, the power difference ("binary filter"), and the bit-edge
detector -- and the frame logic behind them (:160-269), which is host code in the
reference: the lookahead peak pick (peakdetect.py), the bit slicer (bit_repeated,
per-bit means, NRZI, start flags, stuffing marks) and the per-flag-pair frame check
(de-stuffing, length tests, CRC) with the accepted frames' bytes.  Each stage is
callable on its own here; decode_afsk1200.py chains them.

The FM audio that feeds it comes from the same fused chain as every other decoder
(offsetFreq -> blackmanHarris(151) -> bwLim(bw) -> demod_fm -> butter band-pass,
decode_afsk1200.py:67-98).
"""
import ctypes as C

import numpy as np

from . import _hip
from ._hip import DevArray, check, lib

_F64 = np.dtype(np.float64)

BAUDRATE = 1200             # decode_afsk1200.py:31-33
MARK_FREQUENCY = 1200
SPACE_FREQUENCY = 2200


def correlator_tables(bw, baud=BAUDRATE, mark=MARK_FREQUENCY, space=SPACE_FREQUENCY):
    """decode_afsk1200.py:99-123 -> (tables[4, buffer_size] = mark_i, mark_q, space_i, space_q; samples per baud)"""
    buffer_size = int(np.round(bw / baud))
    samples_per_baud = bw // baud
    i = np.arange(buffer_size)
    mark_angle = (i * 1.0 / bw) / (1 / mark) * 2 * np.pi
    space_angle = (i * 1.0 / bw) / (1 / space) * 2 * np.pi
    return np.ascontiguousarray([np.cos(mark_angle), np.sin(mark_angle), np.cos(space_angle), np.sin(space_angle)],
                                dtype=np.float64), int(samples_per_baud)


def _dev(x):
    if isinstance(x, DevArray):
        if x.dtype != _F64:
            raise TypeError("float64 device array expected, got %s" % x.dtype)
        return x, False
    return DevArray.from_host(np.asarray(x, dtype=np.float64).ravel()), True


def binary_filter(sig, bw=22050, baud=BAUDRATE, mark=MARK_FREQUENCY, space=SPACE_FREQUENCY):
    """mark-minus-space correlator power per sample (decode_afsk1200.py:126-141).
    NumPy in -> NumPy out; DevArray in -> DevArray out."""
    _hip.require_gpu()
    tables, _ = correlator_tables(bw, baud, mark, space)
    d, host = _dev(sig)
    out = DevArray(d.n, _F64)
    check(lib().dd_afsk_binary_filter_f64(d.ptr, d.n, tables.ctypes.data_as(C.POINTER(C.c_double)), tables.shape[1],
                                          out.ptr, None), "dd_afsk_binary_filter_f64")
    return out.to_host() if host else out


def bit_edges(bf, samples_per_baud):
    """np.correlate(np.sign(bf), edge kernel, 'same') / samples_per_baud (decode_afsk1200.py:147-156)"""
    _hip.require_gpu()
    d, host = _dev(bf)
    out = DevArray(d.n, _F64)
    check(lib().dd_afsk_edges_f64(d.ptr, d.n, int(samples_per_baud), out.ptr, None), "dd_afsk_edges_f64")
    return out.to_host() if host else out


_I64 = np.dtype(np.int64)
_I8 = np.dtype(np.int8)


def _dev_i64(x):
    if isinstance(x, DevArray):
        if x.dtype != _I64:
            raise TypeError("int64 device array expected, got %s" % x.dtype)
        return x
    return DevArray.from_host(np.ascontiguousarray(x, dtype=np.int64).ravel())


def peak_lists(y, lookahead, delta=0.0):
    """peakdetect.peakdetect's lists on the device (dd_peakdetect_f64): ((max_pos, max_val), (min_pos, min_val)) as device
    arrays of the exact lengths.  Finite input only (DD_ERR_INVALID otherwise)."""
    _hip.require_gpu()
    d, _ = _dev(y)
    cap = d.n // 2 + 2
    mp, mv, np_, nv = DevArray(cap, _I64), DevArray(cap, _F64), DevArray(cap, _I64), DevArray(cap, _F64)
    counts = np.zeros(2, dtype=np.int64)
    check(lib().dd_peakdetect_f64(d.ptr, d.n, int(lookahead), float(delta), mp.ptr, mv.ptr, cap, np_.ptr, nv.ptr, cap,
                                  counts.ctypes.data_as(C.POINTER(C.c_int64)), None), "dd_peakdetect_f64")
    a, b = int(counts[0]), int(counts[1])
    return (mp.view(0, a), mv.view(0, a)), (np_.view(0, b), nv.view(0, b))


class BitStream:
    """dd_afsk_bits_f64's outputs (device arrays): mean (the reference's bitstream_nrzi), sgn (np.sign of it, NaN as 2),
    bits (decode_nrzi), marks (find_bit_stuffing), flags (bit_startflag)"""

    def __init__(self, mean, sgn, bits, marks, flags):
        self.mean, self.sgn, self.bits, self.marks, self.flags = mean, sgn, bits, marks, flags

    def __len__(self):
        return self.bits.n


def bit_stream(bf, peaks, bw=22050, baud=BAUDRATE):
    """decode_afsk1200.py:189-229 on the device: from binary_filter and the maxima positions (peakdetect's, ascending, in
    [0, len(bf))) to the bits, their stuffing marks and the start-flag positions.  Bit-exact (NumPy's summation order)."""
    _hip.require_gpu()
    spb = int(bw // baud)
    d, _ = _dev(bf)
    pk = _dev_i64(peaks)
    q = bw / baud
    # rint(d / q) <= d / q + 1/2 per interval, the intervals add up to less than n
    cap = int(d.n / q + pk.n / 2.0) + 2 if pk.n >= 2 else 0
    cap = max(cap, 1)
    mean, sgn, bits, marks = DevArray(cap, _F64), DevArray(cap, _I8), DevArray(cap, _I8), DevArray(cap, _I8)
    capf = max(cap, 1)
    flags = DevArray(capf, _I64)
    counts = np.zeros(2, dtype=np.int64)
    check(lib().dd_afsk_bits_f64(d.ptr, d.n, pk.ptr, pk.n, float(bw), spb, cap, mean.ptr, sgn.ptr, bits.ptr, marks.ptr,
                                 flags.ptr, capf, counts.ctypes.data_as(C.POINTER(C.c_int64)), None), "dd_afsk_bits_f64")
    nb, nf = int(counts[0]), int(counts[1])
    return BitStream(mean.view(0, nb), sgn.view(0, nb), bits.view(0, nb), marks.view(0, nb), flags.view(0, nf))


def frames(bs):
    """decode_afsk1200.py:236-269 on the device, one wave per consecutive flag pair: -> (info[npairs, 2] = (unstuffed bit count,
    accepted), [message bytes of each accepted pair, in pair order]).  Only the counts and the accepted bytes come down."""
    _hip.require_gpu()
    nf = bs.flags.n
    npairs = max(nf - 1, 0)
    info = np.zeros((npairs, 2), dtype=np.int64)
    if npairs == 0:
        return info, []
    P = C.POINTER(C.c_int64)
    check(lib().dd_afsk_frames_check(bs.bits.ptr, bs.marks.ptr, bs.bits.n, bs.flags.ptr, nf, info.ctypes.data_as(P), None),
          "dd_afsk_frames_check")
    nbytes = np.where(info[:, 1] == 1, (info[:, 0] - 16) // 8, 0)
    off = np.where(info[:, 1] == 1, np.cumsum(nbytes) - nbytes, -1).astype(np.int64)
    total = int(nbytes.sum())
    if total == 0:
        return info, []
    padded = (total + 3) // 4 * 4
    out = DevArray(padded, np.uint8)
    check(lib().dd_afsk_frames_pack(bs.bits.ptr, bs.marks.ptr, bs.bits.n, bs.flags.ptr, nf, info.ctypes.data_as(P),
                                    off.ctypes.data_as(P), out.ptr, padded, None), "dd_afsk_frames_pack")
    host = out.to_host()
    return info, [host[o:o + k].tobytes() for o, k in zip(off, nbytes) if o >= 0]
