"""
Doppler tracking (reference: sandbox/frequency_shift.py, used by decode_funcube.py:202-228 under --freqshift).

The spectrum waterfall (``make_fft``) and the per-row band argmax of ``find_shift`` run on the MI355X over the raw uint8 I,Q
recording (dd_waterfall_u8, dd_band_argmax_f32); everything after the argmax -- the track offset, ``rolling_window``, the
multiplication by ``df``, ``correct_shift`` -- is the reference's float64 arithmetic on the host, in its operation order: a few
hundred numbers.  Function names and argument orders are the reference module's.

``iq_stream`` may be a flat uint8 array or memmap (I,Q interleaved), a source object of this package (its recording is made
resident once through ``read_device_raw`` and shared with the decoders) or a device array of raw pairs (``_hip.IQ8``).

``dopplerTrack`` computes the track once per recording and answers every chunk from it (the reference recomputes it over the
whole file for each chunk); ``dopplerRamp`` is the per-chunk ramp state machine of decode_funcube.py:211-226, whose descriptors
``commSignal.offsetFreq`` turns into samples on the device (dd_nco_c64_ramp).

Inputs the reference itself cannot handle raise ValueError: fewer than 10 waterfall rows (its rolling mean is over 0 rows),
``every <= 1`` with a partial last window (it fails in fftshift of a scalar), a recording shorter than one window, an odd
number of raw bytes, a band that leaves [0, window).  Its last loop (:115-116) changes nothing that is returned and is left out.
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

from . import _hip, constants
from ._hip import DevArray

WINDOW = 2048 * 2 * 2              # frequency_shift.py:62

# a frequency ramp for commSignal.offsetFreq: f[i] = start + i * delta clipped to target (from above when target > start,
# from below otherwise), i < n.  `delta` is the step NumPy's arange fills with, (start + d) - start.
ramp = namedtuple("ramp", "start delta target n")


def _raw_on_device(iq_stream):
    """-> (device array that keeps the bytes alive, pointer, number of raw bytes)"""
    if hasattr(iq_stream, "read_device_raw"):
        d = iq_stream.read_device_raw(0, iq_stream.length)
        if d is None:
            raise ValueError("the recording is larger than DD_RESIDENT_BYTES: it cannot be made resident on the device")
        return d, d.ptr, d.nbytes
    if isinstance(iq_stream, DevArray):
        if iq_stream.dtype not in (_hip.IQ8, np.dtype(np.uint8)):
            raise TypeError("device iq_stream must hold raw uint8 I,Q (dtype _hip.IQ8 or uint8), not %s" % iq_stream.dtype)
        return iq_stream, iq_stream.ptr, iq_stream.nbytes
    a = np.asarray(iq_stream)
    if a.dtype != np.uint8:
        raise TypeError("iq_stream must be raw uint8 I,Q, not %s" % a.dtype)
    d = DevArray.from_host(a.reshape(-1), dtype=np.uint8)
    return d, d.ptr, d.nbytes


def _stream_bytes(iq_stream):
    """len(iq_stream) of the reference: the number of raw bytes"""
    if hasattr(iq_stream, "read_device_raw"):
        return 2 * int(iq_stream.length)
    if isinstance(iq_stream, DevArray):
        return int(iq_stream.nbytes)
    return int(np.size(iq_stream))


def _row_count(nbytes, window, every):
    """rows make_fft closes (frequency_shift.py:15-40), after the checks of what the reference cannot handle"""
    window = int(window)
    if window < 16 or window > 8192 or window & (window - 1):
        raise ValueError("window must be a power of two in 16..8192, got %r" % (window,))
    if nbytes % 2:
        raise ValueError("odd number of raw bytes (%d): the last I has no Q" % nbytes)
    if not every > 0 or math.isinf(every):
        raise ValueError("every must be positive and finite, got %r" % (every,))
    span = 2 * window
    n_full, n_slices = nbytes // span, -(-nbytes // span)
    if n_full < 1:
        raise ValueError("recording shorter than one window: %d samples, window %d" % (nbytes // 2, window))
    row_len = int(math.ceil(every))
    if row_len <= 1 and n_slices != n_full:
        raise ValueError("every <= 1 (%r) with a partial last window: that row would hold no spectrum "
                         "(the reference fails in fftshift of a scalar)" % (every,))
    return n_slices // row_len


def waterfall(iq_stream, window, every):
    """make_fft's rows as one device array, float32 [rows * window], and the row count"""
    nbytes = _stream_bytes(iq_stream)
    rows = _row_count(nbytes, window, float(every))
    _hip.require_gpu()
    keep, ptr, nb = _raw_on_device(iq_stream)
    assert nb == nbytes
    out = DevArray(rows * int(window), np.float32)
    got = C.c_int64(0)
    _hip.check(_hip.lib().dd_waterfall_u8(ptr, nbytes, int(window), float(every), out.ptr, rows, C.byref(got), None),
               "dd_waterfall_u8")
    if got.value != rows:
        raise _hip.HipError("dd_waterfall_u8 closed %d rows, expected %d" % (got.value, rows))
    _hip.sync()
    del keep
    return out, rows


def band_argmax(rows_dev, rows, window, band_start, band_stop):
    """np.argmax(row[band_start:band_stop]) of every waterfall row -> int32 [rows] on the host"""
    if not (0 <= band_start < band_stop <= window):
        raise ValueError("band [%d, %d) leaves [0, %d)" % (band_start, band_stop, window))
    idx = DevArray(rows, np.int32)
    _hip.check(_hip.lib().dd_band_argmax_f32(rows_dev.ptr, rows, int(window), int(band_start), int(band_stop), idx.ptr, None),
               "dd_band_argmax_f32")
    return idx.to_host()


def make_fft(window, samplerate, df, every, iq_stream, device=False):
    """frequency_shift.py:5-44: a list of host rows (float64 copies of the device's float32 rows); ``device=True`` returns the
    device array [rows * window] instead, nothing downloaded"""
    dev, rows = waterfall(iq_stream, window, every)
    if device:
        return dev
    return list(dev.to_host().astype(np.float64).reshape(rows, int(window)))


def rolling_window(input, window):
    """frequency_shift.py:46-57: mean over `window` entries, the first window for the head, the last -window // 2 for the tail"""
    half = window // 2
    output = []
    for i in range(len(input)):
        if i < half:
            output.append(np.mean(input[0:window]))
        elif i > len(input) - half:
            output.append(np.mean(input[-window // 2:]))
        else:
            output.append(np.mean(input[i - half:i - half + window]))
    return output


def _band(samplerate, center_frequency, channel_frequency, bandwidth, window=WINDOW):
    """(df, every's divisor aside) the band columns of find_shift (:65-79)"""
    T = 1.0 / samplerate
    xf = np.fft.fftshift(np.fft.fftfreq(window, T))
    df = xf[1] - xf[0]
    center = (samplerate / 2 + (channel_frequency - center_frequency)) / df
    band_start = int(center - bandwidth / (2 * df))
    band_stop = int(center + bandwidth / (2 * df))
    if not (0 <= band_start < band_stop <= window):
        raise ValueError("the band of %r Hz around channel offset %r Hz is columns [%d, %d): it leaves [0, %d)" %
                         (bandwidth, channel_frequency - center_frequency, band_start, band_stop, window))
    return df, band_start, band_stop


def smooth_track(argmax, bandwidth, df):
    """find_shift from the raw per-row argmax on (:92-107), float64 on the host"""
    track = [int(a) - bandwidth / (2 * df) for a in argmax]
    N = int(len(track) * 0.1)
    if N < 1:
        raise ValueError("fewer than 10 waterfall rows (%d): the rolling mean would be over 0 rows" % len(track))
    return np.multiply(rolling_window(track, N), df)


def _find(iq_stream, samplerate, center_frequency, channel_frequency, bandwidth):
    window = WINDOW
    df, band_start, band_stop = _band(samplerate, center_frequency, channel_frequency, bandwidth, window)
    every = (_stream_bytes(iq_stream) / (samplerate * 2.0)) * 8192.0 / window
    rows = _row_count(_stream_bytes(iq_stream), window, every)
    if rows < 10:
        raise ValueError("fewer than 10 waterfall rows (%d): the rolling mean would be over 0 rows" % rows)
    dev, rows = waterfall(iq_stream, window, every)
    argmax = band_argmax(dev, rows, window, band_start, band_stop)
    return argmax, smooth_track(argmax, bandwidth, df)


def find_shift(iq_stream, samplerate, center_frequency, channel_frequency, bandwidth):
    """frequency_shift.py:60-126: the smoothed Doppler track in Hz, one value per waterfall row"""
    return _find(iq_stream, samplerate, center_frequency, channel_frequency, bandwidth)[1]


def correct_shift(shift, position):
    """frequency_shift.py:128-144: the track entry at `position` in [0, 1]"""
    step = 1 / (len(shift) - 1)
    x1 = int(np.floor(position / step + (step / 2)))
    return shift[x1]


def correct(iq_stream, samplerate, center_frequency, channel_frequency, bandwidth, chunk_number, chunk_length):
    """frequency_shift.py:147-149.  Computes the whole track on every call like the reference; a chunk loop wants dopplerTrack."""
    shift = find_shift(iq_stream, samplerate, center_frequency, channel_frequency, bandwidth)
    return correct_shift(shift, chunk_number / chunk_length)


class dopplerTrack:
    '''The Doppler track of one recording, computed on first use and kept: ``shift(chunk_number, n_chunks)`` is
    ``correct(sigsrc.memmap, sigsrc.sampFreq, center, channel, bandwidth, chunk_number, n_chunks)`` without the recomputation.
    A source narrowed by ``limitData`` is tracked over the part it exposes (``read_device_raw(0, sigsrc.length)``, the samples
    the decoders see), while ``memmap`` is always the whole file: the two agree on a source that is not narrowed.'''

    def __init__(self, sigsrc, center_frequency, channel_frequency, bandwidth=20000):
        self.__sigsrc = sigsrc
        self.__args = (center_frequency, channel_frequency, bandwidth)
        self.__found = None
        self.computed = 0              # how many times the device pass ran (stays 1)

    def __compute(self):
        if self.__found is None:
            self.__found = _find(self.__sigsrc, self.__sigsrc.sampFreq, *self.__args)
            self.computed += 1
        return self.__found

    @property
    def argmax(self):
        ''':obj:`numpy array`: the raw per-row argmax inside the band (int32)'''
        return self.__compute()[0]

    @property
    def track(self):
        ''':obj:`numpy array`: the smoothed track in Hz (find_shift's return value)'''
        return self.__compute()[1]

    def shift(self, chunk_number, n_chunks):
        '''Doppler shift in Hz for chunk `chunk_number` of `n_chunks`'''
        return correct_shift(self.track, chunk_number / n_chunks)


class dopplerRamp:
    '''The ramp state machine of decode_funcube.py:211-226: each chunk's mixer frequency moves from where the last chunk ended
    towards ``offset + shift`` at 2000 Hz per PROC_CHUNKSIZE samples and stays there once it arrives.'''

    def __init__(self, offset, samp_rate=None):
        self.offset = offset
        self.samp_rate = samp_rate     # of the signal the ramps are for (not needed to form them)
        self.current = None
        self.bw = 2000.0 / constants.PROC_CHUNKSIZE

    def next(self, target_shift, n):
        '''-> ramp(start, delta, target, n) for a chunk of n samples; ``current`` moves to the ramp's last sample'''
        n = int(n)
        if n < 1:
            raise ValueError("a ramp needs at least one sample (the reference reads doppCorrect_freqs[-1])")
        target = self.offset + target_shift
        if self.current is None:
            self.current = target
        start = self.current
        d = self.bw if target > start else -1 * self.bw
        delta = (start + d) - start                      # NumPy's arange: start + i * (buffer[1] - buffer[0])
        last = start + (n - 1) * delta
        if (last > target) if target > start else (last < target):
            last = target
        self.current = last
        return ramp(float(start), float(delta), float(target), n)
