"""
Funcube BPSK sync detection -- the reference's decode_funcube surface (decode_funcube.py): `useful`, `getSyncs` and the module
helpers `lim` / `limBin`, plus `getSymbols`, the PLL-corrected soft symbols (gardnerA after pllObj.loop) a later telemetry decoder
would read.

One decode pass, cached, feeds every property.  Per chunk of the recording (the reference's chunker, no chunker handed to the
signal, so the mixer phase restarts at 0 in every chunk): offsetFreq in the reference's float64 arithmetic (bpsk.mix; with
corrfreq the Doppler ramp of decode_funcube.py:202-226 formed in the kernel, bpsk.mix_ramp, from frequency_shift.dopplerTrack --
computed once per recording -- and dopplerRamp) -> butter(fs, bw) low-pass in scipy.signal.lfilter's own operation order
(bpsk.Lowpass: complex64 in, complex128 out, the state carried from chunk to chunk; bit for bit lfilter's output, which the
package's block-parallel IIR is not near enough to at 7 kHz), then the symbol walk (bpsk.Walker: Gardner timing, agc, costas) and the per-sample lim values.  After the last
chunk: the MINSYNC list on the device, the MAXSYNC buffers on the host and their correlations on the device.  Only counts, the
MINSYNC list, a few sample indices and the argmaxes come down.

Deviations from the reference:
  - no progress / ETA log lines (the MINSYNC, MAXSYNC and "doppler shift is" logging.info lines are kept);
  - with exactly one MAXSYNC the reference raises ValueError (np.min of an empty np.diff); here getSyncs returns [] with useful 0.
"""
import logging
import time

import numpy as np

from . import _hip, bpsk, chunker, comm, frequency_shift
from .bpsk import lim, limBin  # noqa: F401  (module-level helpers, as in the reference)


class decode_funcube:
    """Object to decode Funcube: decode_funcube(sigsrc, offset, bw, center_frequency, signal_freq, corrfreq) as in the reference
    (bw None -> 7000).  use_device_raw: read the recording as raw u8 pairs resident on the device when the source offers it
    (source.read_device_raw)."""

    def __init__(self, sigsrc, offset, bw, center_frequency, signal_freq, corrfreq=False, use_device_raw=True):
        self.__bw = 7000 if bw is None else bw
        self.__sigsrc = sigsrc
        self.__offset = offset
        self.__center_frequency = int(center_frequency)
        self.__signal_freq = int(signal_freq)
        self.__corrfreq = corrfreq
        self.__use_raw = use_device_raw
        self.__useful = 0
        self.__result = None
        self.timings = {}                 # seconds per stage of the last decode: doppler, mix, lowpass, walk, lim (summed over chunks), minsync, maxsync
        self.minsyncs = []                # MINSYNC ctr values of the last decode
        self.buffers = []                 # the MAXSYNC correlation buffers: (intervals [(first sample, count)], maxBuffStart)
        self.argmax = []                  # argmax of each buffer's |correlation|
        self.ramps = []                   # with corrfreq, per chunk: (chunk_offset, frequency_shift.ramp, doppCorrect_current after it)

    @property
    def useful(self):
        """1 if two MAXSYNCs lie 4.98 s +- 0.2 s apart, else 0 (0 until getSyncs has run)"""
        return self.__useful

    @property
    def getSyncs(self):
        """The MAXSYNC sample positions (np.int64) but the first"""
        return list(self._decode()[0])

    @property
    def getSymbols(self):
        """The PLL-corrected soft symbols as a device-resident commSignal at 12000 Hz"""
        return comm.commSignal(bpsk.SYMBOL_RATE, self._decode()[1])

    def walker(self):
        """the symbol walk of the last decode (bpsk.Walker: per-symbol device arrays)"""
        return self._decode()[2]

    def _decode(self):
        if self.__result is not None:
            return self.__result
        _hip.require_gpu()
        src = self.__sigsrc
        t = {"doppler": 0.0, "mix": 0.0, "lowpass": 0.0, "walk": 0.0, "lim": 0.0}
        t0 = time.perf_counter()

        def lap(name):
            nonlocal t0
            _hip.sync()
            now = time.perf_counter()
            t[name] = t.get(name, 0.0) + now - t0
            t0 = now
        ck = chunker.chunker(src)
        bf = bpsk.Lowpass(src.sampFreq, self.__bw)
        read = src.read
        if self.__use_raw and hasattr(src, "read_device_raw") and src.length > 0 and src.read_device_raw(0, 1) is not None:
            read = src.read_device_raw
        track = ramp = None
        ramps = []
        if self.__corrfreq and src.length > 0:
            track = frequency_shift.dopplerTrack(src, self.__center_frequency, self.__signal_freq, 20000)
            ramp = frequency_shift.dopplerRamp(self.__offset, src.sampFreq)
            track.shift(0, len(ck.getChunks))             # the one device pass over the recording, timed on its own
            lap("doppler")
        w = bpsk.Walker(src.sampFreq, src.length)
        for number, (a, b) in enumerate(ck.getChunks):
            if b <= a:
                continue
            d = read(a, b)
            if not isinstance(d, _hip.DevArray):
                d = _hip.DevArray.from_host(np.asarray(d), dtype=np.complex64)
            if track is None:
                mixed = bpsk.mix(d, src.sampFreq, self.__offset)
            else:
                chunk_offset = track.shift(number, len(ck.getChunks))
                logging.info("doppler shift is %f Hz", chunk_offset)
                r = ramp.next(chunk_offset, b - a)
                ramps.append((float(chunk_offset), r, float(ramp.current)))
                mixed = bpsk.mix_ramp(d, src.sampFreq, r)
            lap("mix")
            x = bf.apply(mixed)
            lap("lowpass")
            w.walk(x)
            lap("walk")
            w.lim(x)
            lap("lim")
        mins = bpsk.minsync_list(w)
        lap("minsync")
        for k, m in mins:
            logging.info("MINSYNC: %d %f", k + 1, abs(m - bpsk.WIN / 2))
        aidx = w.aidx

        def a_at(k):
            return int(aidx.view(k, 1).to_host()[0])
        bufs = bpsk.maxsync_buffers(mins[:, 0], src.length, a_at, w.nsym)
        am = bpsk.maxsync_argmax(w.lim_values, bufs)
        lap("maxsync")
        self.timings = t
        maxSyncs = []
        for (ivs, start), (arg, _) in zip(bufs, am):
            v = start + np.int64(arg)
            logging.info("MAXSYNC %d", v)
            maxSyncs.append(v)
        self.minsyncs = [int(k) + 1 for k in mins[:, 0]]
        self.buffers = bufs
        self.argmax = [int(a) for a in am[:, 0]]
        self.ramps = ramps
        syncs = []
        if len(maxSyncs) > 1:
            if np.min(np.abs(np.diff(maxSyncs) - (4.98 * 2048000))) < (0.2 * 2048000):
                self.__useful = 1
            syncs = list(maxSyncs)[1:]
        self.__result = (syncs, w.view("sym"), w)
        return self.__result
