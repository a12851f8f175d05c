"""
Meteor-M2 QPSK sync detection -- the reference's decode_meteorm2 surface (decode_meteorm2.py): `useful`, `getSyncs` and the
module helpers `lim` / `limBin`, plus `getSymbols`, the PLL-corrected soft symbols (gardnerA after pllObj.loop) a later LRPT decoder
would read.

One decode pass, cached, feeds both properties.  Per chunk of the recording (the reference's chunker, no chunker handed to the
signal, so the mixer phase restarts at 0 in every chunk): offsetFreq in the reference's float64 arithmetic (qpsk.mix: the package's
fixed-point NCO is 1e-7 off, enough to move a Gardner timing decision) -> butter(fs, bw) low-pass (complex64 in, complex128 out, the
state carried from chunk to chunk), then the symbol walk (qpsk.Walker: Gardner timing, agc, costas) and the per-sample lim values.
After the last chunk: the MINSYNC candidates on the device, the gating scan on the host, the MAXSYNC buffers on the host and their
correlations on the device.  Only counts, candidate windows, a few symbol bits and sample indices, and the argmaxes come down.

Deviations from the reference:
  - no progress / ETA log lines (the MINSYNC and MAXSYNC logging.info lines are kept);
  - with exactly one MAXSYNC the reference raises ValueError (np.min of an empty np.diff); here getSyncs returns [] with useful 0.
"""
import logging
import time

import numpy as np

from . import _hip, chunker, comm, filters, qpsk
from .qpsk import lim, limBin  # noqa: F401  (module-level helpers, as in the reference)


class decode_meteorm2:
    """Object to decode Meteor m2: decode_meteorm2(sigsrc, offset, bw) as in the reference (bw None -> 70000).
    use_device_raw: read the recording as raw u8 pairs resident on the device when the source offers it (source.read_device_raw)."""

    def __init__(self, sigsrc, offset, bw=None, use_device_raw=True):
        self.__bw = 70000 if bw is None else bw
        self.__sigsrc = sigsrc
        self.__offset = offset
        self.__use_raw = use_device_raw
        self.__useful = 0
        self.__result = None
        self.timings = {}                 # seconds per stage of the last decode: front_end, walk, lim (summed over chunks), minsync, maxsync
        self.minsyncs = []                # MINSYNC events of the last decode: (ctr, template 0 = sync2mhz / 1 = sync2mhz2)
        self.buffers = []                 # the MAXSYNC correlation buffers: (intervals [(first sample, count)], maxBuffStart, template)
        self.argmax = []                  # argmax of each buffer's |correlation|

    @property
    def useful(self):
        """1 if two MAXSYNCs lie 0.11 s +- 0.05 s apart, else 0 (0 until getSyncs has run)"""
        return self.__useful

    @property
    def getSyncs(self):
        """The MAXSYNC sample positions (np.float64) but the first"""
        return list(self._decode()[0])

    @property
    def getSymbols(self):
        """The PLL-corrected soft symbols as a device-resident commSignal at 72000 Hz"""
        return comm.commSignal(qpsk.SYMBOL_RATE, self._decode()[1])

    def walker(self):
        """the symbol walk of the last decode (qpsk.Walker: per-symbol device arrays)"""
        return self._decode()[2]

    def _decode(self):
        if self.__result is not None:
            return self.__result
        _hip.require_gpu()
        src = self.__sigsrc
        t = {"front_end": 0.0, "walk": 0.0, "lim": 0.0}
        t0 = time.perf_counter()

        def lap(name):
            nonlocal t0
            _hip.sync()
            now = time.perf_counter()
            t[name] = t.get(name, 0.0) + now - t0
            t0 = now
        ck = chunker.chunker(src)
        bf = filters.butter(src.sampFreq, self.__bw)
        read = src.read
        if self.__use_raw and hasattr(src, "read_device_raw") and src.length > 0 and src.read_device_raw(0, 1) is not None:
            read = src.read_device_raw
        w = qpsk.Walker(src.sampFreq, src.length)
        for a, b in ck.getChunks:
            if b <= a:
                continue
            d = read(a, b)
            if not isinstance(d, _hip.DevArray):
                d = _hip.DevArray.from_host(np.asarray(d), dtype=np.complex64)
            sig = comm.commSignal(src.sampFreq, qpsk.mix(d, src.sampFreq, self.__offset))
            sig.filter(bf)
            x = sig.device_signal
            lap("front_end")
            w.walk(x)
            lap("walk")
            w.lim(x)
            lap("lim")
        cands, bits = qpsk.minsync_candidates(w)

        def fetch(lo, hi):
            v = bits.view(lo, hi - lo).to_host().astype(np.int64)
            return np.stack((v & 1, v >> 1), axis=1)
        events = qpsk.minsync_scan(cands, w.nsym, fetch)
        lap("minsync")
        for k, _ in events:
            logging.info("MINSYNC: %d", k + 1)
        aidx = w.aidx

        def a_at(k):
            return int(aidx.view(k, 1).to_host()[0])
        bufs = qpsk.maxsync_buffers(events, src.length, a_at, w.nsym)
        am = qpsk.maxsync_argmax(w.lim_values, bufs)
        lap("maxsync")
        self.timings = t
        maxSyncs = []
        for (ivs, start, _), (arg, _) in zip(bufs, am):
            v = start + (np.int64(arg) / 2.0)
            logging.info("MAXSYNC %d", v)
            maxSyncs.append(v)
        self.minsyncs = [(k + 1, tm) for k, tm in events]
        self.buffers = bufs
        self.argmax = [int(a) for a in am[:, 0]]
        syncs = []
        if len(maxSyncs) > 1:
            if np.min(np.abs(np.diff(maxSyncs) - (0.11 * 2048000))) < (0.05 * 2048000):
                self.__useful = 1
            syncs = list(maxSyncs)[1:]
        self.__result = (syncs, w.view("sym"), w)
        return self.__result
