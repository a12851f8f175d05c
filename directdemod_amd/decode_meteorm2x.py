"""
Meteor-M N2-x LRPT decoding from an IQ recording -- beyond the reference, which has no OQPSK: the N2-x satellites send offset QPSK
at 72 or 80 ksym/s, differentially (NRZ-M) coded, the 80 ksym/s mode interleaved (DESIGN.md sections 4.18 and 4.19).

One decode pass, cached.  Per chunk of the recording: the package's phase-continuous NCO (commSignal.offsetFreq with the chunker handed to
the signal, so the mixer's phase runs on from chunk to chunk -- the OQPSK walk keeps the carrier phase it has locked to) ->
butter(fs, bw) low-pass with carried state -> the OQPSK symbol walk (oqpsk.Walker: agc, Gardner timing on both staggered rails, Costas
loop, one serial chain).  After the last chunk the walk's symbols become int8 soft pairs (lrpt.soft_symbols) and run through
decode_lrpt's chain with stagger="auto": at two of the walk's four carrier-phase ambiguities its rails come out one symbol apart.

Nothing here has been verified against a recording of a satellite: every stage is defined in DESIGN.md and tested against its NumPy
restatement on synthesised recordings.
"""

import numpy as np

from . import _hip, chunker, comm, constants, filters, lrpt, oqpsk
from ._burst import Laps
from .decode_lrpt import decode_lrpt


class decode_meteorm2x(decode_lrpt):
    """decode_meteorm2x(sigsrc, offset, bw=None, *, symbol_rate=72000, differential=True, interleaved=False, branches=36, delay=2048,
    apids=..., period=..., use_device_raw=True, chunk_size=constants.PROC_CHUNKSIZE): `offset` as in decode_meteorm2 (the signal is
    multiplied by exp(-2 pi j offset t)); bw None -> 70000 * symbol_rate / 72000.
    `getSymbols`: the walk's symbols (I + jQ, complex128) as a device-resident commSignal at the symbol rate; `getSoft`: their int8
    soft pairs as a host array, what decode_lrpt(..., stagger="auto") takes; `walker()`: the oqpsk.Walker of the decode.
    `stagger`, `locked`, `lock`, `deintInfo` and getFrames ... getImage are decode_lrpt's.  frameInfo['sample'] is the sample at which
    the I rail of the frame's first symbol was read (the walk's A sample), -1 when interleaved.  timings: front_end, walk (summed over
    the chunks), then decode_lrpt's."""

    def __init__(self, sigsrc, offset, bw=None, *, symbol_rate=72000, differential=True, interleaved=False,
                 branches=lrpt.INTERLEAVER_BRANCHES, delay=lrpt.INTERLEAVER_DELAY, apids=lrpt.IMAGE_APIDS, period=lrpt.IMAGE_PERIOD,
                 use_device_raw=True, chunk_size=constants.PROC_CHUNKSIZE):
        if symbol_rate not in oqpsk.SYMBOL_RATES:
            raise ValueError("decode_meteorm2x: a symbol rate of 72000 or 80000 expected, got %r" % (symbol_rate,))
        super().__init__(np.zeros(0, dtype=np.int8), differential=differential, interleaved=interleaved, branches=branches, delay=delay,
                         apids=apids, period=period, stagger="auto")
        self._sigsrc = sigsrc
        self._offset = offset
        self._symbol_rate = symbol_rate
        self._bw = 70000.0 * symbol_rate / 72000.0 if bw is None else bw
        self._use_raw = use_device_raw
        self._chunk_size = int(chunk_size)
        self._walker = None

    @property
    def getSymbols(self):
        """The walk's symbols as a device-resident commSignal at the symbol rate"""
        return comm.commSignal(self._symbol_rate, self.walker().view("sym"))

    @property
    def getSoft(self):
        """The int8 soft pairs of the walk's symbols (lim(I / 2), lim(Q / 2)) as a host array, int8[2 nsym], before any re-stagger"""
        self.walker()
        return self._input.to_host()

    def walker(self):
        """the OQPSK walk of the decode (per-symbol device arrays), run on first use"""
        if self._walker is not None:
            return self._walker
        _hip.require_gpu()
        src = self._sigsrc
        t = dict(front_end=0.0, walk=0.0)
        lap = Laps(t).lap
        ck = chunker.chunker(src, self._chunk_size)
        read = src.read
        if self._use_raw and hasattr(src, "read_device_raw") and src.length > 0 and src.read_device_raw(0, 1) is not None:
            read = src.read_device_raw
        bf = filters.butter(src.sampFreq, self._bw)
        w = oqpsk.Walker(src.sampFreq, src.length, self._symbol_rate)
        for a, b in ck.getChunks:
            if b <= a:
                continue
            d = read(a, b)
            if not isinstance(d, _hip.DevArray):
                d = _hip.DevArray.from_host(np.asarray(d), dtype=np.complex64)
            sig = comm.commSignal(src.sampFreq, d, ck).offsetFreq(self._offset)
            sig.filter(bf)
            x = sig.device_signal
            lap("front_end")
            w.walk(x)
            lap("walk")
        self._input = lrpt.soft_symbols(w.view("sym"))
        self.timings.update(t)
        self._walker = w
        return w

    def _deint(self):
        self.walker()
        return super()._deint()

    def _lrpt_soft(self):
        soft, nsym, samples = super()._lrpt_soft()
        if self._interleaved:
            return soft, nsym, samples
        w = self.walker()
        lead = 1 if self.stagger < 0 else 0              # pair k of the re-staggered stream holds the I rail of symbol k + lead

        def a_samples(symbols):
            return np.array([int(w.aidx.view(int(k) + lead, 1).to_host()[0]) for k in symbols], dtype=np.int64)
        return soft, nsym, a_samples
