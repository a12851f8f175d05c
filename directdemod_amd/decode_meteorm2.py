"""
Meteor-M2 QPSK sync detection -- the reference's decode_meteorm2 surface (decode_meteorm2.py): `useful`, `getSyncs` and the
module helpers `lim` / `limBin`, plus `getSymbols`, the PLL-corrected soft symbols (gardnerA after pllObj.loop), and beyond the
reference `getFrames` / `frameInfo`: the LRPT channel frames decoded from those symbols (lrpt.py), and
`getVCDUs` / `rsInfo` / `getPackets` / `packetInfo`: the frames after Reed-Solomon correction and the CCSDS source packets
reassembled from them, and `getImage` / `getChannel` / `imageInfo`: the picture decoded from the image
packets among them.

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

import numpy as np

from . import comm, filters, lrpt, qpsk, symbolsync
from .decode_lrpt import LrptChain
from .qpsk import lim, limBin  # noqa: F401  (module-level helpers, as in the reference)


class decode_meteorm2(symbolsync.SyncDecoder, LrptChain):
    """Object to decode Meteor m2: decode_meteorm2(sigsrc, offset, bw) as in the reference (bw None -> 70000).
    use_device_raw: read the recording as raw u8 pairs resident on the device when the source offers it (source.read_device_raw).
    `useful`: 1 if two MAXSYNCs lie 0.11 s +- 0.05 s apart; `getSyncs`: np.float64 positions; `getSymbols`: at 72000 Hz.
    minsyncs: (ctr, template 0 = sync2mhz / 1 = sync2mhz2) per MINSYNC event; buffers: (intervals, maxBuffStart, template).
    `getFrames`: uint8[n, 1020], the de-randomised LRPT frame bodies in stream order (Reed-Solomon parity still attached);
    `frameInfo`: one lrpt.INFO record per frame.  Both come from the same cached walk, whether or not the 120-bit sync was seen.
    `getVCDUs`: uint8[n, 892], the frames' data bytes after Reed-Solomon correction, row-aligned with getFrames; `rsInfo`: one
    lrpt.RS_INFO record per frame; `getPackets`: the source packets as bytes, in order of completion; `packetInfo`: one
    lrpt.PACKET_INFO record per packet.
    `getImage`: uint8[H, 1568, 3], the picture decoded from the image packets of the three channels `apids` (keyword, in the
    order in which they occupy a strip cycle of `period` packets); `getChannel(apid)`: one plane; `imageInfo`: one
    lrpt.IMAGE_INFO record per image packet.  The chain from the soft symbols on is decode_lrpt.LrptChain,
    shared with decode_lrpt; `getSoft`: the walk's int8 soft pairs, what decode_lrpt reads."""
    WALKER = qpsk.Walker
    STAGES = ("front_end",)
    SPACING = (0.11, 0.05)

    def __init__(self, sigsrc, offset, bw=None, use_device_raw=True, *, apids=lrpt.IMAGE_APIDS, period=lrpt.IMAGE_PERIOD):
        super().__init__(sigsrc, use_device_raw)
        self._bw = 70000 if bw is None else bw
        self._offset = offset
        self._init_chain(apids, period)

    @property
    def getSoft(self):
        """The int8 soft pairs of the walk's symbols (lim(re / 2), lim(im / 2) per symbol) as a host array, int8[2 nsym]: what
        decode_lrpt takes and lrpt.write_soft writes"""
        return self._lrpt_soft()[0].to_host()

    def _lrpt_prepare(self):
        self.walker()

    def _lrpt_soft(self):
        w = self.walker()
        return (lrpt.soft_symbols(w.view("sym")), w.nsym,
                lambda symbols: np.array([int(w.aidx.view(int(k), 1).to_host()[0]) for k in symbols], dtype=np.int64))

    def _front_end(self, src, ck, lap):
        bf = filters.butter(src.sampFreq, self._bw)

        def front(number, a, b, d):
            sig = comm.commSignal(src.sampFreq, qpsk.mix(d, src.sampFreq, self._offset))
            sig.filter(bf)
            lap("front_end")
            return sig.device_signal
        return front

    def _sync_search(self, w, total, a_at, lap):
        cands, bits = qpsk.minsync_candidates(w)

        def fetch(lo, hi):
            v = bits.view(lo, hi - lo).to_host().astype(np.int64)
            return np.stack((v & 1, v >> 1), axis=1)
        events = qpsk.minsync_scan(cands, w.nsym, fetch)
        lap("minsync")
        for k, _ in events:
            logging.info("MINSYNC: %d", k + 1)
        bufs = qpsk.maxsync_buffers(events, total, a_at, w.nsym)
        am = qpsk.maxsync_argmax(w.lim_values, bufs)
        lap("maxsync")
        return [(k + 1, tm) for k, tm in events], bufs, am

    def _position(self, start, arg):
        return start + (np.int64(arg) / 2.0)
