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
import time

import numpy as np

from . import _hip, comm, filters, lrpt, qpsk, symbolsync
from .qpsk import lim, limBin  # noqa: F401  (module-level helpers, as in the reference)


class decode_meteorm2(symbolsync.SyncDecoder):
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
    lrpt.IMAGE_INFO record per image packet."""
    WALKER = qpsk.Walker
    STAGES = ("front_end",)
    SPACING = (0.11, 0.05)

    def __init__(self, sigsrc, offset, bw=None, use_device_raw=True, *, apids=lrpt.IMAGE_APIDS, period=lrpt.IMAGE_PERIOD):
        super().__init__(sigsrc, use_device_raw)
        self._bw = 70000 if bw is None else bw
        self._offset = offset
        self._frames = None
        self._rs = None
        self._apids = tuple(int(a) for a in apids)
        self._period = int(period)
        if len(self._apids) != 3 or len(set(self._apids)) != 3 or self._period < 1:
            raise ValueError("decode_meteorm2: three different channel APIDs and a period >= 1 expected")
        self._image = None

    @property
    def getImage(self):
        """The picture, uint8[H, 1568, 3]: the three channel planes in `apids` order, 8 rows per strip cycle, zero wherever no packet
        was placed"""
        return self._decode_image()[0]

    def getChannel(self, apid):
        """One channel's plane, uint8[H, 1568]"""
        if apid not in self._apids:
            raise ValueError("decode_meteorm2.getChannel: APID %r is none of %r" % (apid, self._apids))
        return self._decode_image()[0][:, :, self._apids.index(apid)]

    @property
    def imageInfo(self):
        """Per image packet (lrpt.IMAGE_INFO): packet (the row of packetInfo), apid, mcun (its first block in the strip), q, mcus
        (blocks decoded, 14: all), strip (-1: not placed), and the on-board time day, ms, us"""
        return self._decode_image()[1]

    def _decode_image(self):
        if self._image is not None:
            return self._image
        pkts = self._decode_rs()[2]
        t0 = time.perf_counter()
        took = {}

        def decode(*args):
            _hip.sync()
            t1 = time.perf_counter()
            mcus = lrpt.jpeg_decode(*args)
            took["jpeg"] = took.get("jpeg", 0.0) + time.perf_counter() - t1
            return mcus
        self._image = lrpt.image(pkts, self._apids, self._period, decode=decode)
        self.timings["lrpt_jpeg"] = took.get("jpeg", 0.0)
        self.timings["lrpt_image_host"] = time.perf_counter() - t0 - self.timings["lrpt_jpeg"]
        return self._image

    @property
    def getFrames(self):
        """The LRPT frame bodies, uint8[n, 1020], in stream order"""
        return self._decode_frames()[0]

    @property
    def frameInfo(self):
        """Per frame (lrpt.INFO): symbol (of the marker's first bit), sample (the walk's A sample of that symbol), hypothesis,
        asm_score (of 52), asm_errors (of 32 decoded marker bits), corrected (channel bits the decoder changed), vcid, counter"""
        return self._decode_frames()[1]

    @property
    def getVCDUs(self):
        """The frames' 892 data bytes, uint8[n, 892], row-aligned with getFrames: corrected where the codeword was decodable, as
        received where it was not"""
        return self._decode_rs()[0]

    @property
    def rsInfo(self):
        """Per frame (lrpt.RS_INFO): errors (bytes changed in each of the four codewords, -1: not decodable), ok (all four decoded),
        and vcid, counter from the corrected header (meaningful when ok)"""
        return self._decode_rs()[1]

    @property
    def getPackets(self):
        """The CCSDS source packets (bytes, header included) reassembled from the ok frames, in order of completion"""
        return self._decode_rs()[2]

    @property
    def packetInfo(self):
        """Per packet (lrpt.PACKET_INFO): apid, flags, count, vcid, frame (the row of getFrames in which its first byte lies), length"""
        return self._decode_rs()[3]

    def _decode_rs(self):
        if self._rs is not None:
            return self._rs
        bodies = self._decode_frames()[0]
        t0 = time.perf_counter()
        fixed, errors = lrpt.reed_solomon(bodies)
        info = np.zeros(len(bodies), dtype=lrpt.RS_INFO)
        info["errors"] = errors
        info["ok"] = np.all(errors >= 0, axis=1)
        info["vcid"] = fixed[:, 1] & 0x3F
        info["counter"] = (fixed[:, 2].astype(np.int64) << 16) | (fixed[:, 3].astype(np.int64) << 8) | fixed[:, 4]
        vcdus = np.ascontiguousarray(fixed[:, :lrpt.VCDU_BYTES])
        t1 = time.perf_counter()
        pkts, pinfo = lrpt.packets(vcdus, info["ok"], info["vcid"], info["counter"])
        self.timings["lrpt_rs"] = t1 - t0
        self.timings["lrpt_packets"] = time.perf_counter() - t1
        self._rs = (vcdus, info, pkts, pinfo)
        return self._rs

    def _decode_frames(self):
        if self._frames is not None:
            return self._frames
        w = self.walker()
        t0 = time.perf_counter()

        def lap(name):
            nonlocal t0
            _hip.sync()
            now = time.perf_counter()
            self.timings["lrpt_" + name] = now - t0
            t0 = now
        soft = lrpt.soft_symbols(w.view("sym"))
        lap("soft")
        starts = lrpt.frame_starts(lrpt.asm_candidates(soft, w.nsym), w.nsym)
        lap("asm")
        bits = lrpt.viterbi(soft, w.nsym, starts[:, :2])
        lap("viterbi")
        bodies, fin = lrpt.finish(bits, soft, w.nsym, starts[:, :2])
        info = np.zeros(len(starts), dtype=lrpt.INFO)
        info["symbol"], info["hypothesis"], info["asm_score"] = starts[:, 0], starts[:, 1], starts[:, 2]
        info["asm_errors"], info["corrected"], info["vcid"] = fin[:, 0], fin[:, 1], fin[:, 2]
        info["sample"] = [int(w.aidx.view(int(k), 1).to_host()[0]) for k in starts[:, 0]]
        info["counter"] = [lrpt.vcdu_header(b)["counter"] for b in bodies]
        lap("finish")
        self._frames = (bodies, info)
        return self._frames

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
