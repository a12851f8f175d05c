"""
LRPT decoding from soft symbols -- the int8 I, Q pairs that demodulators write and decoders read (the `.s` file), in the mode of
Meteor-M N2 and in the modes of the N2-x satellites: differential (NRZ-M) coding in front of the convolutional encoder, and the
80 ksym/s mode's convolutional interleaver with its 8-bit marker (lrpt.py), with the rails of an OQPSK
demodulator's output brought back together where they lie one symbol apart (`stagger`, section 4.19).

`LrptChain` is the chain behind the soft symbols -- frames (section 4.14), Reed-Solomon correction and source packets (4.15), the
picture (4.16) -- that `decode_lrpt` here, `decode_meteorm2` (whose soft symbols come from its symbol walk) and `decode_meteorm2x`
(decode_lrpt behind the OQPSK walk) all run.
"""
import os
import time

import numpy as np

from . import _hip, lrpt


class LrptChain:
    """getFrames / frameInfo, getVCDUs / rsInfo / getPackets / packetInfo, getImage / getChannel / imageInfo over the soft symbols a
    subclass supplies: _lrpt_prepare() does what has to be there before them (not timed here); _lrpt_soft() -> (device int8 pairs,
    nsym, samples) with samples(symbols) -> frameInfo['sample'] of frames that start at those symbols; _lrpt_starts(soft, nsym) is
    the marker search, which a subclass that has searched already answers from what it found.  Every stage runs once and is cached; `timings` gains lrpt_* (seconds per stage)."""

    def _init_chain(self, apids, period, differential=False):
        self._nrzm = bool(differential)
        self._template = lrpt.ASM_ENCODED_NRZM if differential else lrpt.ASM_ENCODED
        self._frames = None
        self._rs = None
        self._image = None
        self._apids = tuple(int(a) for a in apids)
        self._period = int(period)
        if len(self._apids) != 3 or len(set(self._apids)) != 3 or self._period < 1:
            raise ValueError("%s: three different channel APIDs and a period >= 1 expected" % type(self).__name__)

    @property
    def getImage(self):
        """The picture, uint8[H, 1568, 3]: the three channel planes in `apids` order, 8 rows per strip cycle, zero wherever no packet
        was placed"""
        return self._decode_image()[0]

    def getChannel(self, apid):
        """One channel's plane, uint8[H, 1568]"""
        if apid not in self._apids:
            raise ValueError("%s.getChannel: APID %r is none of %r" % (type(self).__name__, apid, self._apids))
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
        """Per frame (lrpt.INFO): symbol (of the marker's first bit), sample (the walk's A sample of that symbol; -1 where there is
        no walk), hypothesis, asm_score (of 52), asm_errors (of 32 decoded marker bits), corrected (channel bits the decoder
        changed), vcid, counter"""
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

    def _lrpt_starts(self, soft, nsym):
        """the frame starts int64[m, 3] = (symbol, hypothesis, asm_score) among the soft pairs"""
        return lrpt.frame_starts(lrpt.asm_candidates(soft, nsym, template=self._template), nsym)

    def _decode_frames(self):
        if self._frames is not None:
            return self._frames
        self._lrpt_prepare()
        t0 = time.perf_counter()

        def lap(name):
            nonlocal t0
            _hip.sync()
            now = time.perf_counter()
            self.timings["lrpt_" + name] = now - t0
            t0 = now
        soft, nsym, samples = self._lrpt_soft()
        lap("soft")
        starts = self._lrpt_starts(soft, nsym)
        lap("asm")
        bits = lrpt.viterbi(soft, nsym, starts[:, :2])
        lap("viterbi")
        bodies, fin = lrpt.finish(bits, soft, nsym, starts[:, :2], nrzm=self._nrzm)
        info = np.zeros(len(starts), dtype=lrpt.INFO)
        info["symbol"], info["hypothesis"], info["asm_score"] = starts[:, 0], starts[:, 1], starts[:, 2]
        info["asm_errors"], info["corrected"], info["vcid"] = fin[:, 0], fin[:, 1], fin[:, 2]
        info["sample"] = samples(starts[:, 0])
        info["counter"] = [lrpt.vcdu_header(b)["counter"] for b in bodies]
        lap("finish")
        self._frames = (bodies, info)
        return self._frames


class decode_lrpt(LrptChain):
    """decode_lrpt(soft, *, differential=False, interleaved=False, branches=36, delay=2048, apids=..., period=..., stagger=0): `soft` is a path
    to a soft-symbol file, an int8 NumPy array of I, Q pairs or a device int8 array of them.
    differential: the data are NRZ-M coded in front of the convolutional encoder (the N2-x satellites).
    interleaved: the 80 ksym/s mode -- the code bits pass a convolutional interleaver of `branches` branches and `delay` bits per
    branch step and come in groups of 72 behind the marker 0x27.  `locked`: whether the marker was found (at least 3/4 of the counted
    markers' bits match at the best offset and hypothesis); a stream that is not locked gives zero frames.  `deintInfo`: one
    lrpt.DEINT_INFO record per segment of 256 periods.  Without `interleaved`, `locked` is True and `deintInfo` is empty.
    stagger: the rails of an OQPSK demodulator's output may lie one symbol apart.  0, -1 or +1 decodes the
    pairs (I[k], Q[k + stagger]); "auto" tries 0, -1, +1 in that order and keeps the stream whose frame starts have the largest
    sum of asm_score -- with `interleaved`, the largest marker score of the lock -- the earlier one among equals.  `stagger` (the
    attribute) is the one used; with "auto" the three marker searches' time is timings["lrpt_stagger"] (and lrpt_deint_scores is
    not set: the chosen candidate's lock is reused).
    The results are LrptChain's, with the dtypes of decode_meteorm2's; frameInfo['sample'] is -1 (there is no walk) and
    frameInfo['symbol'] counts in the deinterleaved stream when `interleaved`."""

    def __init__(self, soft, *, differential=False, interleaved=False, branches=lrpt.INTERLEAVER_BRANCHES, delay=lrpt.INTERLEAVER_DELAY,
                 apids=lrpt.IMAGE_APIDS, period=lrpt.IMAGE_PERIOD, stagger=0):
        self._init_chain(apids, period, differential)
        if isinstance(stagger, bool) or stagger not in (0, -1, 1, "auto"):
            raise ValueError("decode_lrpt: a stagger of 0, -1, +1 or \"auto\" expected, got %r" % (stagger,))
        self._stagger_arg = stagger
        self._stagger = None
        self._starts = None
        self.timings = {}
        self._interleaved = bool(interleaved)
        self._branches, self._delay = int(branches), int(delay)
        lrpt._check_interleaver(self._branches, self._delay)
        if isinstance(soft, (str, os.PathLike)):
            soft = lrpt.read_soft(soft)
        if isinstance(soft, _hip.DevArray):
            if soft.dtype != np.dtype(np.int8):
                raise TypeError("decode_lrpt: int8 device array expected, got %s" % soft.dtype)
        else:
            soft = np.asarray(soft)
            if soft.dtype != np.dtype(np.int8) or soft.ndim != 1:
                raise TypeError("decode_lrpt: a path, an int8 array of I, Q pairs or a device int8 array expected")
        self._input = soft
        self._lock = None

    @property
    def locked(self):
        """True when the interleaver's marker was found (always True without `interleaved`)"""
        return self._deint()[0]["locked"]

    @property
    def deintInfo(self):
        """Per segment of 256 marker periods (lrpt.DEINT_INFO): score and markers counted at the lock, and the segment's own best
        offset, hypothesis and best_score -- where they differ from the lock, the stream slipped"""
        return self._deint()[0]["info"]

    @property
    def stagger(self):
        """The stagger the stream was decoded with: the keyword's, or the one "auto" chose"""
        self._deint()
        return self._stagger

    @property
    def lock(self):
        """lrpt.deint_lock's dict: offset, hypothesis, score, markers, groups, locked"""
        return {k: v for k, v in self._deint()[0].items() if k != "info"}

    def _deint(self):
        """(the lock, the device soft pairs the frame chain reads, their count)"""
        if self._lock is not None:
            return self._lock
        _hip.require_gpu()
        soft = self._input if isinstance(self._input, _hip.DevArray) else _hip.DevArray.from_host(self._input)
        nsym = soft.n // 2
        self._input = soft
        if self._stagger_arg == "auto":
            return self._deint_auto(soft, nsym)
        self._stagger = self._stagger_arg
        if self._stagger:
            soft = lrpt.restagger(soft, nsym, self._stagger)
            nsym = soft.n // 2
        if not self._interleaved:
            self._lock = (dict(offset=0, hypothesis=0, score=0, markers=0, groups=0, locked=True, info=np.zeros(0, dtype=lrpt.DEINT_INFO)),
                          soft, nsym)
            return self._lock
        t0 = time.perf_counter()
        lock = lrpt.deint_lock(lrpt.deint_scores(soft, nsym), nsym)
        _hip.sync()
        t1 = time.perf_counter()
        if lock["locked"]:
            out = lrpt.deint(soft, nsym, lock["offset"], lock["hypothesis"], self._branches, self._delay)
        else:
            out = soft.view(0, 0)
        _hip.sync()
        self.timings["lrpt_deint_scores"], self.timings["lrpt_deinterleave"] = t1 - t0, time.perf_counter() - t1
        self._lock = (lock, out, out.n // 2)
        return self._lock

    def _deint_auto(self, soft, nsym):
        """stagger="auto": the three candidate streams, each through the marker search of its mode, and the best of them"""
        t0 = time.perf_counter()
        tried = []
        for s in lrpt.STAGGERS:
            cand = lrpt.restagger(soft, nsym, s) if s else soft
            n = cand.n // 2
            if self._interleaved:
                found = lrpt.deint_lock(lrpt.deint_scores(cand, n), n)
                tried.append((found["score"], cand, n, found))
            else:
                found = LrptChain._lrpt_starts(self, cand, n)
                tried.append((int(found[:, 2].sum()), cand, n, found))
        self._stagger = lrpt.stagger_pick([t[0] for t in tried])
        _, cand, n, found = tried[lrpt.STAGGERS.index(self._stagger)]
        _hip.sync()
        self.timings["lrpt_stagger"] = time.perf_counter() - t0
        if not self._interleaved:
            self._starts = found
            self._lock = (dict(offset=0, hypothesis=0, score=0, markers=0, groups=0, locked=True, info=np.zeros(0, dtype=lrpt.DEINT_INFO)),
                          cand, n)
            return self._lock
        t1 = time.perf_counter()
        out = lrpt.deint(cand, n, found["offset"], found["hypothesis"], self._branches, self._delay) if found["locked"] else cand.view(0, 0)
        _hip.sync()
        self.timings["lrpt_deinterleave"] = time.perf_counter() - t1      # (the three marker searches are in lrpt_stagger)
        self._lock = (found, out, out.n // 2)
        return self._lock

    def _lrpt_starts(self, soft, nsym):
        return self._starts if self._starts is not None else super()._lrpt_starts(soft, nsym)

    def _lrpt_prepare(self):
        self._deint()

    def _lrpt_soft(self):
        _, soft, nsym = self._deint()
        return soft, nsym, lambda symbols: np.full(len(symbols), -1, dtype=np.int64)
