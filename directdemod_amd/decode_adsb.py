"""
1090 MHz Mode S / ADS-B squitter decoding (beyond the reference): every sample offset of an RTL-SDR style
u8 recording at 2 to 20 MS/s, times `phases` sub-sample offsets, is tested as a frame start on the device (adsb.candidates: chip
energies from LDS, thirteen strict comparisons), the survivors are demodulated one wave each (adsb.demod: bit decisions, CRC
remainder, one-bit repair), and only that short list comes down.  The acceptance and duplicate rules run on the host (adsb.accept).
There is no front end: the kernels read the raw pairs.

INTEGRATION.md lists the limits: recordings at exactly 2.0 MS/s lose frames whose pulses straddle two samples evenly, and rates
strictly between 2.0 and 2.4 MS/s lose most frames.
"""
import logging

import numpy as np

from . import _hip, adsb
from ._burst import Laps


class decode_adsb:
    """Object to decode Mode S: decode_adsb(sigsrc, phases, fix, use_device_raw).  phases None: the smallest of 1, 2, 4, 8 that
    gives at least 8 000 000 candidates per second.  fix 1: DF 17 / 18 frames with one repaired bit are accepted when their
    address also occurs in a frame that needed no repair.  piece: samples per walk step (the result does not depend on it).
    ValueError for a sample rate outside 2 .. 20 MS/s or another phases value."""

    PIECE = 1 << 24

    def __init__(self, sigsrc, phases=None, fix=1, use_device_raw=True, piece=None):
        self.__sigsrc = sigsrc
        self.__raw = None
        self.__rate, self.__Q = adsb.check_rate(sigsrc.sampFreq, phases) if sigsrc is not None else (None, phases)
        self.__fix = fix
        self.__use_raw = use_device_raw
        self.__piece = self.PIECE if piece is None else int(piece)
        if not 1 <= self.__piece <= 1 << 27:                         # (dd_adsb_candidates takes fewer than 2^28 samples a call)
            raise ValueError("decode_adsb: piece must be from 1 to 2^27 samples")
        self.__done = False
        self.__msgs = []
        self.__info = {}
        self.__cand = None
        self.timings = {}                  # seconds per stage of the last decode

    @classmethod
    def fromIQ(cls, raw, rate, phases=None, fix=1, piece=None):
        """The decoder over raw pairs: a uint8[N, 2] array or a device array of _hip.IQ8, at `rate` samples per second"""
        obj = cls(None, phases, fix, True, piece)
        obj.__rate, obj.__Q = adsb.check_rate(rate, phases)
        if isinstance(raw, _hip.DevArray):
            if raw.dtype != _hip.IQ8:
                raise TypeError("decode_adsb.fromIQ: a device array of _hip.IQ8 expected, got %s" % raw.dtype)
            obj.__raw = raw
        else:
            raw = np.ascontiguousarray(raw, dtype=np.uint8)
            if raw.ndim != 2 or raw.shape[1] != 2:
                raise TypeError("decode_adsb.fromIQ: a uint8 array of shape [N, 2] expected")
            obj.__raw = raw
        return obj

    @property
    def useful(self):
        """1 if at least one message was decoded, else 0"""
        self._decode()
        return 1 if self.__msgs else 0

    @property
    def getMsgs(self):
        """one dict per message in time order: t (seconds), start (samples), df, icao (six hex digits), raw (bytes), fixed (the
        repaired bit or -1), score, tc (DF 17 / 18, else None) and the fields adsb.parse finds for the type code"""
        self._decode()
        return [dict(m) for m in self.__msgs]

    @property
    def getFrames(self):
        """(uint8[n, 14] frames, zero beyond their length; int64[n] lengths in bytes)"""
        self._decode()
        frames = np.zeros((len(self.__msgs), 14), dtype=np.uint8)
        for i, m in enumerate(self.__msgs):
            frames[i, :len(m["raw"])] = np.frombuffer(m["raw"], dtype=np.uint8)
        return frames, np.array([len(m["raw"]) for m in self.__msgs], dtype=np.int64)

    @property
    def getAircraft(self):
        """{icao: {callsign, velocity, track}}: track is a list of (t, lat, lon, alt) (adsb.aircraft)"""
        self._decode()
        return adsb.aircraft(self.__msgs)

    @property
    def frameInfo(self):
        """samples, candidates, passed (the preamble test), clean, repaired, address_parity (messages kept, by how they were
        accepted), duplicates, phases"""
        self._decode()
        return dict(self.__info)

    @property
    def candidateInfo(self):
        """every candidate that passed the preamble test, accepted or not: a dict of int arrays k, L, df, rem, fixed, score"""
        self._decode()
        return {key: v.copy() for key, v in self.__cand.items() if key != "frames"}

    def _pieces(self, n):
        """(first sample, samples) per walk step: a step's candidates start inside its first `piece` samples, and it reads on to the
        end of the last one's 240 chips"""
        ext = adsb.reach(self.__rate)
        return [(a, min(n, a + self.__piece + ext) - a) for a in range(0, max(n, 1), self.__piece)]

    def _view(self, a, count):
        if self.__raw is None:
            v = self.__sigsrc.read_device_raw(a, a + count) if self.__use_raw else None
            return v if v is not None else adsb.to_device(self.__sigsrc.read_raw_u8(a, a + count))
        if not isinstance(self.__raw, _hip.DevArray):
            self.__raw = adsb.to_device(self.__raw)
        return self.__raw.view(a, count)

    def _decode(self):
        if self.__done:
            return
        _hip.require_gpu()
        laps = {}
        lap = Laps(laps).lap
        rate, Q = self.__rate, self.__Q
        n = self.__sigsrc.length if self.__raw is None else (self.__raw.n if isinstance(self.__raw, _hip.DevArray) else len(self.__raw))
        dets, passed = [], 0
        for a, count in self._pieces(n) if n else []:
            iq = self._view(a, count)
            lap("upload")
            lst, m = adsb.candidates(iq, rate, Q)
            lap("candidates")
            ks = lst.view(0, m).to_host() if m else np.zeros(0, dtype=np.int64)
            m = int(np.searchsorted(ks, self.__piece * Q))           # (those past the step's own starts belong to the next step)
            det = adsb.demod(iq, rate, Q, lst, m)
            det["k"] = det["k"] + a * Q
            lap("demod")
            dets.append(det)
            passed += m
        det = adsb.concat_det(dets)
        self.__msgs, self.__info = finish(det, passed, n, rate, Q, self.__fix)
        self.__cand = det
        lap("host")
        self.timings = laps
        logging.info("ADS-B: %d messages from %d candidates (%d passed the preamble test)", len(self.__msgs),
                     self.__info["candidates"], passed)
        self.__done = True


def finish(det, passed, n, rate, Q, fix=1):
    """The host end of the decoder over a recording's detections (device or restatement): (messages, frameInfo)"""
    msgs, counts = adsb.accept(det, rate, Q, fix)
    out = []
    for m in msgs:
        f = adsb.parse(m["raw"])
        f.update(t=m["k"] / float(Q * rate), start=m["k"] / float(Q), icao="%06X" % m["icao"], raw=m["raw"], fixed=m["fixed"],
                 score=m["score"])
        out.append(f)
    info = {"samples": int(n), "candidates": adsb.n_candidates(n, rate, Q), "passed": int(passed), "phases": Q}
    info.update(counts)
    return out, info


def decode_host(raw, rate, phases=None, fix=1):
    """(messages, frameInfo, aircraft) of a uint8[N, 2] recording by the NumPy restatement of both kernels"""
    rate, Q = adsb.check_rate(rate, phases)
    det, passed = adsb.detect_host(raw, rate, Q)
    msgs, info = finish(det, passed, len(raw), rate, Q, fix)
    return msgs, info, adsb.aircraft(msgs)
