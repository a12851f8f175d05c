"""
Vaisala RS41 radiosonde telemetry decoding (beyond the reference): decode_pocsag's front end with its own
cut-off (the fused offsetFreq -> blackmanHarris -> bwLim chain per chunk, a channel low-pass at the audio rate and demod_fm over the
whole signal); then every audio sample is tested as the start of a frame on the device (rs41.candidates: the 64 bits of the header
from an LDS prefix sum against the midpoint of their two classes), the survivors are demodulated one wave each (rs41.frames: 2560 or
4144 bits, the whitening mask, two RS(255,231) codewords through the Reed-Solomon wave), and only that short list comes down.  The
frames are merged, followed from second to second and parsed on the host (rs41.decode).

Every frame carries its own header: nothing has to pull in, so a recording that starts inside a frame is decoded from the next one
on.  The format is taken from public descriptions and has been met in synthesised recordings only; INTEGRATION.md lists the limits.
"""
import logging

import numpy as np

from . import _channel, _hip, rs41

_KEYS = ("t", "start", "status", "extended", "polarity", "frame_number", "serial", "battery", "gps_week", "gps_tow", "time", "lat", "lon",
         "alt", "speed", "heading", "climb", "sats", "meas_raw", "xdata", "blocks", "corrected", "header_errors", "followed")


def _public(f):
    out = {k: f[k] for k in _KEYS}
    out["blocks"] = [dict(b) for b in f["blocks"]]
    return out


def _sondes(found):
    return {s: {"first": v["first"], "last": v["last"], "frames": v["frames"], "position": v["position"],
                "calibration": v["calibration"].copy(), "seen": v["seen"].copy()} for s, v in rs41.assemble(found).items()}


def _track(found):
    out = {}
    for f in found:
        if f["serial"] is not None and f["lat"] is not None:
            out.setdefault(f["serial"], []).append((f["time"], f["lat"], f["lon"], f["alt"]))
    return out


class decode_rs41:
    """Object to decode RS41 telemetry: decode_rs41(sigsrc, offset, bw, cut, slack, follow, use_device_raw).  offset: the channel's
    frequency offset with decode_afsk1200's sign.  bw None -> 48 000; the audio rate fs / int(fs / bw) must give 4 to 64 samples per
    bit at 4800 baud (ValueError otherwise).  cut: the channel filter's cut-off in Hz (None -> rs41.CUT).  slack: places of the
    header's 64 that may differ (0 .. 11).  follow: frames taken in a row at their predicted start, one second after the frame
    before, when the header test found nothing there.  use_device_raw: read the recording as raw u8 pairs resident on the device
    when the source offers it (source.read_device_raw)."""

    def __init__(self, sigsrc, offset, bw=None, cut=None, slack=4, follow=2, use_device_raw=True):
        bw = 48000 if bw is None else bw
        cut = rs41.CUT if cut is None else float(cut)
        self.__opts = {"slack": slack, "follow": follow}
        self.__front = None
        self.__audio = None
        if int(follow) != follow or follow < 0:
            raise ValueError("decode_rs41: follow must be a count from 0 up, got %r" % (follow,))
        if sigsrc is not None:
            self.__front = _channel.Channels("decode_rs41", sigsrc, [offset], bw, cut, use_device_raw,
                                             lambda rate: rs41.params(rate, None, slack))    # (4 to 64 samples per bit)
            self.__rate = self.__front.rate
        self.__done = False
        self.__frames = []
        self.__info = {}
        self.__cand = {}
        self.timings = {}                  # seconds per stage of the last decode (front_end, candidates, frames, host)

    @classmethod
    def fromAudio(cls, audio, rate, slack=4, follow=2):
        """The decoder over FM-demodulated audio (NumPy or float64 device array, radians per sample) at `rate` S/s: no front end."""
        rs41.params(rate, None, slack)
        obj = cls(None, 0.0, None, None, slack, follow)
        obj.__rate = rate
        obj.__audio = audio if isinstance(audio, _hip.DevArray) else np.ascontiguousarray(audio, dtype=np.float64).ravel()
        return obj

    @property
    def audioRate(self):
        """samples per second of the audio the kernels read"""
        return self.__rate

    @property
    def useful(self):
        """1 if at least one frame was decoded, else 0"""
        self._decode()
        return 1 if self.__frames else 0

    @property
    def getFrames(self):
        """one dict per frame in time order: t (seconds), start (the audio sample of the header), status (ok: both codewords decoded;
        partial: not both, and only the blocks whose CRC holds are parsed), extended, polarity, frame_number, serial, battery (V),
        gps_week, gps_tow (ms), time (GPS time, ISO), lat, lon (degrees, WGS-84), alt (m), speed, heading, climb (m/s, degrees),
        sats, meas_raw (twelve 24-bit counts), xdata (bytes or None), blocks (id, crc_ok, bytes), corrected (bytes changed per
        codeword, -1: not decodable), header_errors, followed; a field whose block is missing is None"""
        self._decode()
        return [_public(f) for f in self.__frames]

    @property
    def getTrack(self):
        """per serial a list of (time, lat, lon, alt) of the frames whose GPSPOS block is valid"""
        self._decode()
        return _track(self.__frames)

    @property
    def getSondes(self):
        """per serial: first and last frame number, frames, position (the last lat, lon, alt), calibration uint8[51, 16] and seen
        bool[51], the subframes met"""
        self._decode()
        return _sondes(self.__frames)

    @property
    def getRaw(self):
        """(uint8[n, 518] frames, de-whitened and corrected, zero past their length; int64[n] lengths)"""
        self._decode()
        f = self.__frames
        return (np.array([x["raw"] for x in f], dtype=np.uint8).reshape(len(f), rs41.EXT), np.array([x["length"] for x in f], dtype=np.int64))

    @property
    def frameInfo(self):
        """samples (of the audio), candidates (that passed the header test), duplicates (candidates merged into another of their
        frame), dropped (neither ok nor partial), followed (frames taken at their predicted start), frames, ok, partial"""
        self._decode()
        return dict(self.__info)

    @property
    def candidateInfo(self):
        """every candidate that passed the header test, kept or not: a dict of arrays t, fixed, recv, status, polarity, length, mis,
        errs"""
        self._decode()
        return {key: v.copy() for key, v in self.__cand.items()}

    # ------------------------------------------------------------------ the device pipeline
    def audio(self):
        """the FM-demodulated audio as a float64 device array (the front end runs once)"""
        _hip.require_gpu()
        if self.__audio is None:
            self.__audio, = self.__front.audios(_channel.fm_audio)
        self.__audio, = _channel.on_device([self.__audio])
        return self.__audio

    def _decode(self):
        if self.__done:
            return
        _hip.require_gpu()
        ops = rs41.DeviceOps({})
        audio = self.audio()
        ops.lap("front_end")
        self.__frames, self.__info, self.__cand = rs41.decode(audio, self.__rate, ops=ops, **self.__opts)
        self.timings = ops.finish("candidates", "frames", "host")
        for f in self.__frames:
            logging.info("RS41 %s frame %s at %.4f s: %s, %s", f["serial"], f["frame_number"], f["t"], f["status"],
                         "no position" if f["lat"] is None else "%.5f %.5f %.1f m" % (f["lat"], f["lon"], f["alt"]))
        self.__done = True


def decode_host(raw, fs, offset, bw=None, cut=None, slack=4, follow=2):
    """(frames, frameInfo) of a uint8[N, 2] recording by the NumPy restatement of the front end (rs41.audio_host, float64) and of
    both kernels"""
    audio, rate = rs41.audio_host(raw, fs, float(offset), 48000 if bw is None else bw, rs41.CUT if cut is None else cut)
    return decode_audio_host(audio, rate, slack, follow)


def decode_audio_host(audio, rate, slack=4, follow=2):
    """(frames, frameInfo) of FM-demodulated audio by the restatement of both kernels; the frames as getFrames gives them"""
    found, info, _ = rs41.decode(np.ascontiguousarray(audio, dtype=np.float64).ravel(), rate, slack, follow)
    return [_public(f) for f in found], info


def sondes_host(frames):
    """getSondes of decode_audio_host's frames"""
    out = []
    for f in frames:
        g = dict(f)
        st = [b for b in f["blocks"] if b["id"] == rs41.BLOCK_STATUS and b["crc_ok"]]
        g["subframe"], g["calibration"] = (st[0]["bytes"][0x17], bytes(st[0]["bytes"][0x18:0x28])) if st else (None, None)
        out.append(g)
    return _sondes(out)
