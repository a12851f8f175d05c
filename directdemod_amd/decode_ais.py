"""
AIS message decoding, both channels (beyond the reference): per channel decode_afsk1200's front end (the fused
offsetFreq -> blackmanHarris -> bwLim chain per chunk), a channel low-pass at the audio rate (filters.lowpass) and demod_fm over the
whole signal; then every audio sample is tested as the start of a burst on the device (ais.candidates: 24 bit values from LDS
against the training bits' mean), the survivors are demodulated one wave each (ais.demod: NRZI, end flag, de-stuffing, CRC-16), and
only that short list comes down.  The accepted candidates of one burst are merged, parsed and armoured on the host (ais.decode).

A burst is a single transmission of 26.7 ms with 24 training bits in front: nothing has to pull in, so a burst that starts a
recording cold is decoded like any other.  INTEGRATION.md lists the limits.
"""
import logging

import numpy as np

from . import _channel, _hip, ais


def channel_names(count):
    return [chr(ord("A") + i) for i in range(count)]


class decode_ais:
    """Object to decode AIS: decode_ais(sigsrc, offsets, bw, cut, slack, use_device_raw).  offsets: one frequency offset per channel
    with decode_afsk1200's sign, labelled A, B, .. in their order (AIS 1 and AIS 2 lie 25 kHz below and above 162 MHz).  bw None ->
    48 000; the audio rate fs / int(fs / bw) must give 4 to 16 samples per bit (ValueError otherwise).  cut: the channel filter's
    cut-off in Hz (None -> 7000).  slack: template places of the 24 that may differ.
    use_device_raw: read the recording as raw u8 pairs resident on the device when the source offers it (source.read_device_raw)."""

    def __init__(self, sigsrc, offsets=(-25000.0, 25000.0), bw=None, cut=None, slack=0, use_device_raw=True):
        bw = 48000 if bw is None else bw
        cut = ais.CUT if cut is None else float(cut)
        self.__offsets = [float(o) for o in np.atleast_1d(offsets)]
        self.__channels = channel_names(len(self.__offsets))
        self.__front = None
        self.__audios = None
        self.__slack = slack
        if sigsrc is not None:
            self.__front = _channel.Channels("decode_ais", sigsrc, self.__offsets, bw, cut, use_device_raw,
                                             lambda rate: ais.params(rate, None, slack))     # (4 to 16 samples per bit)
            self.__rate = self.__front.rate
        self.__done = False
        self.__msgs = []
        self.__info = {}
        self.__cand = {}
        self.timings = {}                  # seconds per stage of the last decode (front end, candidates, demod, host)

    @classmethod
    def fromAudio(cls, audio, rate, channel="A", slack=0):
        """The decoder over one channel's FM-demodulated audio (NumPy or float64 device array, radians per sample) at `rate` S/s:
        no front end."""
        ais.params(rate, None, slack)
        obj = cls(None, (0.0,), None, None, slack)
        obj.__rate = rate
        obj.__channels = [channel]
        obj.__audios = [audio if isinstance(audio, _hip.DevArray) else np.ascontiguousarray(audio, dtype=np.float64).ravel()]
        return obj

    @property
    def audioRate(self):
        """samples per second of the audio the kernels read"""
        return self.__rate

    @property
    def useful(self):
        """1 if at least one message was decoded, else 0"""
        self._decode()
        return 1 if self.__msgs else 0

    @property
    def getMsgs(self):
        """one dict per message in time order: t (seconds), start (the audio sample of the start flag), channel, type, mmsi, nbits,
        raw (the message's bytes without FCS), nmea (its sentences), score, repeat and the fields ais.parse finds for the type"""
        self._decode()
        return [dict(m) for m in self.__msgs]

    @property
    def getNMEA(self):
        """every message's !AIVDM sentences, in time order, as one flat list"""
        self._decode()
        return [s for m in self.__msgs for s in m["nmea"]]

    @property
    def getVessels(self):
        """{mmsi: {shipname, callsign, shiptype, destination, track}}: track is a list of (t, lat, lon, sog, cog) (ais.vessels)"""
        self._decode()
        return ais.vessels(self.__msgs)

    @property
    def getFrames(self):
        """(uint8[n, 158] message bytes, zero beyond their length; int64[n] lengths in bytes)"""
        self._decode()
        frames = np.zeros((len(self.__msgs), ais.FRAME_BYTES - 2), dtype=np.uint8)
        for i, m in enumerate(self.__msgs):
            frames[i, :len(m["raw"])] = np.frombuffer(m["raw"], dtype=np.uint8)
        return frames, np.array([len(m["raw"]) for m in self.__msgs], dtype=np.int64)

    @property
    def frameInfo(self):
        """samples (of the audio), candidates (that passed the preamble test), accepted (messages kept), duplicates (accepted
        candidates merged into another of their burst) and, over all candidates, no_end_flag, abort, stuffing_violation, bad_length,
        bad_crc"""
        self._decode()
        return dict(self.__info)

    @property
    def candidateInfo(self):
        """per channel, every candidate that passed the preamble test, accepted or not: a dict of int arrays t, status, nbits, rem,
        polarity, score"""
        self._decode()
        return {ch: {key: v.copy() for key, v in det.items() if key != "frames"} for ch, det in self.__cand.items()}

    # ------------------------------------------------------------------ the device pipeline
    def audio(self):
        """the channels' FM-demodulated audio as float64 device arrays (the front end runs once)"""
        _hip.require_gpu()
        if self.__audios is None:
            self.__audios = self.__front.audios(_channel.fm_audio)
        self.__audios = _channel.on_device(self.__audios)
        return self.__audios

    def _decode(self):
        if self.__done:
            return
        _hip.require_gpu()
        ops = ais.DeviceOps({})
        audios = self.audio()
        ops.lap("front_end")
        self.__msgs, self.__info, self.__cand = ais.decode(audios, self.__rate, self.__channels, self.__slack, ops=ops)
        self.timings = ops.finish()
        for m in self.__msgs:
            logging.info("AIS %s at %.4f s: type %d, MMSI %09d, %d bits: %s", m["channel"], m["t"], m["type"], m["mmsi"], m["nbits"],
                         " ".join(m["nmea"]))
        self.__done = True


def decode_host(raw, fs, offsets=(-25000.0, 25000.0), bw=None, cut=None, slack=0):
    """(messages, frameInfo, vessels) of a uint8[N, 2] recording by the NumPy restatement of the front end (ais.audio_host, float64)
    and of both kernels"""
    bw = 48000 if bw is None else bw
    offsets = [float(o) for o in np.atleast_1d(offsets)]
    audios, rate = [], None
    for o in offsets:
        x, rate = ais.audio_host(raw, fs, o, bw, ais.CUT if cut is None else cut)
        audios.append(x)
    msgs, info, _ = ais.decode(audios, rate, channel_names(len(offsets)), slack)
    return msgs, info, ais.vessels(msgs)


def decode_audio_host(audio, rate, channel="A", slack=0):
    """(messages, frameInfo, vessels) of one channel's audio by the restatement of both kernels"""
    msgs, info, _ = ais.decode([np.ascontiguousarray(audio, dtype=np.float64).ravel()], rate, [channel], slack)
    return msgs, info, ais.vessels(msgs)
