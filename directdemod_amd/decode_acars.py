"""
ACARS message decoding on VHF, several channels of one recording (beyond the reference): per channel
decode_ais's front end (the fused offsetFreq -> blackmanHarris -> bwLim chain per chunk, a channel low-pass at the audio rate) and
the magnitude of the complex signal in float64 (dd_abs_f64) instead of the discriminator; then every audio sample is tested as the
start of a block on the device (acars.candidates: the 32 bits of * SYN SYN SOH, each a difference of two half-bit sums from an LDS
prefix sum), the survivors are demodulated one wave each (acars.blocks: 240 characters, the end, the block check sequence, repair
guided by the characters' parity), and only that short list comes down.  The accepted candidates of one block are merged, parsed
and joined into messages on the host (acars.decode, acars.messages).

A block starts cold behind a short pre-key: nothing has to pull in, so every block is timed from its own template.
INTEGRATION.md lists the limits.
"""
import logging

import numpy as np

from . import _channel, _hip, acars
from .decode_ais import channel_names


def _rates(rate, fs=None):
    """ValueError unless the audio rate gives 8 to 64 samples per bit"""
    try:
        acars.params(rate)
    except ValueError:
        if fs is None:
            raise
        raise ValueError("decode_acars: a recording at %r S/s gives an audio rate of %r S/s, %r samples per bit at %d baud; %g to %g "
                         "are supported" % (fs, rate, rate / float(acars.BAUD), acars.BAUD, acars.SPS_MIN, acars.SPS_MAX)) from None


class decode_acars:
    """Object to decode ACARS: decode_acars(sigsrc, offsets, bw, cut, slack, fix, use_device_raw).  offsets: one frequency offset per
    channel with decode_afsk1200's sign, labelled A, B, .. in their order.  bw None -> 48 000; the audio rate fs / int(fs / bw) must
    give 8 to 64 samples per bit (ValueError otherwise).  cut: the channel filter's cut-off in Hz (None -> 5000: the next channel's
    carrier lies 25 kHz away and would beat in the envelope).  slack: template places of the 32 that may differ (0 .. 5).  fix: bits
    repaired per block (0 .. 2).  use_device_raw: read the recording as raw u8 pairs resident on the device when the source offers it
    (source.read_device_raw)."""

    def __init__(self, sigsrc, offsets, bw=None, cut=None, slack=2, fix=2, use_device_raw=True):
        bw = 48000 if bw is None else bw
        cut = acars.CUT if cut is None else float(cut)
        self.__offsets = [float(o) for o in np.atleast_1d(offsets)]
        self.__channels = channel_names(len(self.__offsets))
        self.__front = None
        self.__audios = None
        self.__slack, self.__fix = slack, fix
        acars.params(acars.BAUD * acars.SPS_MIN, None, slack, fix)           # ValueError for a slack or a fix out of range
        if sigsrc is not None:
            self.__front = _channel.Channels("decode_acars", sigsrc, self.__offsets, bw, cut, use_device_raw,
                                             lambda rate: _rates(rate, sigsrc.sampFreq))
            self.__rate = self.__front.rate
        self.__done = False
        self.__blocks = []
        self.__info = {}
        self.__cand = {}
        self.timings = {}                  # seconds per stage of the last decode (front end, candidates, blocks, host)

    @classmethod
    def fromAudio(cls, audio, rate, channel="A", slack=2, fix=2):
        """The decoder over one channel's AM-demodulated audio (NumPy or float64 device array: an envelope, or an AM receiver's
        audio output, in either polarity) at `rate` S/s: no front end."""
        _rates(rate)
        obj = cls(None, (0.0,), None, None, slack, fix)
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
        """1 if at least one block was decoded, else 0"""
        self._decode()
        return 1 if self.__blocks else 0

    @property
    def getBlocks(self):
        """one dict per block in time order: t (seconds), start (the audio sample of the template), channel, mode, address, ack
        (None for NAK), label, block_id, downlink, msgno, flight, text, more (ETB: more blocks follow), corrected (bits repaired),
        parity_errors (characters whose parity failed as received), polarity, score, closed (DEL behind the block check), bytes (the
        characters from the mode through the block check, parity bits on)"""
        self._decode()
        return [dict(b) for b in self.__blocks]

    @property
    def getMessages(self):
        """the blocks joined into messages (acars.messages): t, channel, address, label, msgno, flight, text, blocks, complete"""
        self._decode()
        return acars.messages(self.__blocks)

    @property
    def getText(self):
        """every block as a line like ACARS A: Mode: 2 Reg: G-ABCD Ack: ! Label: H1 Block: 3 ... Text: ..."""
        self._decode()
        return [acars.line(b) for b in self.__blocks]

    @property
    def frameInfo(self):
        """samples (of the audio), blocks, and per channel: candidates (that passed the sync test), accepted (blocks kept),
        duplicates (accepted candidates merged into another of their block), over all candidates outside, no_end, bad_bcs, and over
        the accepted ones by route: clean, one_character, bcs, two_characters"""
        self._decode()
        info = dict(self.__info)
        info["channels"] = {ch: dict(v) for ch, v in info["channels"].items()}
        return info

    @property
    def candidateInfo(self):
        """per channel, every candidate that passed the sync test, accepted or not: a dict of arrays t, bytes, status, polarity,
        mis, end, flags, repaired, del, residual, score"""
        self._decode()
        return {ch: {key: v.copy() for key, v in det.items()} for ch, det in self.__cand.items()}

    # ------------------------------------------------------------------ the device pipeline
    def audio(self):
        """the channels' envelopes as float64 device arrays (the front end runs once)"""
        _hip.require_gpu()
        if self.__audios is None:
            self.__audios = self.__front.audios(lambda sig: _magnitude(sig.device_signal))
        self.__audios = _channel.on_device(self.__audios)
        return self.__audios

    def _decode(self):
        if self.__done:
            return
        _hip.require_gpu()
        ops = acars.DeviceOps({})
        audios = self.audio()
        ops.lap("front_end")
        self.__blocks, self.__info, self.__cand = acars.decode(audios, self.__rate, self.__channels, self.__slack, self.__fix, ops=ops)
        self.timings = ops.finish("candidates", "blocks", "host")
        for b in self.__blocks:
            logging.info("%s (at %.4f s, %d bits repaired)", acars.line(b), b["t"], b["corrected"])
        self.__done = True


def _magnitude(d):
    """|d| of a complex device signal as float64 (dd_abs_f64)"""
    from .comm import flush_all
    flush_all()
    kind = {np.dtype(np.complex128): 1, np.dtype(np.complex64): 2}.get(d.dtype)
    if kind is None:
        raise TypeError("decode_acars: a complex signal expected, got %s" % d.dtype)
    mag = _hip.DevArray(d.n, np.float64)
    _hip.check(_hip.lib().dd_abs_f64(d.ptr, kind, mag.ptr, d.n, None), "dd_abs_f64")
    return mag


def decode_host(raw, fs, offsets, bw=None, cut=None, slack=2, fix=2):
    """(blocks, frameInfo, messages) of a uint8[N, 2] recording by the NumPy restatement of the front end (acars.audio_host,
    float64) and of both kernels"""
    bw = 48000 if bw is None else bw
    offsets = [float(o) for o in np.atleast_1d(offsets)]
    audios, rate = [], None
    for o in offsets:
        x, rate = acars.audio_host(raw, fs, o, bw, acars.CUT if cut is None else cut)
        audios.append(x)
    found, info, _ = acars.decode(audios, rate, channel_names(len(offsets)), slack, fix)
    return found, info, acars.messages(found)


def decode_audio_host(audio, rate, channel="A", slack=2, fix=2):
    """(blocks, frameInfo, messages) of one channel's audio by the restatement of both kernels"""
    found, info, _ = acars.decode([np.ascontiguousarray(audio, dtype=np.float64).ravel()], rate, [channel], slack, fix)
    return found, info, acars.messages(found)
