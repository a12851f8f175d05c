"""
POCSAG pager decoding at 512, 1200 and 2400 baud (beyond the reference): decode_ais's front end for one channel
(the fused offsetFreq -> blackmanHarris -> bwLim chain per chunk, a channel low-pass at the audio rate and demod_fm over the whole
signal); then, per baud rate, every audio sample is tested as the start of a batch on the device (pocsag.candidates: the 32 bits of
the frame sync codeword from an LDS prefix sum against their own mean), the survivors are demodulated one wave each (pocsag.batches:
544 bits, polarity, BCH(31,21) correction of up to two bits per codeword), and only that short list comes down.  The batches are
merged, chained into transmissions and parsed into pages on the host (pocsag.decode).

Every batch carries its own sync codeword: nothing has to pull in, so a recording that starts inside a transmission is decoded
from its next batch on.  INTEGRATION.md lists the limits.
"""
import logging

import numpy as np

from . import _channel, _hip, pocsag


class decode_pocsag:
    """Object to decode POCSAG: decode_pocsag(sigsrc, offset, bw, bauds, cut, slack, fix, follow, content, use_device_raw).  offset:
    the channel's frequency offset with decode_afsk1200's sign.  bw None -> 48 000; the audio rate fs / int(fs / bw) must give 4 to
    128 samples per bit at every baud rate of `bauds` (ValueError otherwise).  cut: the channel filter's cut-off in Hz (None -> 7000).
    slack: places of the sync codeword's 32 that may differ (0 .. 8).  fix: bit errors repaired per codeword (0 .. 2).  follow: batches
    taken in a row at their predicted start after a sync codeword was lost.  content: auto, numeric or alpha.
    use_device_raw: read the recording as raw u8 pairs resident on the device when the source offers it (source.read_device_raw)."""

    def __init__(self, sigsrc, offset, bw=None, bauds=pocsag.BAUDS, cut=None, slack=2, fix=2, follow=2, content="auto",
                 use_device_raw=True):
        bw = 48000 if bw is None else bw
        cut = pocsag.CUT if cut is None else float(cut)
        self.__bauds = tuple(bauds)
        self.__opts = {"slack": slack, "fix": fix, "follow": follow, "content": content}
        self.__front = None
        self.__audio = None
        if content not in ("auto", "numeric", "alpha"):
            raise ValueError("decode_pocsag: content must be auto, numeric or alpha, got %r" % (content,))
        if int(follow) != follow or follow < 0:
            raise ValueError("decode_pocsag: follow must be a count from 0 up, got %r" % (follow,))
        if sigsrc is not None:
            def check_rate(rate):                  # ValueError unless it gives 4 to 128 samples per bit
                for baud in self.__bauds:
                    pocsag.params(rate, baud, None, slack, fix)
            self.__front = _channel.Channels("decode_pocsag", sigsrc, [offset], bw, cut, use_device_raw, check_rate)
            self.__rate = self.__front.rate
        self.__done = False
        self.__pages = []
        self.__info = {}
        self.__cand = {}
        self.__batches = []
        self.timings = {}                  # seconds per stage of the last decode (front end, candidates, batches, host)

    @classmethod
    def fromAudio(cls, audio, rate, bauds=pocsag.BAUDS, slack=2, fix=2, follow=2, content="auto"):
        """The decoder over FM-demodulated audio (NumPy or float64 device array, radians per sample) at `rate` S/s: no front end."""
        for baud in bauds:
            pocsag.params(rate, baud, None, slack, fix)
        obj = cls(None, 0.0, None, bauds, None, slack, fix, follow, content)
        obj.__rate = rate
        obj.__audio = audio if isinstance(audio, _hip.DevArray) else np.ascontiguousarray(audio, dtype=np.float64).ravel()
        return obj

    @property
    def audioRate(self):
        """samples per second of the audio the kernels read"""
        return self.__rate

    @property
    def useful(self):
        """1 if at least one page was decoded, else 0"""
        self._decode()
        return 1 if self.__pages else 0

    @property
    def getPages(self):
        """one dict per page in time order: t (seconds), start (the audio sample of the address codeword), baud, polarity, address,
        function, nbits, bits (the message's 20-bit fields as bytes), numeric, alpha, text (the one of the two that `kind` names),
        kind (tone, numeric, alpha), complete (False when an uncorrectable codeword cut the message), corrected (bits repaired),
        batches (how many the page spans)"""
        self._decode()
        return [dict(p) for p in self.__pages]

    @property
    def getText(self):
        """every page as a line like POCSAG1200: Address: 1234567 Function: 3 Alpha: ..."""
        self._decode()
        return [pocsag.line(p) for p in self.__pages]

    @property
    def getBatches(self):
        """(uint32[n, 17] codewords, uint8[n, 17] error counts, int64[n] start samples, int64[n] baud rates) of the batches kept, in
        time order"""
        self._decode()
        b = self.__batches
        return (np.array([x["words"] for x in b], dtype=np.uint32).reshape(len(b), pocsag.WORDS),
                np.array([x["errs"] for x in b], dtype=np.uint8).reshape(len(b), pocsag.WORDS),
                np.array([x["t"] for x in b], dtype=np.int64), np.array([x["baud"] for x in b], dtype=np.int64))

    @property
    def frameInfo(self):
        """samples (of the audio); bauds: per baud rate candidates (that passed the sync test), accepted (batches kept), duplicates
        (accepted candidates merged into another of their batch), followed (batches taken at their predicted start); overlaps
        (batches dropped for one of another baud rate), batches, transmissions; codewords by errors repaired, uncorrectable, idle,
        orphans (message codewords with no page open); pages"""
        self._decode()
        info = dict(self.__info)
        info["bauds"] = {b: dict(v) for b, v in info["bauds"].items()}
        info["codewords"] = dict(info["codewords"])
        return info

    @property
    def candidateInfo(self):
        """per baud rate, every candidate that passed the sync test, accepted or not: a dict of arrays t, words, errs, status,
        polarity, good, mis, score"""
        self._decode()
        return {baud: {key: v.copy() for key, v in det.items()} for baud, det in self.__cand.items()}

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
        ops = pocsag.DeviceOps({})
        audio = self.audio()
        ops.lap("front_end")
        self.__pages, self.__info, self.__cand, self.__batches = pocsag.decode(audio, self.__rate, self.__bauds, ops=ops, **self.__opts)
        self.timings = ops.finish("candidates", "batches", "host")
        for p in self.__pages:
            logging.info("%s (at %.4f s, %d bits repaired)", pocsag.line(p), p["t"], p["corrected"])
        self.__done = True


def decode_host(raw, fs, offset, bw=None, bauds=pocsag.BAUDS, cut=None, slack=2, fix=2, follow=2, content="auto"):
    """(pages, frameInfo) of a uint8[N, 2] recording by the NumPy restatement of the front end (pocsag.audio_host, float64) and of
    both kernels"""
    audio, rate = pocsag.audio_host(raw, fs, float(offset), 48000 if bw is None else bw, pocsag.CUT if cut is None else cut)
    return decode_audio_host(audio, rate, bauds, slack, fix, follow, content)


def decode_audio_host(audio, rate, bauds=pocsag.BAUDS, slack=2, fix=2, follow=2, content="auto"):
    """(pages, frameInfo) of FM-demodulated audio by the restatement of both kernels"""
    found, info, _, _ = pocsag.decode(np.ascontiguousarray(audio, dtype=np.float64).ravel(), rate, bauds, slack, fix, follow, content)
    return found, info
