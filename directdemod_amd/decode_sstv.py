"""
Slow-scan television image decoding, PD modes (beyond the reference): the pictures the ISS sends as PD120
on 145.800 MHz FM, and the other six modes of the family.

The front end is decode_fm's chunk loop (fm_audio_chunks: offsetFreq -> blackmanHarris(151) -> bwLim(bw) -> demod_fm -> strict
bwLim(audioFreq)), widened to float64; behind it every stage runs on the device (sstv.decode over sstv.DeviceOps): the analytic lag
product, the tone classes, the sync and leader run searches, the pixel sums and the colour conversion.  Only the short position
lists, about a second of tone classes per header and the finished images come down.

The mode figures are taken from public descriptions of the PD modes; nothing here has been checked against a recording or another
decoder (INTEGRATION.md lists the limits).
"""
import logging

import numpy as np

from . import _hip, comm, decode_fm, sstv


class decode_sstv:
    """Object to decode SSTV: decode_sstv(sigsrc, offset, bw, audioFreq, mode) with bw None -> 30000 and audioFreq None -> 24000.
    mode None: every image's mode comes from its VIS header (a header with a parity failure or an unknown code is skipped); a mode
    name forces that mode, tolerates parity failures, and without any header starts the image at the first line sync.
    ValueError when the audio rate is outside sstv.RATE_MIN .. RATE_MAX or gives a forced mode's pixel fewer than two samples.
    use_device_raw: read the recording as raw u8 pairs resident on the device when the source offers it."""

    def __init__(self, sigsrc, offset, bw=None, audioFreq=None, mode=None, use_device_raw=True):
        self.__bw = 30000 if bw is None else bw
        self.__rate = 24000 if audioFreq is None else audioFreq
        self.__mode = sstv.mode_of(mode)
        sstv.check_rate(self.__rate, self.__mode)
        self.__sigsrc = sigsrc
        self.__offset = offset
        self.__use_raw = use_device_raw
        self.__audio = None
        self.__done = False
        self.__images = []
        self.__info = []
        self.timings = {}                  # seconds per stage of the last decode

    @classmethod
    def fromAudio(cls, audio, rate, mode=None):
        """The decoder over FM-demodulated audio (NumPy or float64 device array) at `rate` S/s, such as a receiver's WAV: no
        front end."""
        obj = cls(None, 0, None, rate, mode)
        obj.__audio = audio if isinstance(audio, _hip.DevArray) else np.ascontiguousarray(audio, dtype=np.float64).ravel()
        return obj

    @property
    def useful(self):
        """1 if at least one image was decoded, else 0"""
        self._decode()
        return 1 if self.__images else 0

    @property
    def audioRate(self):
        """samples per second of the audio the chain reads"""
        return self.__rate

    @property
    def getImages(self):
        """uint8[rows, W, 3] RGB arrays, one per image found, in stream order"""
        self._decode()
        return list(self.__images)

    @property
    def getImage(self):
        """the first image, or None"""
        self._decode()
        return self.__images[0] if self.__images else None

    @property
    def imageInfo(self):
        """one dict per image: mode, vis (the header's code; None without a header), parity_ok, start (audio sample of the first
        line sync), rows, syncs_matched, syncs_expected, period (fitted samples per line pair), slant_ppm, empty_pixels"""
        self._decode()
        return [dict(i) for i in self.__info]

    def audio(self):
        """the FM-demodulated audio as a float64 device array (the front end runs once)"""
        if not isinstance(self.__audio, _hip.DevArray):
            _hip.require_gpu()
            if self.__audio is not None:
                self.__audio = _hip.DevArray.from_host(self.__audio)
            else:
                sig = decode_fm.fm_audio_chunks(self.__sigsrc, self.__offset, self.__bw, self.__rate, True,
                                                use_device_raw=self.__use_raw)
                self.__audio = comm._convert(sig.device_signal, np.float64)
        if self.__audio.dtype != np.dtype(np.float64):
            raise TypeError("float64 audio expected, got %s" % self.__audio.dtype)
        return self.__audio

    def _decode(self):
        if self.__done:
            return
        _hip.require_gpu()
        ops = sstv.DeviceOps({})
        audio = self.audio()
        ops.lap("front_end")
        self.__images, self.__info = sstv.decode(audio, self.__rate, self.__mode, ops)
        self.timings = ops.finish()
        for i in self.__info:
            logging.info("SSTV %s image at sample %d: %d rows, %d of %d syncs, slant %.0f ppm, %d empty pixels", i["mode"], i["start"],
                         i["rows"], i["syncs_matched"], i["syncs_expected"], i["slant_ppm"], i["empty_pixels"])
        self.__done = True
