"""
G3RUH 9600 baud FSK decoding (beyond the reference): the modem of most amateur and cubesat packet
downlinks besides APRS, carrying the AX.25 frames decode_afsk1200 checks.

Every stage runs on the device and hands device arrays to the next: decode_afsk1200's front end (the fused offsetFreq ->
blackmanHarris(151) -> bwLim chain per chunk, demod_fm over the whole signal), the bit-timing walk (fsk.walk), the hard decision,
descrambler and NRZI (fsk.bit_stream) and the AFSK1200 frame check (afsk.frames).  Only counts, flag positions and the accepted
frames' bytes come down, and what a getter is asked for.

The format is taken from public descriptions of the G3RUH modem; the limits are listed in INTEGRATION.md.
"""
import logging
import time

import numpy as np

from . import _hip, afsk, comm, decode_afsk1200 as _afsk1200, fsk


class decode_fsk9600:
    """Object to decode 9600 baud FSK: decode_fsk9600(sigsrc, offset, bw, baud) with bw None -> 5 * baud.  The audio rate is
    fs / int(fs / bw), and it must give 2 to 64 samples per symbol (ValueError otherwise).
    use_device_raw: read the recording as raw u8 pairs resident on the device when the source offers it (source.read_device_raw)."""

    def __init__(self, sigsrc, offset, bw=None, baud=fsk.BAUDRATE, use_device_raw=True):
        self.__baud = baud
        self.__bw = 5 * baud if bw is None else bw
        self.__front = None
        self.__audio = None
        if sigsrc is not None:
            fs = sigsrc.sampFreq
            if self.__bw <= 0 or fs < self.__bw:
                raise ValueError("decode_fsk9600: a bandwidth of %r S/s cannot be cut from %r S/s" % (self.__bw, fs))
            self.__rate = fs / int(fs / self.__bw)
            fsk.params(self.__rate, baud)              # ValueError unless it gives 2 to 64 samples per symbol
            self.__front = _afsk1200.decode_afsk1200(sigsrc, offset, self.__bw, use_device_raw)
        self.__done = False
        self.__useful = 0
        self.__frames = []
        self.__sym = self.__sidx = self.__bs = None
        self.__info = {}
        self.timings = {}                  # seconds per stage of the last decode (front end, walk, bits, frames)

    @classmethod
    def fromAudio(cls, audio, rate, baud=fsk.BAUDRATE):
        """The decoder over FM-demodulated audio (NumPy or float64 device array) at `rate` S/s, such as a receiver's WAV: no
        front end."""
        fsk.params(rate, baud)
        obj = cls(None, 0, None, baud)
        obj.__rate = rate
        obj.__audio = audio if isinstance(audio, _hip.DevArray) else np.ascontiguousarray(audio, dtype=np.float64).ravel()
        return obj

    @property
    def useful(self):
        """1 if at least one frame with a correct CRC was found, else 0"""
        return self.__useful

    @property
    def audioRate(self):
        """samples per second of the audio the walk reads"""
        return self.__rate

    @property
    def getFrames(self):
        """The accepted frames in stream order, one dict each, as decode_afsk1200.getFrames gives them: flag (index of its start
        flag), start (bit of that flag), nbytes, destination, source, path, control, pid, info and raw"""
        self._decode()
        return list(self.__frames)

    @property
    def getSymbols(self):
        """(sym float64, sidx int64): per symbol the eye sample and the audio sample it was read at"""
        self._decode()
        return self.__sym.to_host(), self.__sidx.to_host()

    @property
    def getBits(self):
        """the descrambled, NRZI-decoded bits, int8, one per symbol"""
        self._decode()
        return self.__bs.bits.to_host()

    @property
    def bitInfo(self):
        """dict: symbols, flags, pairs (consecutive flag pairs checked), frames (accepted) and period, the mean samples per symbol
        (sidx[-1] - sidx[0]) / (symbols - 1) (None below two symbols)"""
        self._decode()
        return dict(self.__info)

    # ------------------------------------------------------------------ the device pipeline
    def audio(self):
        """the FM-demodulated audio as a float64 device array (the front end runs once)"""
        if not isinstance(self.__audio, _hip.DevArray):
            _hip.require_gpu()
            if self.__audio is not None:
                self.__audio = _hip.DevArray.from_host(self.__audio)
            else:
                self.__audio = comm._convert(self.__front._audio().device_signal, np.float64)
        if self.__audio.dtype != np.dtype(np.float64):
            raise TypeError("float64 audio expected, got %s" % self.__audio.dtype)
        return self.__audio

    def _decode(self):
        if self.__done:
            return
        _hip.require_gpu()
        t = {}
        t0 = time.perf_counter()

        def lap(name):
            nonlocal t0
            _hip.sync()
            now = time.perf_counter()
            t[name] = now - t0
            t0 = now
        audio = self.audio()
        lap("front_end")
        sym, sidx, _, _ = fsk.walk(audio, self.__rate, self.__baud)
        lap("walk")
        bs = fsk.bit_stream(sym)
        lap("bits")
        info, raws = afsk.frames(bs)
        flags = bs.flags.to_host() if len(raws) else None
        lap("frames")
        self.timings = t
        frames = []
        acc = np.nonzero(info[:, 1] == 1)[0] if len(info) else []
        for f, raw in zip(acc, raws):
            dst, src, path, control, pid, text = _afsk1200._fields(raw)
            rec = {"flag": int(f), "start": int(flags[f]), "nbytes": int(info[f, 0]) // 8, "destination": dst, "source": src,
                   "path": path, "control": control, "pid": pid, "info": text, "raw": raw}
            logging.info("FSK9600 frame #%d at bit %d, %d bytes: %s > %s %s: %s", rec["flag"], rec["start"], rec["nbytes"],
                         src, dst, path, text)
            frames.append(rec)
        period = None
        if sym.n >= 2:
            ends = (int(sidx.view(0, 1).to_host()[0]), int(sidx.view(sym.n - 1, 1).to_host()[0]))
            period = (ends[1] - ends[0]) / (sym.n - 1)
        self.__info = {"symbols": sym.n, "flags": bs.flags.n, "pairs": len(info), "frames": len(frames), "period": period}
        self.__sym, self.__sidx, self.__bs = sym, sidx, bs
        self.__frames = frames
        self.__useful = 1 if frames else 0
        self.__done = True
