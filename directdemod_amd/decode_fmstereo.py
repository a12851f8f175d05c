"""
FM stereo audio of a broadcast FM station (beyond the reference): decode_rds's front end (decode_afsk1200's
fused offsetFreq -> blackmanHarris -> bwLim chain per chunk at 240 kS/s with rds.window_taps' short window, demod_fm over the whole
signal, the multiplex kept as float64 on the device); then the 19 kHz pilot is correlated in blocks of 256 samples
(fmstereo.pilot), the 38 kHz correction is formed per block (fmstereo.carrier) and every sample is mixed and run through one
decimating FIR per channel, the low-pass and the de-emphasis in one set of taps (fmstereo.audio).  Left and right come down as int32
pairs at about 48 kS/s.

The same multiplex carries RDS: ``decode_rds.fromAudio(obj.multiplex(), obj.multiplexRate)`` decodes it without a second front-end
pass.  There is no noise-dependent blend and no SCA; met in synthesised recordings only (INTEGRATION.md lists the limits).
"""
import numpy as np

from . import _hip, comm, decode_afsk1200 as _afsk1200, demod_fm, fmstereo, rds

BW = 240000


def _gain(diffGain, fs, rate):
    """the difference channel's gain: as given, else the front end's analytic one for a recording and 1 for a bare multiplex"""
    if diffGain is not None:
        return float(diffGain)
    g = 1.0 if fs is None else fmstereo.diff_gain(fs, rate)
    if not fmstereo.GAIN_MIN <= g <= fmstereo.GAIN_MAX:
        raise ValueError("decode_fmstereo: the front end's difference gain %r at %r S/s is not supported; give diffGain" % (g, fs))
    return g


class decode_fmstereo:
    """Object to decode FM stereo audio: decode_fmstereo(sigsrc, offset, bw, deemphasis, pilotMin, diffGain, use_device_raw).
    offset: the station's frequency offset with decode_afsk1200's sign.  bw None -> 240 000; the multiplex rate R = fs / int(fs / bw)
    must lie in 125 000 .. 500 000 (ValueError otherwise).  deemphasis: 50e-6, 75e-6 or None.  pilotMin: the pilot level, as a
    fraction of the 75 kHz peak deviation, from which a block of 256 samples is decoded as stereo.  diffGain: the gain of L - R against
    L + R; None -> fmstereo.diff_gain, which makes up for what the front end's window and the discriminator take from the 38 kHz
    band.  use_device_raw: read the recording as raw u8 pairs resident on the device when the source offers it."""

    def __init__(self, sigsrc, offset, bw=None, deemphasis=50e-6, pilotMin=0.03, diffGain=None, use_device_raw=True):
        self.__bw = BW if bw is None else bw
        self.__opts = {"deemphasis": deemphasis, "pilotMin": pilotMin}
        self.__front = None
        self.__mpx = None
        self.__gain = None
        try:
            fmstereo.check_options(deemphasis, pilotMin, diffGain)
        except ValueError as e:
            raise ValueError(str(e).replace("fmstereo:", "decode_fmstereo:", 1)) from None
        if sigsrc is not None:
            fs = sigsrc.sampFreq
            if self.__bw <= 0 or fs < self.__bw:
                raise ValueError("decode_fmstereo: a bandwidth of %r S/s cannot be cut from %r S/s" % (self.__bw, fs))
            self.__rate = fs / int(fs / self.__bw)
            self.__params(self.__rate)
            self.__gain = _gain(diffGain, fs, self.__rate)
            self.__taps = rds.window_taps(fs)
            self.__front = _afsk1200.decode_afsk1200(sigsrc, float(offset), self.__bw, use_device_raw)
        self.__done = False
        self.__out = np.zeros((0, 2), np.int32)
        self.__info = {}
        self.__lock = np.zeros(0, np.uint8)
        self.timings = {}                  # seconds per stage of the last decode (front_end, pilot, carrier, audio, download, host)

    @staticmethod
    def __params(rate):
        try:
            return fmstereo.params(rate)
        except ValueError as e:
            raise ValueError(str(e).replace("fmstereo:", "decode_fmstereo:", 1)) from None

    @classmethod
    def fromAudio(cls, mpx, rate, deemphasis=50e-6, pilotMin=0.03, diffGain=None):
        """The decoder over the multiplex, the FM discriminator's output (NumPy or float64 device array, radians per sample) at `rate`
        S/s: no front end, and a difference gain of 1 unless diffGain says otherwise."""
        cls.__params(rate)
        obj = cls(None, 0.0, None, deemphasis, pilotMin, diffGain)
        obj.__rate = rate
        obj.__gain = _gain(diffGain, None, rate)
        obj.__mpx = mpx if isinstance(mpx, _hip.DevArray) else np.ascontiguousarray(mpx, dtype=np.float64).ravel()
        return obj

    @property
    def multiplexRate(self):
        """samples per second of the multiplex the kernels read"""
        return self.__rate

    @property
    def audioRate(self):
        """samples per second of the audio: multiplexRate / max(1, rint(multiplexRate / 48000))"""
        return self.__rate / fmstereo.params(self.__rate)[0]

    @property
    def diffGain(self):
        """the gain of the difference channel in use"""
        return self.__gain

    @property
    def getSamples(self):
        """int32[n, 2]: left and right as the kernels give them; getAudio is this times fmstereo.audio_scale(multiplexRate)"""
        self._decode()
        return self.__out.copy()

    @property
    def getAudio(self):
        """float32[n, 2]: left and right; +-1 is the peak deviation at full programme level (the int32 output times
        multiplexRate / (2 * 75000 * 2^21))"""
        self._decode()
        return fmstereo.to_float(self.__out, self.__rate)

    @property
    def getPCM(self):
        """int16[n, 2]: rint(32767 getAudio), clipped"""
        self._decode()
        return fmstereo.to_pcm(self.__out, self.__rate)

    @property
    def getStereo(self):
        """an object with sampRate and signal = getPCM: sink.wavFile(name, obj.getStereo).write writes a two-channel WAV"""
        return fmstereo.StereoSignal(self.audioRate, self.getPCM)

    def __channel(self, x):
        return comm.commSignal(int(round(self.audioRate)), np.ascontiguousarray(x, dtype=np.float64))

    @property
    def getLeft(self):
        """the left channel of getAudio as a commSignal at audioRate"""
        return self.__channel(self.getAudio[:, 0])

    @property
    def getRight(self):
        """the right channel of getAudio as a commSignal at audioRate"""
        return self.__channel(self.getAudio[:, 1])

    @property
    def getMono(self):
        """(left + right) / 2 as a commSignal at audioRate"""
        a = self.getAudio.astype(np.float64)
        return self.__channel(0.5 * (a[:, 0] + a[:, 1]))

    @property
    def stereo(self):
        """1 if more than half of the blocks are locked to a pilot, else 0"""
        self._decode()
        return fmstereo.is_stereo(self.__info)

    @property
    def useful(self):
        """1 if audio came out, else 0"""
        self._decode()
        return 1 if len(self.__out) else 0

    @property
    def pilotInfo(self):
        """blocks (of 256 multiplex samples), locked, level (the pilot's, as a fraction of the peak deviation), freqError (Hz: the
        pilot against 19 kHz by the receiver's clock)"""
        self._decode()
        return dict(self.__info)

    @property
    def lockInfo(self):
        """uint8 per block: 1 where it was decoded as stereo"""
        self._decode()
        return self.__lock.copy()

    # ------------------------------------------------------------------ the device pipeline
    def multiplex(self):
        """the multiplex as a float64 device array (the front end runs once)"""
        _hip.require_gpu()
        if self.__mpx is None:
            sig = self.__front._baseband(self.__taps)
            sig.funcApply(demod_fm.demod_fm().demod)
            self.__mpx = comm._convert(sig.device_signal, np.float64)
        if not isinstance(self.__mpx, _hip.DevArray):
            self.__mpx = _hip.DevArray.from_host(self.__mpx)
        if self.__mpx.dtype != np.dtype(np.float64):
            raise TypeError("a float64 multiplex expected, got %s" % self.__mpx.dtype)
        return self.__mpx

    def _decode(self):
        if self.__done:
            return
        _hip.require_gpu()
        ops = fmstereo.DeviceOps({})
        mpx = self.multiplex()
        ops.lap("front_end")
        self.__out, self.__info, self.__lock = fmstereo.decode(mpx, self.__rate, gain=self.__gain, ops=ops, **self.__opts)
        self.timings = ops.finish("pilot", "carrier", "audio", "download", "host")
        self.__done = True


def decode_host(raw, fs, offset, bw=None, deemphasis=50e-6, pilotMin=0.03, diffGain=None):
    """(int32[n, 2], pilotInfo, lock) of a uint8[N, 2] recording by the NumPy restatement of the front end (rds.audio_host, float64)
    and of the kernels"""
    mpx, rate = rds.audio_host(raw, fs, float(offset), BW if bw is None else bw)
    fmstereo.check_options(deemphasis, pilotMin, diffGain)
    return decode_audio_host(mpx, rate, deemphasis, pilotMin, _gain(diffGain, fs, rate))


def decode_audio_host(mpx, rate, deemphasis=50e-6, pilotMin=0.03, diffGain=None):
    """(int32[n, 2], pilotInfo, lock) of the multiplex by the restatement of the kernels; a difference gain of 1 unless given"""
    fmstereo.check_options(deemphasis, pilotMin, diffGain)
    return fmstereo.decode(np.ascontiguousarray(mpx, dtype=np.float64).ravel(), rate, deemphasis, pilotMin, _gain(diffGain, None, rate))
