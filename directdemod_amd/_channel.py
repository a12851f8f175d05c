"""
The narrowband channel front end of decode_ais, decode_pocsag, decode_rs41 and decode_acars: per channel decode_afsk1200's fused
offsetFreq -> blackmanHarris -> bwLim chain per chunk with a window that fits the recording's rate (ais.window_taps), a channel
low-pass at the audio rate (filters.lowpass) and a detector over the whole signal: the FM discriminator (fm_audio) or, for ACARS,
the magnitude.  The audio the burst kernels read is float64 on the device (on_device).
"""
import numpy as np

from . import _hip, ais, comm, decode_afsk1200 as _afsk1200, demod_fm, filters

_F64 = np.dtype(np.float64)


class Channels:
    """The channels at `offsets` (decode_afsk1200's sign) of the recording `sigsrc`, each cut to `bw` S/s and low-passed at `cut`
    Hz.  ValueError, in `who`'s name, unless bw can be cut from the recording and cut fits the audio rate; check_rate(rate), called
    between the two, raises the decoder's own for an audio rate it does not serve.  rate: the audio rate, fs / int(fs / bw)."""

    def __init__(self, who, sigsrc, offsets, bw, cut, use_device_raw, check_rate=None):
        fs = sigsrc.sampFreq
        if bw <= 0 or fs < bw:
            raise ValueError("%s: a bandwidth of %r S/s cannot be cut from %r S/s" % (who, bw, fs))
        self.rate = fs / int(fs / bw)
        if check_rate is not None:
            check_rate(self.rate)
        if not 0 < cut < self.rate / 2.0:
            raise ValueError("%s: a cut-off of %r Hz does not fit an audio rate of %r S/s" % (who, cut, self.rate))
        self._cut = cut
        self._taps = ais.window_taps(fs)
        self._fronts = [_afsk1200.decode_afsk1200(sigsrc, float(o), bw, use_device_raw) for o in offsets]

    def audios(self, detect):
        """one float64 device array per channel: detect(the channel's filtered commSignal)"""
        out = []
        for front in self._fronts:
            sig = front._baseband(self._taps)
            sig.filter(filters.lowpass(self.rate, self._cut, storeState=False))
            out.append(detect(sig))
        return out


def fm_audio(sig):
    """the FM discriminator's output in radians per sample, float64"""
    sig.funcApply(demod_fm.demod_fm().demod)
    return comm._convert(sig.device_signal, np.float64)


def on_device(audios):
    """the audios as float64 device arrays: host arrays are uploaded; TypeError for another type"""
    out = [a if isinstance(a, _hip.DevArray) else _hip.DevArray.from_host(a) for a in audios]
    for a in out:
        if a.dtype != _F64:
            raise TypeError("float64 audio expected, got %s" % a.dtype)
    return out
