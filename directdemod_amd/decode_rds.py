"""
RDS decoding of a broadcast FM station (beyond the reference): decode_afsk1200's front end with a shorter
window (the fused offsetFreq -> blackmanHarris -> bwLim chain per chunk at 240 kS/s, demod_fm over the whole signal, no low-pass in
between: the multiplex up to 60 kHz is wanted); then the 57 kHz subcarrier is mixed down with a table phasor and block-summed on the
device (rds.baseband), every baseband sample is tested as the start of a group (rds.candidates: 104 differential bit decisions from an
LDS prefix sum, four block remainders), the survivors are decoded one wave each (rds.groups: burst repair of up to `fix` bits), and
only that short list comes down.  The groups are merged, chained, followed and parsed on the host (rds.decode).

No carrier and no bit clock is recovered: every group is found on its own, so a recording that starts inside a group is decoded from
the next one on.  The format is IEC 62106 / EN 50067 as publicly described and has been met in synthesised recordings only;
INTEGRATION.md lists the limits.
"""
import logging

import numpy as np

from . import _hip, comm, decode_afsk1200 as _afsk1200, demod_fm, rds

_KEYS = ("t", "start", "pi", "group", "tp", "pty", "words", "repaired", "followed")
BW = 240000


def _public(g):
    out = {k: g[k] for k in _KEYS}
    out["words"] = list(g["words"])
    return out


class decode_rds:
    """Object to decode RDS: decode_rds(sigsrc, offset, bw, clean, fix, follow, use_device_raw).  offset: the station's frequency
    offset with decode_afsk1200's sign.  bw None -> 240 000; the multiplex rate R = fs / int(fs / bw) must lie in 125 000 ..
    500 000 and give 12 to 32 baseband samples per bit (ValueError otherwise).  clean: the clean blocks of four a start needs to
    be listed (2 .. 4).  fix: the longest burst repaired in a block (0 .. 5).  follow: groups taken in a row at their predicted
    start, 104 bits after the group before, where the block test listed nothing.  use_device_raw: read the recording as raw u8 pairs
    resident on the device when the source offers it (source.read_device_raw)."""

    def __init__(self, sigsrc, offset, bw=None, clean=3, fix=2, follow=2, use_device_raw=True):
        self.__bw = BW if bw is None else bw
        self.__opts = {"clean": clean, "fix": fix, "follow": follow}
        self.__front = None
        self.__audio = None
        rds.check_options(clean, fix, follow)
        if sigsrc is not None:
            fs = sigsrc.sampFreq
            if self.__bw <= 0 or fs < self.__bw:
                raise ValueError("decode_rds: a bandwidth of %r S/s cannot be cut from %r S/s" % (self.__bw, fs))
            self.__rate = fs / int(fs / self.__bw)
            rds.params(self.__rate)                          # ValueError unless the rate is served
            self.__taps = rds.window_taps(fs)
            self.__front = _afsk1200.decode_afsk1200(sigsrc, float(offset), self.__bw, use_device_raw)
        self.__done = False
        self.__groups = []
        self.__info = {}
        self.__cand = {}
        self.timings = {}                  # seconds per stage of the last decode (front_end, baseband, candidates, groups, host)

    @classmethod
    def fromAudio(cls, mpx, rate, clean=3, fix=2, follow=2):
        """The decoder over the multiplex, the FM discriminator's output (NumPy or float64 device array, radians per sample) at `rate`
        S/s: no front end."""
        rds.params(rate)
        obj = cls(None, 0.0, None, clean, fix, follow)
        obj.__rate = rate
        obj.__audio = mpx if isinstance(mpx, _hip.DevArray) else np.ascontiguousarray(mpx, dtype=np.float64).ravel()
        return obj

    @property
    def audioRate(self):
        """samples per second of the multiplex the kernels read"""
        return self.__rate

    @property
    def useful(self):
        """1 if at least one group was decoded, else 0"""
        self._decode()
        return 1 if self.__groups else 0

    @property
    def getGroups(self):
        """one dict per group in time order: t (seconds), start (the baseband sample of the group's first bit boundary), pi, group
        ("0A" .. "15B"), tp, pty, words (four, None where a block was not decoded), repaired (bits), followed; pi, group, tp and pty
        are None where their block is missing"""
        self._decode()
        return [_public(g) for g in self.__groups]

    @property
    def getStations(self):
        """per PI: ps (eight characters, undecoded places as spaces), ps_complete, radiotext, pty, tp, ta, ms, di, af (MHz, method A),
        af_count, clock ((ISO UTC, local offset in half hours) of the last 4A group, or None), groups (a count per group type)"""
        self._decode()
        return rds.stations(self.__groups)

    @property
    def getText(self):
        """one line per station: RDS D318 PS: 'RADIO 1 ' RT: '...'"""
        self._decode()
        return rds.text_lines(self.__groups)

    @property
    def frameInfo(self):
        """samples (of the baseband), candidates (that passed the block test), duplicates (candidates merged into another of their
        group), dropped (kept candidates neither chained nor clean in all four blocks), followed, groups, repaired (groups with a
        repaired block)"""
        self._decode()
        return dict(self.__info)

    @property
    def candidateInfo(self):
        """every candidate that passed the block test, kept or not: a dict of arrays t, words, status, third, metric, state, good"""
        self._decode()
        return {key: v.copy() for key, v in self.__cand.items()}

    # ------------------------------------------------------------------ the device pipeline
    def audio(self):
        """the multiplex as a float64 device array (the front end runs once)"""
        _hip.require_gpu()
        if self.__audio is None:
            sig = self.__front._baseband(self.__taps)
            sig.funcApply(demod_fm.demod_fm().demod)
            self.__audio = comm._convert(sig.device_signal, np.float64)
        if not isinstance(self.__audio, _hip.DevArray):
            self.__audio = _hip.DevArray.from_host(self.__audio)
        if self.__audio.dtype != np.dtype(np.float64):
            raise TypeError("a float64 multiplex expected, got %s" % self.__audio.dtype)
        return self.__audio

    def _decode(self):
        if self.__done:
            return
        _hip.require_gpu()
        ops = rds.DeviceOps({})
        mpx = self.audio()
        ops.lap("front_end")
        self.__groups, self.__info, self.__cand = rds.decode(mpx, self.__rate, ops=ops, **self.__opts)
        self.timings = ops.finish("baseband", "candidates", "groups", "host")
        for line in rds.text_lines(self.__groups):
            logging.info("%s", line)
        self.__done = True


def decode_host(raw, fs, offset, bw=None, clean=3, fix=2, follow=2):
    """(groups, frameInfo) of a uint8[N, 2] recording by the NumPy restatement of the front end (rds.audio_host, float64) and of
    the kernels"""
    mpx, rate = rds.audio_host(raw, fs, float(offset), BW if bw is None else bw)
    return decode_audio_host(mpx, rate, clean, fix, follow)


def decode_audio_host(mpx, rate, clean=3, fix=2, follow=2):
    """(groups, frameInfo) of the multiplex by the restatement of the kernels; the groups as getGroups gives them"""
    found, info, _ = rds.decode(np.ascontiguousarray(mpx, dtype=np.float64).ravel(), rate, clean, fix, follow)
    return [_public(g) for g in found], info


def stations_host(groups):
    """getStations of decode_audio_host's groups"""
    return rds.stations(groups)
