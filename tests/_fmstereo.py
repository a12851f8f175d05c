"""What the two FM stereo test files share: the multiplexes and the recording of the tone tests, a tone's amplitude in a channel, the
separation of a decoded pair and the full-scale case of the mixer and the filter."""
import functools

import numpy as np

from directdemod_amd import fmstereo as F

TONE_LEVEL = 0.8                                                      # of full programme level, in one channel
FS, CHANNEL = 1200000, 0.0                                            # the end-to-end recording: 1.2 MS/s, the station at the centre
SECONDS = 0.2
EDGE = 0.02                                                           # seconds left out at either end of a measurement


@functools.lru_cache(maxsize=None)
def tone_multiplex(rate, freq, clock_ppm=0.0, channel=0, seconds=0.15, pilot=0.09):
    """radians per sample: a tone of 0.8 in the left (channel 0) or the right channel only, the other silent"""
    n = int(seconds * rate)
    t = F.tone(freq, TONE_LEVEL, n, rate, clock_ppm)
    z = np.zeros(n)
    x = F.encode_mpx(t, z, rate, clock_ppm=clock_ppm, pilot=pilot) if channel == 0 else F.encode_mpx(z, t, rate, clock_ppm=clock_ppm, pilot=pilot)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tone_recording(fs=FS, offset=CHANNEL, freq=1000.0, seconds=SECONDS):
    """u8 IQ: the left-only tone of 0.8 as a station `offset` Hz from the centre, noise of sigma 1 per rail"""
    n = int(seconds * fs)
    raw = F.encode(F.tone(freq, TONE_LEVEL, n, fs), np.zeros(n), fs, offset=offset, amplitude=60.0, sigma=1.0, seed=3)
    raw.setflags(write=False)
    return raw


def amplitude(x, freq, rate):
    """the amplitude of the tone at `freq` Hz in x, by a Hann-weighted projection"""
    x = np.asarray(x, dtype=np.float64)
    w = np.hanning(len(x))
    return 2.0 * abs(np.sum(x * w * np.exp(-2j * np.pi * freq * np.arange(len(x)) / rate))) / w.sum()


def levels(out, freq, rate, edge=EDGE):
    """(left, right): the tone's amplitude in either channel of an int32[n, 2] output at `rate`, in getAudio's unit only when the
    caller scales it; the first and last `edge` seconds are left out (the filter's run-in, the carrier's clipped sums)"""
    k = int(edge * rate)
    o = np.asarray(out, dtype=np.float64)[k:len(out) - k]
    return amplitude(o[:, 0], freq, rate), amplitude(o[:, 1], freq, rate)


def separation_db(out, freq, rate, channel=0):
    """dB by which the tone in `channel` stands above its image in the other"""
    a = levels(out, freq, rate)
    return 20.0 * np.log10(a[channel] / max(a[1 - channel], 1e-12))


def full_scale(rate, deemphasis, o, n, channel=0, g=1.5):
    """(mpx, u, G): every sample at +-pi (q = +-2^15) with the sign of its tap times its mixer factor for output `o` of `channel`,
    u = (0, 2^14) in every block, so that c is the table's real part and the factor 2^14 +- c2 spans -2 * 2^14 .. 4 * 2^14 at g = 1.5:
    the largest |a|, |b| and the largest sum the chain can make"""
    D, _, step38 = F.params(rate)
    h, d0 = F.taps(rate, deemphasis)
    nb = n // F.B
    u = np.tile(np.array([[0, 1 << F.Q]], np.int64), (nb, 1))
    G = F.gain_word(g)
    probe = F.mix_host(np.full(n, np.pi), step38, u, G)[:, channel]            # q = 2^15 everywhere: the factor's sign
    i = o * D + d0 - np.arange(n)
    tap = np.where((i >= 0) & (i < len(h)), h[np.clip(i, 0, len(h) - 1)], 0)
    sign = np.where(tap * probe >= 0, 1.0, -1.0)
    return sign * np.pi, u, G
