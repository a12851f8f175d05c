"""What the two RDS test files share: a station's groups, the multiplex and the recording of the end-to-end tests, and builders of
crafted basebands whose half-bit differences are chosen integers, so that a group decodes at a chosen start without any front end."""
import functools

import numpy as np

from directdemod_amd import rds

PI = 0xD318
PS = "RADIO 1 "
TEXT = "Hi RDS\r"                                                     # seven characters: two 2A groups
MJD, HOUR, MINUTE, OFFSET_HALF_HOURS = 60000, 13, 37, 2
CLOCK = ("2023-02-25T13:37:00Z", 2)
AF = ((224 + 3, 10), (20, 205), (30, rds.FILLER), (rds.FILLER, rds.FILLER))     # three frequencies: 88.5, 89.5, 90.5
FS, CHANNEL = 1200000, 150000.0                                       # the recording: 1.2 MS/s, the station 150 kHz above the centre


def station_groups():
    """seven groups: the name's four 0A segments, the text's two 2A segments and one 4A, interleaved"""
    a = [rds.group_0a(PI, PS, s, tp=1, pty=10, ta=0, ms=1, di=0b1001, af=AF[s]) for s in range(4)]
    t = [rds.group_2a(PI, TEXT, s, flag=0, tp=1, pty=10) for s in range(2)]
    c = rds.group_4a(PI, MJD, HOUR, MINUTE, OFFSET_HALF_HOURS, tp=1, pty=10)
    return [a[0], t[0], a[1], c, a[2], t[1], a[3]]


def same_station(st):
    """getStations' entry against what station_groups sends"""
    assert st["ps"] == PS and st["ps_complete"] and st["radiotext"] == "Hi RDS" and st["clock"] == CLOCK
    assert (st["pty"], st["tp"], st["ta"], st["ms"], st["di"]) == (10, 1, 0, 1, 0b1001)
    assert st["af"] == [88.5, 89.5, 90.5] and st["af_count"] == 3 and st["groups"] == {"0A": 4, "2A": 2, "4A": 1}


@functools.lru_cache(maxsize=None)
def multiplex(rate=171000.0, clock_ppm=0.0, phase=0.0):
    """the seven groups as the discriminator gives them, a tone and the pilot beside them, 10 ms of lead"""
    x = rds.encode_mpx(station_groups(), rate, start=0.01, clock_ppm=clock_ppm, phase=phase)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def recording(clock_ppm=0.0, carrier_ppm=0.0):
    """the seven groups as u8 IQ at 1.2 MS/s, about 0.63 s, with noise of sigma 4 per rail"""
    raw = rds.encode(station_groups(), FS, offset=CHANNEL, amplitude=60.0, sigma=4.0, seed=5, start=0.01, clock_ppm=clock_ppm,
                     carrier_ppm=carrier_ppm, carrier=1e6)
    raw.setflags(write=False)
    return raw


# ---------------------------------------------------------------------------------------------------------------- crafted basebands
def levels(bits):
    """the 105 biphase levels (+-1) around the boundaries p_-1 .. p_103 that make the restatement read `bits` (104 of them)"""
    d = np.concatenate(([0], np.cumsum(np.asarray(bits, dtype=np.int64)) & 1))
    return 2 * d - 1


def craft(bits, sps, t, m, amp=(3000, -1700), fill=0):
    """int32[m, 2]: a baseband in which the start t reads `bits`: around each boundary t + k sps, k = -1 .. 103, the samples from the
    boundary on hold +level * amp and those before it -level * amp, out to half a bit either way, so every z[p_k] is level_k times a
    fixed positive multiple of amp and Re(z[p_k] conj(z[p_(k-1)])) has the sign of level_k level_(k-1).  Elsewhere `fill`."""
    lv = levels(bits)
    b = np.full((m, 2), fill, dtype=np.int64)
    i = np.arange(m)
    k = np.rint((i - t) / sps).astype(np.int64)                       # the nearest boundary
    inside = (k >= -1) & (k <= rds.BITS - 1)
    after = i >= np.floor((t + k * sps) + 0.5)
    sign = np.where(after, 1, -1) * lv[np.clip(k + 1, 0, rds.BITS)]
    b[inside] = (sign[inside, None] * np.asarray(amp, dtype=np.int64)[None, :])
    return b.astype(np.int32)


def group_bits(words):
    return rds.air_bits([words])


def room(sps):
    """samples a crafted group takes behind its start, and before it"""
    return int(104 * sps) + 40, int(2 * sps) + 20


def planted(groups, sps, gap=60, amp=(3000, -1700), noise=0, seed=0):
    """(baseband, the starts): the groups (bit arrays) one behind the other, `gap` samples between them, over Gaussian noise"""
    after, before = room(sps)
    starts = [before + k * (after + before + gap) for k in range(len(groups))]
    m = starts[-1] + after + 5
    b = np.zeros((m, 2), dtype=np.int64)
    for bits, t in zip(groups, starts):
        c = craft(bits, sps, t, m, amp)
        b += c
    if noise:
        b += np.rint(np.random.default_rng(seed).normal(0.0, noise, (m, 2))).astype(np.int64)
    return b.astype(np.int32), starts
