"""What the two ADS-B test files share: the published frames with their published decodes, and builders of crafted recordings."""
import numpy as np

from directdemod_amd import adsb

# real frames with widely published decodes; the remainder of each by 0x1FFF409 is 0
F_CALLSIGN = "8D4840D6202CC371C32CE0576098"        # ICAO 4840D6, TC 4, KLM1023_
F_EVEN = "8D40621D58C382D690C8AC2863A7"            # even position, 38 000 ft
F_ODD = "8D40621D58C386435CC412692AD6"             # odd position
F_VELOCITY = "8D485020994409940838175B284F"        # TC 19 subtype 1: 159.20 kt, 182.88 degrees, -832 ft/min
F_AIRSPEED = "8DA05F219B06B6AF189400CBC33F"        # TC 19 subtype 3
F_EVEN2 = "8D40058B58C901375147EFD09357"
F_ODD2 = "8D40058B58C904A87F402D3B8C59"
F_DF11 = "5D4840D6F8740F"                          # DF 11, 56 bits
FRAMES = [F_CALLSIGN, F_EVEN, F_ODD, F_VELOCITY, F_AIRSPEED, F_EVEN2, F_ODD2, F_DF11]


def flip(frame, *positions):
    """the frame with the bits at `positions` (0 = the first bit sent) inverted, as bytes"""
    b = adsb.bits_of(frame).copy()
    for p in positions:
        b[p] ^= 1
    return np.packbits(b).tobytes()


def double_errors(count=20, seed=11):
    """seeded pairs of distinct bit positions of a 112-bit frame"""
    rng = np.random.default_rng(seed)
    return [tuple(int(v) for v in rng.choice(112, 2, replace=False)) for _ in range(count)]


def slots(frames, rate, Q, frac=0.0, sigma=0.0, seed=0, amplitude=40.0):
    """(recording, candidate numbers): the frames one after another, each `frac` past a whole sample; the candidate of frame i is
    the one at its whole sample"""
    step = adsb.reach(rate) + 24
    at = 8 + step * np.arange(len(frames))
    raw = adsb.encode(frames, rate, at + frac, amplitude, sigma, seed, n=int(at[-1]) + step)
    return raw, at * Q


def comb(rate, n, sigma=3.0, seed=0, amplitude=40.0):
    """a recording of n samples that repeats the preamble's four pulses every 16 chips: candidates pass all along it, so that
    survivors fall on both sides of every tile edge"""
    spc = rate / float(adsb.U)
    c = np.arange(0, int(n / spc) + 16, 16).reshape(-1, 1) + np.array(adsb.PULSES).reshape(1, -1)
    a = c.reshape(-1, 1) * spc
    j = np.arange(n, dtype=np.float64).reshape(1, -1)
    cover = (np.clip(j + 1.0 - a, 0.0, spc) - np.clip(j - a, 0.0, spc)).sum(axis=0)
    rng = np.random.default_rng(seed)
    v = np.stack((amplitude * cover, np.zeros(n)), axis=1) + rng.normal(0.0, 1.0, (n, 2)) * sigma + 127.5
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def recording_with_count(rate, Q, want):
    """the length n at which the recording has exactly `want` candidates, or None"""
    n = adsb.reach(rate) + want // Q
    for m in (n - 1, n, n + 1):
        if adsb.n_candidates(m, rate, Q) == want:
            return m
    return None


# ---- recordings at 4 MS/s, Q = 1, whose chip energies are chosen numbers: a chip is two whole samples, its energy the sum of four
# odd squares (one per rail), so every E = 4 (mod 8) from 4 to 52 can be set, and 6 E[q] = E0 + E2 + E7 + E9 has solutions
CRAFT_RATE = 4000000
BASE = {0: 36, 2: 44, 7: 28, 9: 12}                # the four pulses; every other chip 4; S = 120 = 6 * 20


def _rails(e):
    """four rail values whose (2 v - 255)^2 sum to e, nines first so that a step of 8 down is one rail"""
    m = (e - 4) // 8
    assert e % 8 == 4 and 0 <= m <= 6
    sq = [25] + [9] * (m - 3) + [1] * (6 - m) if m > 4 else [9] * m + [1] * (4 - m)
    assert sum(sq) == e and len(sq) == 4
    return [128 + (int(np.sqrt(s)) - 1) // 2 for s in sq]


def craft(energies):
    """a recording whose candidate 0 has the given preamble energies {chip: E}, every other chip 4"""
    raw = np.full((adsb.reach(CRAFT_RATE) + 8, 2), 128, dtype=np.uint8)
    for c, e in energies.items():
        raw[2 * c:2 * c + 2] = np.array(_rails(e), dtype=np.uint8).reshape(2, 2)
    return raw


def nudged(raw, chip):
    """the recording with one rail of one sample of the chip a step nearer to mid-scale: the chip's energy goes down by 8"""
    out = raw.copy()
    part = out[2 * chip:2 * chip + 2].reshape(-1)                     # (a view: four rails)
    part[np.flatnonzero(part == 129)[0]] = 128
    return out


# one case per inequality: (the energies that make it an equality while the other twelve hold, the chip to nudge down by 8)
EQUALITIES = [
    ("E0>E1", {**BASE, **{1: 36}}, 1), ("E2>E1", {**BASE, **{0: 52, 1: 44}}, 1), ("E2>E3", {**BASE, **{3: 44}}, 3),
    ("E7>E6", {**BASE, **{6: 28}}, 6), ("E7>E8", {**BASE, **{8: 28, 9: 36}}, 8), ("E9>E8", {**BASE, **{8: 12}}, 8),
    ("E9>E10", {**BASE, **{10: 12}}, 10),
] + [("6E%d<S" % q, {**BASE, **{q: 20}}, q) for q in adsb.QUIET]


def comparisons(E):
    """the thirteen left - right differences over a vector of at least 15 energies: each must be positive"""
    s = E[0] + E[2] + E[7] + E[9]
    return [E[0] - E[1], E[2] - E[1], E[2] - E[3], E[7] - E[6], E[7] - E[8], E[9] - E[8], E[9] - E[10]] + [s - 6 * E[q] for q in adsb.QUIET]
