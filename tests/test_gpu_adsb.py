"""The ADS-B kernels on the device (dd_adsb.h through dd_adsb_candidates, dd_adsb_demod and the diagnostic dd_debug_adsb_chips, the
wrappers of directdemod_amd/adsb.py and decode_adsb) against the NumPy restatement in adsb.py.

The chain is all integer, so every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import _adsb as A
from directdemod_amd import adsb, decode_adsb, source

pytestmark = pytest.mark.gpu

SENT = np.int64(-0x5A5A5A5A5A5A5A5B)
SPARE = 16


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def same_det(got, want):
    for key in ("k", "frames", "L", "df", "rem", "fixed", "score"):
        assert np.array_equal(got[key], want[key]), key


def dev_candidates(hip, raw, rate, Q, cap):
    """dd_adsb_candidates with `cap` places and SPARE sentinels behind them -> (rc, count, the places, the sentinels still whole)"""
    iq = adsb.to_device(raw)
    lst = hip.DevArray.from_host(np.full(cap + SPARE, SENT))
    count = C.c_int64(-1)
    rc = hip.lib().dd_adsb_candidates(iq.ptr, iq.n, rate, Q, lst.ptr, cap, C.byref(count), None)
    hip.sync()
    got = lst.to_host()
    return rc, count.value, got[:cap], bool(np.all(got[cap:] == SENT))


# ---------------------------------------------------------------------------------------------------------------- chip energies
GRIDS = [(2000000, 1), (2000000, 2), (2000000, 4), (2400000, 4), (10000000, 1), (20000000, 1), (3000001, 2)]


@pytest.mark.parametrize("rate,Q", GRIDS)
@pytest.mark.parametrize("fill", ["random", 0, 255])
def test_chips_equal_the_restatement(hip, rate, Q, fill):
    n = adsb.reach(rate) + 77
    raw = np.random.default_rng(rate % 1000 + Q).integers(0, 256, (n, 2)).astype(np.uint8) if fill == "random" else np.full((n, 2), fill, np.uint8)
    total = adsb.n_candidates(n, rate, Q)
    ks = np.unique(np.concatenate(([0, 1, total // 2, total - 2, total - 1], np.random.default_rng(3).integers(0, total, 20))))
    got = adsb.chips_device(adsb.to_device(raw), rate, Q, ks)
    want = adsb.chips(adsb.power(raw), rate, Q, ks)
    assert np.array_equal(got, want)
    if fill == 255:                                                  # the largest energy there is: a chip's R / g units of 130 050
        assert got.max() == adsb.grid(rate, Q)[2] * 130050


def test_chips_of_a_k_outside_the_recording_are_zero(hip):
    raw = np.full((400, 2), 200, np.uint8)
    total = adsb.n_candidates(400, 2400000, 4)
    got = adsb.chips_device(adsb.to_device(raw), 2400000, 4, [-1, total, total - 1])
    assert not got[:2].any() and got[2].all()


# ---------------------------------------------------------------------------------------------------------------- candidates
def check_candidates(hip, raw, rate, Q):
    want = adsb.candidates_host(adsb.power(raw), rate, Q)
    rc, count, got, whole = dev_candidates(hip, raw, rate, Q, len(want) + 3)
    assert rc == 0 and count == len(want) and whole
    assert np.array_equal(got[:count], want) and np.all(got[count:] == SENT)
    return want


@pytest.mark.parametrize("rate,Q", [(2400000, 4), (2400000, 1), (3000001, 2), (20000000, 1)])
def test_shortest_recordings(hip, rate, Q):
    full = adsb.reach(rate)                                          # the first length that holds 240 chips
    raw = adsb.encode([A.F_CALLSIGN], rate, [0.0], n=full + 1)
    assert adsb.n_candidates(full - 1, rate, Q) == 0 and adsb.n_candidates(full, rate, Q) >= 1
    rc, count, got, whole = dev_candidates(hip, raw[:full - 1], rate, Q, 4)
    assert (rc, count, whole) == (0, 0, True) and np.all(got == SENT)
    for n in (full, full + 1):
        want = check_candidates(hip, raw[:n], rate, Q)
        assert want[0] == 0                                          # the frame at the very start is found


@pytest.mark.parametrize("rate,Q", [(3000001, 2), (2400000, 4), (2000000, 8)])
@pytest.mark.parametrize("tiles", [255, 256, 257, 1023, 1024, 1025])
def test_candidate_counts_around_tile_edges(hip, rate, Q, tiles):
    n = A.recording_with_count(rate, Q, tiles * Q)
    if n is None:                                                    # this grid's counts are 1 (mod Q): one past the multiple
        n = A.recording_with_count(rate, Q, tiles * Q + 1)
    assert adsb.n_candidates(n, rate, Q) in (tiles * Q, tiles * Q + 1)
    raw = A.comb(rate, n, seed=tiles)
    want = check_candidates(hip, raw, rate, Q)
    assert len(want) >= tiles // 16                                  # survivors all along the recording
    starts = want // Q
    for edge in range(adsb.TILE, int(starts[-1]), adsb.TILE):
        assert np.any(starts < edge) and np.any(starts >= edge)
        assert edge - starts[starts < edge].max() < 40 and starts[starts >= edge].min() - edge < 40


def test_frame_that_ends_on_the_last_sample(hip):
    rate, Q = 2400000, 4
    n = 1000
    raw = adsb.encode([A.F_VELOCITY], rate, [float(n - adsb.reach(rate))], sigma=2.0, seed=4, n=n)
    want = check_candidates(hip, raw, rate, Q)
    last = adsb.n_candidates(n, rate, Q) - 1
    assert last == (n - adsb.reach(rate)) * Q and want[-1] == last
    det = adsb.demod(adsb.to_device(raw), rate, Q, np.array([last]), 1)
    assert bytes(det["frames"][0]).hex().upper() == A.F_VELOCITY and det["rem"][0] == 0


@pytest.mark.parametrize("name,energies,chip", A.EQUALITIES, ids=[e[0] for e in A.EQUALITIES])
def test_each_comparison_is_strict(hip, name, energies, chip):
    tie = A.craft(energies)
    E = adsb.chips(adsb.power(tie), A.CRAFT_RATE, 1, [0])[0]
    assert all(E[c] == energies.get(c, 4) for c in range(16))
    cmp = A.comparisons(E)
    assert sorted(cmp)[0] == 0 and sorted(cmp)[1] > 0                # one equality, twelve hold
    assert np.array_equal(adsb.chips_device(adsb.to_device(tie), A.CRAFT_RATE, 1, [0])[0], E)
    assert 0 not in check_candidates(hip, tie, A.CRAFT_RATE, 1)
    ok = A.nudged(tie, chip)
    assert np.count_nonzero(np.any(ok != tie, axis=1)) == 1          # one sample nudged
    assert min(A.comparisons(adsb.chips(adsb.power(ok), A.CRAFT_RATE, 1, [0])[0])) > 0
    assert 0 in check_candidates(hip, ok, A.CRAFT_RATE, 1)


def test_capacities(hip):
    rate, Q = 2400000, 4
    raw = A.comb(rate, 900, seed=2)
    want = adsb.candidates_host(adsb.power(raw), rate, Q)
    m = len(want)
    assert m >= 20
    for cap in (0, 1, m - 1, m, m + 5):
        rc, count, got, whole = dev_candidates(hip, raw, rate, Q, cap)
        assert count == m and whole
        assert rc == (0 if cap >= m else hip.DD_ERR_INVALID)
        kept = min(cap, m)
        assert np.array_equal(got[:kept], want[:kept]) and np.all(got[kept:] == SENT)
    lst, count = adsb.candidates(adsb.to_device(raw), rate, Q, cap=3)           # the wrapper asks again at the true count
    assert count == m and np.array_equal(lst.view(0, m).to_host(), want)


# ---------------------------------------------------------------------------------------------------------------- demodulation
def check_demod(raw, rate, Q, ks):
    got = adsb.demod(adsb.to_device(raw), rate, Q, np.asarray(ks, dtype=np.int64), len(ks))
    want = adsb.demod_host(adsb.power(raw), rate, Q, ks)
    same_det(got, want)
    return got


def test_single_and_double_bit_errors(hip):
    rate, Q = 2400000, 4
    raw, ks = A.slots([A.flip(A.F_CALLSIGN, p) for p in range(112)], rate, Q, frac=0.25, sigma=1.0, seed=5)
    det = check_demod(raw, rate, Q, ks + 1)                          # (the candidate a quarter sample on)
    assert np.array_equal(det["fixed"][5:], np.arange(5, 112))
    assert np.all(det["fixed"][:5] == -1)
    assert all(bytes(f).hex().upper() == A.F_CALLSIGN for f in det["frames"][5:])
    pairs = A.double_errors()
    raw, ks = A.slots([A.flip(A.F_CALLSIGN, *p) for p in pairs], rate, Q, sigma=1.0, seed=6)
    det = check_demod(raw, rate, Q, ks)
    keeps_df = np.array([min(p) >= 5 for p in pairs])
    assert np.all(det["fixed"][keeps_df] == -1) and np.all(det["rem"] != 0)


def test_short_frames_and_formats_around_16(hip):
    rate, Q = 2400000, 4
    rng = np.random.default_rng(8)
    made = [bytes([df << 3 | 5]) + rng.integers(0, 256, 13).astype(np.uint8).tobytes() for df in (0, 4, 11, 15, 16, 17, 20, 31)]
    raw, ks = A.slots([A.F_DF11] + made, rate, Q, sigma=1.0, seed=9)
    det = check_demod(raw, rate, Q, ks)
    assert det["df"].tolist() == [11, 0, 4, 11, 15, 16, 17, 20, 31]
    assert det["L"].tolist() == [56, 56, 56, 56, 56, 112, 112, 112, 112]
    assert bytes(det["frames"][0]).hex().upper() == A.F_DF11 + "00" * 7 and det["rem"][0] == 0
    assert not det["frames"][:5, 7:].any()
    for i in range(1, 5):                                            # a short frame is the first seven bytes of what was sent
        assert bytes(det["frames"][i][:7]) == made[i - 1][:7]


@pytest.mark.parametrize("rate,Q,fill", [(2400000, 4, 0), (20000000, 1, 255), (2000000, 1, 77)])
def test_equal_energies_read_zero(hip, rate, Q, fill):
    raw = np.full((adsb.reach(rate) + 5, 2), fill, np.uint8)
    det = check_demod(raw, rate, Q, [0, adsb.n_candidates(len(raw), rate, Q) - 1])
    assert not det["frames"].any() and not det["score"].any() and not det["rem"].any() and np.all(det["L"] == 56)


def test_greatest_score(hip):
    """full-scale pulses over silence at 20 MS/s: every bit's difference is a chip of 130 050 less a chip of 2"""
    rate = 20000000
    on = adsb.cover(A.F_AIRSPEED, rate, 3.0, adsb.reach(rate) + 9) > 0.5
    raw = np.where(on.reshape(-1, 1), 255, 128).astype(np.uint8).repeat(2, axis=1)
    det = check_demod(raw, rate, 1, [3])
    assert bytes(det["frames"][0]).hex().upper() == A.F_AIRSPEED
    assert det["score"][0] == 112 * 10 * (130050 - 2)


@pytest.mark.parametrize("m", [1, 65])
def test_list_lengths(hip, m):
    rate, Q = 2400000, 4
    raw, ks = A.slots(A.FRAMES, rate, Q, frac=0.5, sigma=2.0, seed=m)
    total = adsb.n_candidates(len(raw), rate, Q)
    ks = np.concatenate((ks + 2, np.random.default_rng(m).integers(0, total, 65)))[:m]
    det = check_demod(raw, rate, Q, ks)
    assert bytes(det["frames"][0]).hex().upper() == A.F_CALLSIGN
    if m > 8:
        assert bytes(det["frames"][7][:7]).hex().upper() == A.F_DF11


def test_a_listed_k_outside_the_recording(hip):
    raw, ks = A.slots([A.F_EVEN], 2400000, 4)
    total = adsb.n_candidates(len(raw), 2400000, 4)
    det = adsb.demod(adsb.to_device(raw), 2400000, 4, np.array([total, ks[0], -1]), 3)
    assert det["L"].tolist() == [0, 112, 0] and det["fixed"].tolist() == [-1, -1, -1]
    assert not det["frames"][[0, 2]].any() and bytes(det["frames"][1]).hex().upper() == A.F_EVEN


# ---------------------------------------------------------------------------------------------------------------- end to end
RATE = 2400000


@pytest.fixture(scope="module")
def air():
    """about 30 ms at 2.4 MS/s: the eight frames at distinct fractional phases and amplitudes, a pair of which the second starts
    inside the first one's 240 chips (behind the 56 bits of a short frame: two frames that overlap on the air destroy each other's
    bits), and one frame with a flipped bit; with the restatement's answer"""
    rng = np.random.default_rng(21)
    frames = list(A.FRAMES) + [A.F_DF11, A.F_VELOCITY, A.flip(A.F_AIRSPEED, 40)]
    starts = np.concatenate((2000.0 + 6000.0 * np.arange(8) + rng.uniform(0.0, 1.0, 8), [50000.3, 50000.3 + 160.4, 60000.7]))
    amps = np.concatenate((rng.uniform(30.0, 60.0, 8), [35.0, 70.0, 45.0]))
    raw = adsb.encode(frames, RATE, starts, amps, 3.0, seed=22, carrier_offsets=rng.uniform(-50e3, 50e3, 11), n=72000)
    return raw, frames, starts, decode_adsb.decode_host(raw, RATE)


def same_answer(dec, want):
    msgs, info, aircraft = want
    assert dec.getMsgs == msgs
    frames, lengths = dec.getFrames
    assert [bytes(f[:n]) for f, n in zip(frames, lengths)] == [m["raw"] for m in msgs]
    assert dec.frameInfo == info and dec.getAircraft == aircraft
    assert dec.useful == 1


def test_end_to_end(hip, air):
    raw, frames, starts, want = air
    msgs, info, aircraft = want
    dec = decode_adsb.decode_adsb.fromIQ(raw, RATE)
    same_answer(dec, want)
    sent = [adsb.as_bytes(f) for f in frames[:10]] + [adsb.as_bytes(A.F_AIRSPEED)]
    for f, s in zip(sent, starts):                                   # every frame sent is among the messages, where it was sent
        assert any(m["raw"] == f and abs(m["start"] - s) < 1.0 for m in msgs), (f.hex(), s)
    assert info["phases"] == 4 and info["repaired"] == 1 and info["clean"] == 10 and info["samples"] == 72000
    assert [m["fixed"] for m in msgs if m["fixed"] >= 0] == [40]
    assert len(aircraft["40621D"]["track"]) == 1                     # (the odd frame came last: its latitude)
    assert aircraft["40621D"]["track"][0][1] == 52.26578017412606 and aircraft["40621D"]["track"][0][3] == 38000
    assert aircraft["4840D6"]["callsign"] == "KLM1023_"
    cand = dec.candidateInfo
    assert len(cand["k"]) == info["passed"] and set(dec.timings) == {"upload", "candidates", "demod", "host"}
    same_answer(decode_adsb.decode_adsb.fromIQ(adsb.to_device(raw), RATE), want)


def test_end_to_end_from_a_source_and_in_pieces(hip, air):
    raw, frames, starts, want = air
    same_answer(decode_adsb.decode_adsb(source.IQarray(raw, RATE)), want)
    same_answer(decode_adsb.decode_adsb(source.IQarray(raw, RATE), use_device_raw=False), want)
    piece = int(starts[3]) + 100                                     # the fourth frame straddles the first piece's edge
    same_answer(decode_adsb.decode_adsb(source.IQarray(raw, RATE), piece=piece), want)
    same_answer(decode_adsb.decode_adsb.fromIQ(raw, RATE, piece=5000), want)


def test_rate_and_phase_limits(hip):
    raw = np.zeros((10, 2), np.uint8)
    for rate, Q in ((1999999, 1), (20000001, 1), (2400000, 3), (2400000, 16)):
        with pytest.raises(ValueError):
            decode_adsb.decode_adsb.fromIQ(raw, rate, Q)
    dec = decode_adsb.decode_adsb.fromIQ(raw, 2400000)
    assert dec.getMsgs == [] and dec.useful == 0 and dec.frameInfo["candidates"] == 0
