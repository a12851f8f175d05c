"""The RDS kernels on the device (dd_rds.h through dd_rds_baseband, dd_rds_candidates, dd_rds_groups and the diagnostics
dd_debug_rds_masks, dd_debug_rds_halfbit and dd_debug_rds_repair, the wrappers of directdemod_amd/rds.py and decode_rds) against the
NumPy restatement in rds.py.

Everything behind the quantiser is integer, so every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import _rds as T
from directdemod_amd import decode_rds, rds, source

pytestmark = pytest.mark.gpu

SENT = np.int64(-0x5A5A5A5A5A5A5A5B)
SENT32 = np.int32(-0x5A5A5A5B)
SPARE = 16
SPS = [12.0, 16.842, 31.9]
KEYS = ("t", "words", "status", "third", "metric", "state", "good")


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def dev_pairs(hip, b):
    """int32[m, 2] -> the device array the entries read (one spare pair when empty)"""
    b = np.ascontiguousarray(b, dtype=np.int32).reshape(-1, 2)
    return hip.DevArray.from_host(b.ravel() if len(b) else np.zeros(2, np.int32)), len(b)


# ---------------------------------------------------------------------------------------------------------------- baseband
def dev_baseband(hip, mpx, d, step, n0):
    """dd_rds_baseband with sentinels behind its output -> int32[n // d, 2]"""
    nout = len(mpx) // d
    x = hip.DevArray.from_host(np.ascontiguousarray(mpx if len(mpx) else np.zeros(1), dtype=np.float64))
    out = hip.DevArray.from_host(np.full(2 * nout + SPARE, SENT32, np.int32))
    rc = hip.lib().dd_rds_baseband(x.ptr, len(mpx), d, n0, step, rds.table_device().ptr, out.ptr, None)
    hip.sync()
    got = out.to_host()
    assert rc == 0 and np.all(got[2 * nout:] == SENT32)
    return got[:2 * nout].reshape(nout, 2)


def rough_multiplex(n, seed):
    """noise at a third of full scale with a NaN, infinities, +-pi exactly, values just inside and beyond the clip"""
    x = np.random.default_rng(seed).normal(0.0, 1.0, n)
    special = [np.nan, np.inf, -np.inf, np.pi, -np.pi, np.nextafter(np.pi, 4.0), 3.2, -3.2, 1e300, 0.0, -0.0]
    for k, v in enumerate(special):
        if 7 * k + 3 < n:
            x[7 * k + 3] = v
    return x


@pytest.mark.parametrize("rate", [171000.0, 240000.0, 250000.0, 384000.0])
@pytest.mark.parametrize("n0", [0, 1 << 40])
def test_baseband(hip, rate, n0):
    d, _, step = rds.params(rate)
    tile = rds.TILE * d
    for n in (0, 1, d - 1, d, d + 1, tile - 1, tile, tile + 1, 2 * tile + d - 1, 3 * tile + 5 * d):
        x = rough_multiplex(n, n + int(rate))
        want = rds.baseband_sums_host(x, d, step, n0)
        got = dev_baseband(hip, x, d, step, n0)
        assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want), n
    assert rds.quantise([np.pi, -np.pi, np.nextafter(np.pi, 4.0), 3.2, np.nan]).tolist() == [32768, -32768, 32768, 0, 0]


@pytest.mark.parametrize("d", [9, rds.D_MAX])
def test_baseband_at_full_scale(hip, d):
    """every sample at +-pi with the sign of the phasor's component: the largest sum the stage can make stays inside the budget
    (|b| <= 2^24 at D = 32) and equals the int64 restatement, so nothing wrapped"""
    step = rds.params(171000.0)[2]
    n = (rds.TILE + 3) * d
    for n0 in (0, 1 << 40):
        for comp in (0, 1):
            x = np.where(rds.table()[rds.phases(n0, n, step), comp] >= 0, np.pi, -np.pi)
            want = rds.baseband_sums_host(x, d, step, n0)
            assert np.abs(want).max() <= 1 << 24 and np.abs(want[:, comp]).min() > (d << 19) * 0.5
            assert np.array_equal(dev_baseband(hip, x, d, step, n0).astype(np.int64), want)


# ---------------------------------------------------------------------------------------------------------------- half-bit differences
def check_halfbit(hip, b, sps):
    b = np.asarray(b, dtype=np.int32).reshape(-1, 2)
    dev, m = dev_pairs(hip, b)
    want = rds.halfbit_host(b, int(sps // 2))
    got = rds.halfbit_device(dev, m, sps)
    assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want)
    return want


@pytest.mark.parametrize("sps", SPS)
def test_halfbit_differences(hip, sps):
    h = int(sps // 2)
    rng = np.random.default_rng(int(sps * 10))
    for m in (0, 1, h, 2 * h - 1, 2 * h, 2 * h + 1, rds.TILE - 1, rds.TILE, rds.TILE + 1, rds.TILE + h, 2 * rds.TILE + h + 1, 1000):
        z = check_halfbit(hip, rng.integers(-(1 << 24), (1 << 24) + 1, (m, 2)), sps)
        if m >= 2 * h + 2:
            assert not z[:h].any() and not z[m - h + 1:].any() and z[h].any() and z[m - h].any()     # the first and last h samples


@pytest.mark.parametrize("sps", SPS)
def test_halfbit_differences_at_full_scale(hip, sps):
    """a square wave of +-2^24 whose half period is h: |z| reaches 2 h 2^24 (2^29 at h = 16), and the 32-bit prefix sums of a tile
    wrap, which their differences undo"""
    h = int(sps // 2)
    m = 3 * rds.TILE + 7
    sq = np.where((np.arange(m) // h) % 2 == 0, 1 << 24, -(1 << 24))
    z = check_halfbit(hip, np.stack((sq, -sq), axis=1), sps)
    assert np.abs(z).max() == 2 * h << 24
    z = check_halfbit(hip, np.full((m, 2), 1 << 24), sps)                # a constant at full scale: the prefix sum wraps, z is 0
    assert not z.any()


# ---------------------------------------------------------------------------------------------------------------- candidates
def dev_candidates(hip, b, sps, clean, cap):
    """dd_rds_candidates with `cap` places and SPARE sentinels behind them -> (rc, count, the places, the sentinels still whole)"""
    dev, m = dev_pairs(hip, b)
    lst = hip.DevArray.from_host(np.full(cap + SPARE, SENT))
    count = C.c_int64(-1)
    rc = hip.lib().dd_rds_candidates(dev.ptr, m, float(sps), int(clean), lst.ptr, cap, C.byref(count), None)
    hip.sync()
    got = lst.to_host()
    return rc, count.value, got[:cap], bool(np.all(got[cap:] == SENT))


def check_candidates(hip, b, sps, clean=3):
    """the device's list and, through the diagnostic entry, its mask bytes (the scores) against the restatement's -> the scores"""
    scores = rds.scores_host(b, sps)
    want = np.flatnonzero(scores >= clean).astype(np.int64)
    rc, count, got, whole = dev_candidates(hip, b, sps, clean, len(want) + 3)
    assert rc == 0 and count == len(want) and whole
    assert np.array_equal(got[:count], want) and np.all(got[count:] == SENT)
    if len(b):
        dev, m = dev_pairs(hip, b)
        assert np.array_equal(rds.masks_device(dev, m, sps, clean), (scores << 1 | (scores >= clean)).astype(np.uint8))
    return scores


def some_groups():
    return [T.group_bits(g) for g in T.station_groups()[:3]] + [T.group_bits(rds.group_0a(T.PI, T.PS, 1, version="B"))]


@pytest.mark.parametrize("sps", SPS)
@pytest.mark.parametrize("clean", [2, 3, 4])
def test_candidates_on_noise(hip, sps, clean):
    """four groups, the last of version B (C'), under noise at a quarter of their amplitude: some tens of tiles"""
    b, starts = T.planted(some_groups(), sps, noise=800, seed=int(sps) + clean)
    scores = check_candidates(hip, b, sps, clean)
    assert [int(scores[t]) for t in starts] == [4, 4, 4, 4]
    noise = np.rint(np.random.default_rng(clean).normal(0.0, 5000.0, (3 * rds.TILE + 11, 2))).astype(np.int32)
    check_candidates(hip, noise, sps, clean)


@pytest.mark.parametrize("sps", SPS)
def test_a_group_that_ends_on_the_last_admissible_sample(hip, sps):
    h = int(sps // 2)
    bits = some_groups()[0]
    t = 300
    full = int(rds.positions([t], [rds.BITS - 1], sps)[0, 0]) + h        # p_103 = m - h
    b = T.craft(bits, sps, t, full + 50)
    assert rds.fits([t], sps, full)[0] and not rds.fits([t], sps, full - 1)[0]
    assert check_candidates(hip, b[:full], sps, 4)[t] == 4               # the last start that fits, and it is listed
    assert check_candidates(hip, b[:full - 1], sps, 4)[t] == 0           # one sample less: it does not fit
    first = int(np.ceil(sps - 0.5))                                      # the first start with p_-1 >= 0; its p_-1 lies below h: zeros
    assert rds.fits([first], sps, full)[0] and not rds.fits([first - 1], sps, full)[0]
    check_candidates(hip, T.craft(bits, sps, first, full), sps, 2)
    for m in (0, 1, int(104 * sps)):                                     # no start fits
        rc, count, got, whole = dev_candidates(hip, b[:m], sps, 2, 4)
        assert (rc, count, whole) == (0, 0, True) and np.all(got == SENT)


def test_each_bit_flipped_singly(hip):
    """104 copies of a version A group, copy k with bit k flipped, and 26 of a version B group with a bit of the third block
    flipped: the score at the start is 3, as the restatement says, and the whole mask array is equal"""
    sps = 16.842
    for words, which in ((T.station_groups()[0], range(rds.BITS)), (rds.group_0a(T.PI, T.PS, 2, version="B"), range(52, 78))):
        bits = T.group_bits(words)
        flipped = []
        for k in which:
            f = bits.copy()
            f[k] ^= 1
            flipped.append(f)
        b, starts = T.planted(flipped, sps, gap=10)
        scores = check_candidates(hip, b, sps, 3)
        assert [int(scores[t]) for t in starts] == [3] * len(which)
    # C against C': a version A group whose third block carries C' and the other way round are clean in the third block all the same
    swapped = list(rds.group_blocks(T.station_groups()[0]))
    swapped[2] ^= rds.OFFSETS[rds.CC] ^ rds.OFFSETS[rds.CP]
    bits = np.array([blk >> i & 1 for blk in swapped for i in range(25, -1, -1)], dtype=np.uint8)
    b, starts = T.planted([bits], sps)
    assert check_candidates(hip, b, sps, 4)[starts[0]] == 4


@pytest.mark.parametrize("sps", SPS)
def test_zero_products(hip, sps):
    """a product of zero is bit 0: silence reads as blocks of zeros, whose remainder 0 is no offset word; a group with a stretch of
    silence inside reads zeros there"""
    assert not check_candidates(hip, np.zeros((2 * rds.TILE + 500 + int(104 * sps), 2), np.int32), sps, 2).any()
    b, starts = T.planted(some_groups()[:2], sps)
    t = starts[0]
    b[t + int(30 * sps):t + int(50 * sps)] = 0
    b[starts[1] + int(80 * sps):] = 0
    scores = check_candidates(hip, b, sps, 2)
    assert 0 < int(scores[t]) < 4 and 0 < int(scores[starts[1]]) < 4


def test_list_capacity(hip):
    sps = 16.0
    b, starts = T.planted(some_groups(), sps)
    want = rds.candidates_host(b, sps, 3)
    assert len(want) > 8
    for cap in (0, 1, len(want) - 1):
        rc, count, got, whole = dev_candidates(hip, b, sps, 3, cap)
        assert rc == hip.DD_ERR_INVALID and count == len(want) and whole and np.array_equal(got, want[:cap])
    dev, m = dev_pairs(hip, b)
    lst, count = rds.candidates(dev, m, sps, 3, cap=1)                   # the wrapper asks again at the true count
    assert count == len(want) and np.array_equal(lst.to_host()[:count], want)


# ---------------------------------------------------------------------------------------------------------------- block repair
@pytest.fixture(scope="module")
def damaged_words():
    """(words, offset indices): every burst on a block of every offset word; then 6-bit bursts and pairs of separate errors"""
    rng = np.random.default_rng(8)
    words, offs = [], []
    for o in range(5):
        good = rds.block(int(rng.integers(0, 1 << 16)), o)
        words.append(good)
        offs.append(o)
        for e, _, _, _ in rds.bursts():
            words.append(good ^ e)
            offs.append(o)
    first = len(words)
    for o in range(5):
        good = rds.block(int(rng.integers(0, 1 << 16)), o)
        for up in range(21):
            for mid in (0, 6, 9, 15):
                words.append(good ^ (0x21 | mid << 1) << up)               # a burst of six
                offs.append(o)
        for _ in range(60):
            i, j = sorted(rng.choice(26, 2, replace=False))
            if j - i >= 5:
                words.append(good ^ 1 << i ^ 1 << j)                       # two errors too far apart for one burst
                offs.append(o)
    return np.array(words, dtype=np.uint32), np.array(offs, dtype=np.int32), first


@pytest.mark.parametrize("fix", [0, 1, 2, 3, 4, 5])
def test_block_repair(hip, damaged_words, fix):
    words, offs, first = damaged_words
    want = [rds.repair_np(w, o, fix) for w, o in zip(words.tolist(), offs.tolist())]
    fixed, status = rds.repair_device(words, offs, fix)
    assert fixed.tolist() == [w for w, _ in want] and status.tolist() == [s for _, s in want]
    per = 1 + 367
    for o in range(5):                                                   # a burst of at most `fix` bits comes out, a longer one stays
        good = int(words[o * per])
        lens = np.array([ln for _, _, ln, _ in rds.bursts()])
        st = status[o * per + 1:(o + 1) * per]
        assert status[o * per] == 0 and np.all((st > 0) == (lens <= fix)) and np.all(st[lens > fix] == -1)
        assert np.all(fixed[o * per + 1:(o + 1) * per][lens <= fix] == good)
    beyond = status[first:]                                              # not decodable, or the restatement's miscorrection
    assert np.all((beyond == -1) | (beyond > 0)) and (fix < 5 or (beyond > 0).any())
    assert rds.repair_device(np.zeros(0, np.uint32), np.zeros(0, np.int32), fix)[1].shape == (0,)


# ---------------------------------------------------------------------------------------------------------------- groups
def dev_groups(hip, b, sps, fix, ts):
    """dd_rds_groups with sentinels behind both outputs -> the dict of rds.groups_host"""
    n = len(ts)
    dev, m = dev_pairs(hip, b)
    lst = hip.DevArray.from_host(np.ascontiguousarray(ts, dtype=np.int64))
    words = hip.DevArray.from_host(np.full(4 * n + SPARE, 0xA5A5, np.uint16))
    meta = hip.DevArray.from_host(np.full(8 * n + SPARE, SENT32, np.int32))
    rc = hip.lib().dd_rds_groups(dev.ptr, m, float(sps), int(fix), lst.ptr, n, words.ptr, meta.ptr, None)
    hip.sync()
    assert rc == 0
    w, mt = words.to_host(), meta.to_host()
    assert np.all(w[4 * n:] == 0xA5A5) and np.all(mt[8 * n:] == SENT32)
    mt = mt[:8 * n].reshape(n, 8)
    return {"t": np.asarray(ts, dtype=np.int64), "words": w[:4 * n].reshape(n, 4), "status": mt[:, 0:4], "third": mt[:, 4],
            "metric": mt[:, 5], "state": mt[:, 6], "good": mt[:, 7]}


def check_groups(hip, b, sps, fix, ts):
    got = dev_groups(hip, b, sps, fix, ts)
    want = rds.groups_host(b, sps, fix, ts)
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    return got


@pytest.mark.parametrize("sps", SPS)
@pytest.mark.parametrize("count", [1, 65, 300])
def test_groups(hip, sps, count):
    """starts around four planted groups under noise, starts outside the data and starts whose group does not fit among them"""
    b, starts = T.planted(some_groups(), sps, noise=900, seed=count)
    m = len(b)
    rng = np.random.default_rng(count + int(sps))
    outside = [-1, -5000, m, m + 7, 1 << 40, 0, 1, m - 1, m - int(50 * sps)]
    near = [t + int(dt) for t in starts for dt in rng.integers(-int(sps), int(sps) + 1, 80)]
    ts = (starts + outside + near)[:count] if count > 1 else [starts[1]]
    det = check_groups(hip, b, sps, 2, ts)
    if count > 1:
        assert det["state"][4:4 + len(outside)].tolist() == [rds.OUTSIDE] * len(outside)
        assert det["good"][:4].tolist() == [4] * 4 and det["third"][:4].tolist() == [0, 0, 0, 1]
        assert [tuple(w) for w in det["words"][:3].tolist()] == T.station_groups()[:3]
    assert 0 <= det["metric"].min() and det["metric"].max() <= rds.BITS * rds.METRIC_CAP
    check_groups(hip, np.zeros((0, 2), np.int32), sps, 2, [0, 5])        # no data: every start is outside


@pytest.mark.parametrize("fix", [0, 2, 5])
def test_groups_repair_and_the_third_offset(hip, fix):
    """bursts in every block; version B with block 2 damaged beyond repair, where the third block's own remainder says C'; and
    neither: C"""
    sps = 16.842
    a, bb = T.station_groups()[1], rds.group_0a(T.PI, T.PS, 3, version="B")

    def hit(words, errors):
        blocks = rds.group_blocks(words)
        for blk, e in errors:
            blocks[blk] ^= e
        return np.array([v >> i & 1 for v in blocks for i in range(25, -1, -1)], dtype=np.uint8)
    cases = [hit(a, [(0, 1 << 25), (1, 3 << 7), (2, 0x15 << 3), (3, 0x1F)]),          # bursts of 1, 2, 5 and 5 bits
             hit(bb, [(1, 0x2041 << 4)]),                                            # version B, block 2 not decodable: C' by block 3
             hit(bb, [(1, 0x2041 << 4), (2, 0x1001 << 2)]),                          # and block 3 damaged as well: C, not decodable
             hit(bb, [(1, 1 << 21)]),                                                # block 2 "repaired" keeps its version bit's error
             hit(a, [(1, 1 << 21)])]
    b, starts = T.planted(cases, sps, amp=(-2500, 2000))
    det = check_groups(hip, b, sps, fix, starts)
    assert det["status"][1].tolist() == [0, -1, 0, 0] and det["third"][1] == 1
    assert det["status"][2].tolist()[:2] == [0, -1] and det["third"][2] == 0
    assert det["status"][0].tolist() == [1 if fix >= 1 else -1, 2 if fix >= 2 else -1, 3 if fix >= 5 else -1, 5 if fix >= 5 else -1]
    if fix == 5:
        assert tuple(det["words"][0].tolist()) == a


def test_groups_at_full_scale(hip):
    """z of 2 h 2^24 in both components: the products reach 2^59 and the metric its cap in every bit"""
    sps = 31.9
    b, starts = T.planted(some_groups()[:1], sps, amp=(1 << 24, -(1 << 24)))
    det = check_groups(hip, b, sps, 2, starts)
    assert det["good"][0] == 4 and det["metric"][0] == rds.BITS * rds.METRIC_CAP
    check_candidates(hip, b, sps, 4)


# ---------------------------------------------------------------------------------------------------------------- end to end
def same_groups(got, want):
    assert len(got) == len(want)
    for g, v in zip(got, want):
        assert g == v


@pytest.mark.parametrize("clock_ppm", [0.0, 100.0, -100.0])
def test_end_to_end(hip, clock_ppm):
    """decode_rds over 0.63 s of synthesised IQ at 1.2 MS/s.  Its front end is float32 on the device, which float64 NumPy does not
    repeat bit for bit; so the device decoder is held exactly (groups, frameInfo, candidates) to the restatement run over the
    device's own multiplex, and to what was sent."""
    raw = T.recording(clock_ppm, clock_ppm)
    dec = decode_rds.decode_rds(source.IQarray(np.array(raw), T.FS), T.CHANNEL)
    assert dec.audioRate == 240000.0
    mpx = dec.audio().to_host()
    found, info, cands = rds.decode(mpx, dec.audioRate, ops=rds.HostOps())
    same_groups(dec.getGroups, [decode_rds._public(g) for g in found])
    assert dec.frameInfo == info and dec.useful == 1 and info["groups"] == 7
    got = dec.candidateInfo
    for key in KEYS:
        assert np.array_equal(got[key], cands[key]), key
    assert [tuple(g["words"]) for g in dec.getGroups] == T.station_groups()
    assert list(dec.getStations) == [T.PI] and dec.getStations == decode_rds.stations_host(dec.getGroups)
    T.same_station(dec.getStations[T.PI])
    assert dec.getText == ["RDS D318 PS: 'RADIO 1 ' RT: 'Hi RDS' CT: 2023-02-25T13:37:00Z +1.0 h"]
    assert set(dec.timings) == {"front_end", "baseband", "candidates", "groups", "host"}
    if clock_ppm == 0.0:
        hfound, hinfo = decode_rds.decode_host(np.array(raw), T.FS, T.CHANNEL)
        assert [tuple(g["words"]) for g in hfound] == T.station_groups() and hinfo["groups"] == 7


def test_from_audio_on_the_device_and_on_the_host(hip):
    rate = 240000.0
    bits = rds.air_bits(T.station_groups())
    bits[4 * rds.BITS:4 * rds.BITS + 26] ^= 1                            # group 4 loses its first block,
    bits[4 * rds.BITS + 80:4 * rds.BITS + 104] ^= 1                      # and its last: followed from group 3
    x = rds.encode_mpx(bits, rate, start=0.01, clock_ppm=60.0, phase=2.0, sigma=0.01, seed=2)
    for follow, count in ((2, 7), (0, 6)):
        want, info = decode_rds.decode_audio_host(x, rate, follow=follow)
        assert len(want) == count and info["followed"] == (1 if follow else 0)
        for mpx in (x, hip.DevArray.from_host(x)):
            dec = decode_rds.decode_rds.fromAudio(mpx, rate, follow=follow)
            same_groups(dec.getGroups, want)
            assert dec.frameInfo == info
    cut = int((0.01 + 0.5 * rds.BITS / rds.BITRATE) * rate)              # a stream that starts inside the first group
    dec = decode_rds.decode_rds.fromAudio(hip.DevArray.from_host(x[cut:]), rate)
    same_groups(dec.getGroups, decode_rds.decode_audio_host(x[cut:], rate)[0])
    assert len(dec.getGroups) == 6
    empty = decode_rds.decode_rds.fromAudio(np.zeros(10), rate)
    assert empty.getGroups == [] and empty.useful == 0 and empty.frameInfo["groups"] == 0 and empty.getStations == {}
