"""
APT image decoding on the device (directdemod_amd.decode_noaa, include/directdemod_hip.h: dd_median_segments_f64,
dd_apt_lines_f64, dd_apt_map_u8, dd_apt_color_u8): each primitive against numpy / SciPy / colorsys, and getImage, channelID,
the calibration and getColor end to end against the reference's results (tests/golden/apt_image_*.npz).
"""
import colorsys
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_median_segments_match_numpy(hip):
    from directdemod_amd import _ops
    from directdemod_amd._hip import DevArray
    rng = np.random.default_rng(5)
    parts, segs, off = [], [], 0
    lengths = [0, 1, 2, 3, 4, 5, 14, 31, 32, 33, 64, 579, 580, 1001, 10000, 30000, 30001, 52017]
    for i, n in enumerate(lengths * 2):
        kind = i % 6
        if kind == 0:
            x = rng.standard_normal(n)
        elif kind == 1:
            x = rng.integers(-3, 4, n).astype(np.float64)                  # many duplicates
        elif kind == 2:
            x = rng.choice([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf], n)
        elif kind == 3:
            x = rng.standard_normal(n)
            if n:
                x[rng.integers(0, n)] = np.nan
        elif kind == 4:
            x = rng.choice([-0.0, 0.0], n)
        else:
            x = rng.uniform(0, 1, n) * 1e300
        parts.append(x)
        segs.append((off, n))
        off += n
    src = np.concatenate(parts)
    d = DevArray.from_host(src, dtype=np.float64)
    got = _ops.median_segments(d, [s[0] for s in segs], [s[1] for s in segs]).to_host()
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
        ref = np.array([np.median(src[a:a + n]) for a, n in segs])
    assert _same(got, ref), [(n, g, r) for (a, n), g, r in zip(segs, got, ref) if not _same([g], [r])]


def _host_lines(env, starts, lens, use, mask_bits):
    """decode_noaa.py:346-359, 428-430 restated on the host: scipy.signal.resample + np.median, and the sync-pixel streams"""
    import scipy.signal as ss
    pix, low, high = [], [], []
    for h, (a, n) in enumerate(zip(starts, lens)):
        num = (n // 1040) * 1040
        if num == 0:
            pix.append(np.full(1040, np.nan))
            continue
        r = np.reshape(ss.resample(env[a:a + n], num), (1040, num // 1040))
        pix.append(np.median(r, axis=-1))
        if h % 2 == 0 and use[h // 2]:
            for j, bit in enumerate(mask_bits):
                (high if bit else low).extend(r[j])
    return np.concatenate(pix), np.array(low + high)


def test_line_extraction_matches_scipy(hip):
    from directdemod_amd import _ops, constants
    from directdemod_amd._hip import DevArray
    rng = np.random.default_rng(7)
    env = np.abs(rng.standard_normal(200000)).cumsum() % 3.0 + 0.1
    # half-lines of assorted lengths: typical (~15 058), shorter than one pixel row (k = 0), exact multiples of 1040
    lens = [15058, 15059, 15058, 15060, 700, 14560, 15058, 16641, 15057, 15058]
    starts, a = [], 11
    for n in lens:
        starts.append(a)
        a += n + 3
    use = [True, False, True, True, True]
    bits = constants.NOAA_SYNCA
    nlow, nhigh = bits.count(0), bits.count(1)
    off, lo, hi = [], 0, 0
    lo_tot = sum((lens[2 * i] // 1040) * nlow for i in range(5) if use[i])
    for i in range(5):
        k = lens[2 * i] // 1040
        off += [lo, lo_tot + hi] if use[i] else [-1, -1]
        off += [-1, -1]
        if use[i]:
            lo += k * nlow
            hi += k * nhigh
    d = DevArray.from_host(env, dtype=np.float64)
    mask = sum(1 << j for j, b in enumerate(bits) if b)
    pix, stream = _ops.apt_lines(d, starts, lens, off, mask, len(bits), lo_tot + hi)
    got_pix = pix.to_host()[:len(lens) * 1040]
    got_stream = stream.to_host()[:lo_tot + hi]
    with np.errstate(all="ignore"):
        ref_pix, ref_stream = _host_lines(env, starts, lens, use, bits)
    ok = ~np.isnan(ref_pix)
    assert np.array_equal(np.isnan(got_pix), ~ok)
    assert np.max(np.abs(got_pix[ok] - ref_pix[ok]) / np.abs(ref_pix[ok])) < 1e-11
    assert got_stream.shape == ref_stream.shape
    assert np.max(np.abs(got_stream - ref_stream) / np.maximum(np.abs(ref_stream), 1e-300)) < 1e-11


def _np_map(rows, params):
    out = []
    for x, (mode, a, b) in zip(rows, params):
        v = np.round(255 * (x - a) / (b - a)) if mode == 0 else np.round(x * a + b)
        v[v < 0] = 0
        v[v > 255] = 255
        out.append(v.astype(np.uint8))
    return np.array(out)


def test_mapping_bit_exact(hip):
    from directdemod_amd import _ops
    from directdemod_amd._hip import DevArray
    rng = np.random.default_rng(11)
    nrows, w = 40, 2080
    rows = rng.uniform(-0.2, 1.8, (nrows, w))
    params = []
    for r in range(nrows):
        if r % 4 == 0:                      # 255 (x - 0) / (255 - 0) = x: exact halves in the first 64 pixels
            params.append((0.0, 0.0, 255.0))
            rows[r, :64] = np.arange(64) / 2 - 3.0
        elif r % 2 == 0:
            params.append((0.0, 0.05 + 0.01 * r, 1.6 - 0.003 * r))
        else:                               # x * 128 + r: exact halves
            params.append((1.0, 128.0, float(r)))
            rows[r, :64] = (np.arange(64) - 20.5) / 128.0
    d = DevArray.from_host(rows.reshape(-1), dtype=np.float64)
    got = _ops.apt_map(d, nrows, w, params).to_host()[:nrows * w].reshape(nrows, w)
    ref = _np_map(rows, params)
    assert np.array_equal(got, ref)
    # the ties really occur: values exactly on .5 before rounding, in both modes
    for r in (0, 1):
        mode, a, b = params[r]
        x = 255 * (rows[r, :64] - a) / (b - a) if mode == 0 else rows[r, :64] * a + b
        assert np.sum((x - np.floor(x) == 0.5) & (x > 0) & (x < 255)) >= 10


def _colorsys_pixel(v, t):
    """getColor's per-pixel arithmetic (decode_noaa.py:564-595) on numpy uint8 scalars"""
    v, t = np.uint8(v), np.uint8(t)
    if t < 155.0:
        mn, mx, sv, st = [230 / 360.0, 0.2, 0.3], [230 / 360.0, 0.0, 1.0], v / 256.0, (256.0 - t) / 256.0
    elif v < 30.0:
        mn, mx, sv, st = [200.0 / 360.0, 0.7, 0.6], [240.0 / 360.0, 0.6, 0.4], v / 30.0, (256.0 - t) / (256.0 - 155.0)
    else:
        mn, mx, sv, st = [60.0 / 360.0, 0.6, 0.2], [100.0 / 360.0, 0.0, 0.5], (v - 30.0) / (90.0 - 30.0), (256.0 - t) / (256.0 - 155.0)
    s = mx[1] + st * (mn[1] - mx[1])
    vv = mx[2] + sv * (mn[2] - mx[2])
    h = mx[0] + sv * st * (mn[0] - mx[0])
    return [int(k * 255.0) for k in colorsys.hsv_to_rgb(h, s, vv)]


def test_false_colour_bit_exact_all_pairs(hip):
    from directdemod_amd import _ops
    from directdemod_amd._hip import DevArray
    v, t = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    img = np.zeros((64, 2080), dtype=np.uint8)
    flat_v, flat_t = v.reshape(-1).astype(np.uint8), t.reshape(-1).astype(np.uint8)
    img[:, :1024] = flat_v.reshape(64, 1024)
    img[:, 1040:2064] = flat_t.reshape(64, 1024)
    d = DevArray.from_host(img.reshape(-1), dtype=np.uint8)
    got = _ops.apt_color(d, 64, 2080).to_host()[:64 * 1040 * 3].reshape(64, 1040, 3)[:, :1024].reshape(-1, 3)
    ref = np.uint8(np.array([_colorsys_pixel(a, b) for a, b in zip(flat_v, flat_t)]))
    assert np.array_equal(got, ref)


# End to end the crude-rate audio differs from the reference's by up to 2e-5 rad (complex64 front end, test_c4_audio_stage_vs_golden):
# a relative error of a few 1e-5 in the envelope, which moves pixels that sit near a rounding boundary by one level.  Measured on
# MI355X: 97.8 % (plain) and 98.1 % (telemetry) of the pixels identical, none off by more than 1.
MIN_EQUAL = 0.97


def _pixel_bound(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    diff = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    assert np.mean(diff == 0) >= MIN_EQUAL, np.mean(diff == 0)
    assert diff.max() <= 1, diff.max()


@pytest.fixture(scope="module")
def plain():
    from directdemod_amd import decode_noaa, source
    from oracle import dd_oracle as O
    g = np.load(os.path.join(GOLD, "apt_image_plain.npz"))
    raw = O.synth_apt_iq(float(g["dur"]), 2048000, seed=int(g["seed"]))
    return g, source.IQarray(raw, 2048000), decode_noaa


@pytest.fixture(scope="module")
def telemetry():
    from directdemod_amd import decode_noaa, source
    from _apt_telemetry import synth_apt_telemetry_iq
    g = np.load(os.path.join(GOLD, "apt_image_telemetry.npz"))
    raw = synth_apt_telemetry_iq(float(g["dur"]), 2048000, seed=int(g["seed"]))
    return g, source.IQarray(raw, 2048000), decode_noaa


def test_image_plain_vs_golden(hip, plain):
    g, src, dn = plain
    obj = dn.decode_noaa(src, 30000.0)
    assert obj.useful == 1
    img = obj.getImage
    _pixel_bound(img, g["image"])
    assert [-1 if c is None else c for c in obj.channelID] == list(g["channel_id"])
    low, high, slope, _ = obj.calibration
    assert slope is None
    scale = g["high"] - g["low"]
    assert abs(low - g["low"]) <= 1e-4 * scale and abs(high - g["high"]) <= 1e-4 * scale
    assert np.array_equal(obj.getImageA, img[:, :1040]) and np.array_equal(obj.getImageB, img[:, 1040:])


def test_image_telemetry_vs_golden(hip, telemetry):
    g, src, dn = telemetry
    obj = dn.decode_noaa(src, 30000.0)
    img = obj.getImage
    _pixel_bound(img, g["image"])
    assert obj.channelID == [int(c) for c in g["channel_id"]]
    _, _, slope, intercept = obj.calibration
    assert abs(slope - g["slope"]) <= 5e-5 * abs(g["slope"])
    assert abs(intercept - g["intercept"]) <= 0.01                  # output levels (of 255): the intercept itself is near 0
    col = obj.getColor
    # the colour of our own image is exact; against the reference's, a pixel one level off near a branch limit (t = 155,
    # v = 30) changes its colour entirely, so only the share of identical values is bounded
    ref_col = np.uint8(np.array([[_colorsys_pixel(v, t) for v, t in zip(ra, rb)] for ra, rb in zip(img[:, :1040], img[:, 1040:])]))
    assert np.array_equal(col, ref_col)
    assert col.shape == g["color"].shape and np.mean(col == g["color"]) >= MIN_EQUAL


def test_image_deterministic_under_lds_fill(hip, plain):
    g, src, dn = plain
    first = dn.decode_noaa(src, 30000.0).getImage
    hip.check(hip.lib().dd_debug_fill_lds(0xFFFFFFFF, None), "dd_debug_fill_lds")
    second = dn.decode_noaa(src, 30000.0).getImage
    assert np.array_equal(first, second)


def test_accurate_sync_eight_columns(hip):
    from directdemod_amd import decode_noaa, source
    from oracle import dd_oracle as O
    g = np.load(os.path.join(GOLD, "noaa_c4_60s.npz"))
    raw = O.synth_apt_iq(float(g["dur"]), 2048000, seed=int(g["seed"]))
    acc = decode_noaa.decode_noaa(source.IQarray(raw, 2048000), 30000.0).getAccurateSync()
    assert len(acc) == 8
    assert np.array_equal(acc[0], g["acc_syncA"]) and np.array_equal(acc[4], g["acc_syncB"])
    assert np.array_equal(acc[1], np.diff(g["acc_syncA"])) and np.array_equal(acc[5], np.diff(g["acc_syncB"]))
    assert len(acc[2]) == len(acc[3]) == len(acc[0]) and len(acc[6]) == len(acc[7]) == len(acc[4])
