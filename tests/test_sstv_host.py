"""The SSTV chain's NumPy restatement and host logic (directdemod_amd/sstv.py) on the CPU: the polynomial
arctangent, the VIS parser, the sync-grid fit, the colour form, the synthesiser, and the whole restatement against the picture that
was sent.  The device is held to the restatement exactly (tests/test_gpu_sstv.py), so what is measured here is the decoder's error.

The error limits are not fixed in advance: MEASURED holds (mean, maximum) absolute error in RGB levels of each case as the
restatement gave them when this file was written, and each test asserts twice those.  The cases guard against gross faults (a
channel swapped, a line or pixel offset, a wrong delay), which cost tens of levels.  Pixels within one filter length of a segment
edge, and in the bar rows of a bar edge, are excluded: there the frequency jumps."""
import logging
import math

import numpy as np
import pytest

from directdemod_amd import sstv

RATE = 24000
PAIRS = 4
NOISE_SIGMA = 0.05                     # white Gaussian noise on a tone of amplitude 1: 23 dB signal to noise over the whole band

# case -> (mean, max) over the smooth rows, (mean, max) inside the flat bars, measured with the restatement
MEASURED = {
    ("PD50", "clean"): ((0.029, 2), (0.014, 2)),
    ("PD50", "noisy"): ((3.255, 20), (3.286, 19)),
    ("PD50", "slant"): ((0.049, 3), (0.023, 2)),
    ("PD120", "clean"): ((0.267, 3), (0.184, 3)),
    ("PD120", "noisy"): ((3.524, 21), (3.356, 22)),
    ("PD120", "slant"): ((0.266, 3), (0.198, 2)),
    ("PD50", "iq"): ((0.599, 5), (0.549, 3)),
}
CASES = {"clean": dict(clock_error=0.0, sigma=0.0), "noisy": dict(clock_error=0.0, sigma=NOISE_SIGMA),
         "slant": dict(clock_error=1e-3, sigma=0.0)}


def sent(mode, pairs=PAIRS):
    """-> (y, cr, cb, the RGB picture a decoder without error gives)"""
    y, cr, cb = sstv.card(mode, pairs)
    return y, cr, cb, sstv.color_host(np.stack((y[0::2], cr, cb, y[1::2]), axis=1))


def audio_of(mode, case, pairs=PAIRS, rate=RATE, vis=True, seed=5):
    c = CASES[case]
    y, cr, cb, _ = sent(mode, pairs)
    x = sstv.synth(*sstv.tones(y, cr, cb, mode, vis), rate, c["clock_error"])
    if c["sigma"]:
        x = x + c["sigma"] * np.random.default_rng(seed).standard_normal(len(x))
    return x


def excluded(mode, rate=RATE):
    """pixels left out at each jump of the frequency: one filter length"""
    return int(math.ceil(sstv.tap_count(rate) / (sstv.MODES[mode].pixel * rate)))


def errors(img, mode, rate=RATE):
    """image against the sent picture -> ((mean, max) over the smooth rows, (mean, max) inside the bars)"""
    m = sstv.MODES[mode]
    want = sent(mode, img.shape[0] // 2)[3]
    e = np.abs(img.astype(np.int64) - want.astype(np.int64))
    ex = excluded(mode, rate)
    assert 2 * ex < m.width / 4                          # the excluded pixels stay below a quarter of a segment
    cols = np.ones(m.width, dtype=bool)
    cols[:ex] = cols[-ex:] = False
    bars = np.zeros(img.shape[0], dtype=bool)
    bars[1::8] = True
    inner = cols.copy()
    for j in range(1, 8):
        at = -(-j * m.width // 8)
        inner[max(at - ex, 0):at + ex] = False
    es, eb = e[~bars][:, cols], e[bars][:, inner]
    return (float(es.mean()), int(es.max())), (float(eb.mean()), int(eb.max()))


def check_errors(img, mode, case, rate=RATE):
    got = errors(img, mode, rate)
    print("%s %s: smooth rows mean %.3f max %d, inside bars mean %.3f max %d" % (mode, case, *got[0], *got[1]))
    for (mean, worst), (mean0, worst0) in zip(got, MEASURED[(mode, case)]):
        assert mean <= 2 * mean0 and worst <= 2 * worst0, (mode, case, got)
    return got


# ------------------------------------------------------------------------------------------------------------------ arctangent
def test_arctangent_accuracy():
    """against math.atan2 over the upper half plane, the axes and tiny and huge magnitudes included: at most a hundredth of a grey
    level at the largest audio rate, where one level is 2 pi (800 / 255) / rate rad.  Measured maximum: see the assertion below."""
    th = np.concatenate((np.linspace(0.0, np.pi, 400001), [np.pi / 8, np.pi / 4, 3 * np.pi / 8, np.pi / 2, 5 * np.pi / 8]))
    limit = 2 * np.pi * (800.0 / 255.0) / sstv.RATE_MAX / 100.0
    worst = 0.0
    for mag in (1e-300, 1e-150, 1e-9, 1.0, 3.7e5, 1e150, 1e300):
        x, y = mag * np.cos(th), np.abs(mag * np.sin(th))
        ref = np.array([math.atan2(b, a) for a, b in zip(x, y)])
        worst = max(worst, float(np.abs(sstv.atan_host(x, y) - ref).max()))
    for x, y, ref in ((1.0, 0.0, 0.0), (-1.0, 0.0, np.pi), (0.0, 1.0, np.pi / 2), (1.0, 1.0, np.pi / 4), (-1.0, 1.0, 3 * np.pi / 4),
                      (5e-324, 5e-324, np.pi / 4), (1e308, 5e-324, 0.0), (-1e308, 5e-324, np.pi), (5e-324, 1e308, np.pi / 2)):
        worst = max(worst, abs(float(sstv.atan_host(x, y)) - ref))
    print("arctangent: largest error %.3g rad, limit %.3g rad" % (worst, limit))
    assert worst <= limit
    assert worst < 4e-9                                  # the series' own truncation, tan(pi / 8)^19 / 19 = 2.8e-9


# ------------------------------------------------------------------------------------------------------------------ VIS
def vis_classes(code, rate=RATE, flip=None, tail=0.05, cut=None):
    """tone classes of a VIS header for `code` (bit `flip` inverted, parity bit as for the true code), then `tail` s of sync"""
    t = sstv.vis_tones(code)
    if flip is not None:
        f, s = t[4 + flip]
        t[4 + flip] = (sstv.F_ONE if f == sstv.F_ZERO else sstv.F_ZERO, s)
    x = sstv.synth([f for f, _ in t] + [sstv.F_SYNC, sstv.F_PORCH], [s for _, s in t] + [tail, 0.01], rate)
    if cut is not None:
        x = x[:int(cut * rate)]
    return sstv.classes_host(*sstv.lag_host(x, *sstv.design(rate)), sstv.edges(rate))


@pytest.mark.parametrize("name", sorted(sstv.MODES))
def test_vis_parser_codes(name):
    code = sstv.MODES[name].vis
    cls = vis_classes(code)
    wl = int(round(sstv.LEADER_S * RATE))
    leaders = sstv.runs_host(cls, sstv.CLS_LEADER, wl, math.ceil(sstv.LEADER_FRACTION * wl))
    assert len(leaders) >= 1
    for p in leaders:
        h = sstv.parse_vis(cls[p:], RATE)
        assert h is not None and h["code"] == code and h["parity_ok"] is True
        start_bit = p + h["start_bit"] + sstv.sync_edge(RATE) - sstv.delay(sstv.tap_count(RATE))
        assert abs(start_bit - (2 * sstv.LEADER_S + sstv.BREAK_S) * RATE) <= 0.002 * RATE       # within 2 ms: a bit lasts 30
    for flip in (0, 3, 6):
        h = sstv.parse_vis(vis_classes(code, flip=flip)[leaders[0]:], RATE)
        assert h is not None and h["code"] == code ^ (1 << flip) and h["parity_ok"] is False


def test_vis_cut_off_and_absent():
    code = sstv.MODES["PD120"].vis
    for cut in (0.5, 0.62, 0.7, 0.85, 0.89):                             # inside the leader, the start bit, the bits, the stop bit
        assert sstv.parse_vis(vis_classes(code, cut=cut), RATE) is None, cut
        assert sstv.decode_host(sstv.synth(*zip(*sstv.vis_tones(code)), RATE)[:int(cut * RATE)], RATE) == ([], [])
    assert sstv.parse_vis(vis_classes(code, cut=0.905), RATE)["code"] == code       # the stop bit's middle half is all there
    assert sstv.parse_vis(np.zeros(10, dtype=np.int8), RATE) is None
    assert sstv.parse_vis(np.full(RATE, sstv.CLS_1200, dtype=np.int8), RATE) is None    # a start bit needs a leader before it
    assert sstv.parse_vis(np.full(RATE, sstv.CLS_LEADER, dtype=np.int8), RATE) is None


def test_parity_failure_rejected_unless_forced(caplog):
    m = sstv.MODES["PD50"]
    y, cr, cb, _ = sent("PD50")
    f, s = sstv.tones(y, cr, cb, m)
    f = f.copy()
    f[4] = sstv.F_ONE if f[4] == sstv.F_ZERO else sstv.F_ZERO            # data bit 0 flipped: code 92, parity wrong
    x = sstv.synth(f, s, RATE)
    with caplog.at_level(logging.INFO):
        images, infos = sstv.decode_host(x, RATE)
    assert images == [] and infos == [] and "skipped" in caplog.text
    images, infos = sstv.decode_host(x, RATE, "PD50")
    assert len(images) == 1 and infos[0]["parity_ok"] is False and infos[0]["vis"] == 92 and infos[0]["mode"] == "PD50"
    check_errors(images[0], "PD50", "clean")


# ------------------------------------------------------------------------------------------------------------------ grid fit
@pytest.mark.parametrize("clock_error", [0.0, 1e-3, -1e-3])
def test_grid_fit(clock_error):
    period0, start = 12203.52, 21844.25
    period = period0 * (1 + clock_error)
    exact = start + period * np.arange(248)
    rng = np.random.default_rng(3)
    spurious = np.sort(np.concatenate((exact, start + period * (rng.integers(0, 247, 60) + rng.uniform(0.15, 0.85, 60)))))
    for what, cands, count in (("exact", exact, 248), ("every third missing", exact[np.arange(248) % 3 != 2], 166),
                               ("spurious", spurious, 248)):
        ks, ps, s, p = sstv.match_grid(cands, start + 3.0, period0, 0, 248)
        assert len(ks) == count and abs(s - start) < 1e-6 and abs(p - period) < 1e-8, (what, len(ks), s, p)
    # a header places line 0 and its own sync is never matched (k0 = 1); the start estimate may be a few milliseconds off
    ks, ps, s, p = sstv.match_grid(exact[1:], start + 100.0, period0, 1, 248)
    assert ks[0] == 1 and len(ks) == 247 and abs(s - start) < 1e-6 and abs(p - period) < 1e-8
    assert sstv.match_grid(np.zeros(0), start, period0, 0, 10) == ([], [], start, period0)
    assert sstv.fit_grid([5], [start + 5 * period0], 0.0, period0) == (start, period0)


# ------------------------------------------------------------------------------------------------------------------ colour
def test_colour_form():
    lv = []
    for y in (0, 255):
        for cr in (0, 255):
            for cb in (0, 255):
                lv.append((y, cr, cb))
    lv.append((128, 128, 128))
    levels = np.zeros((len(lv), 4, 1), dtype=np.uint8)
    for i, (y, cr, cb) in enumerate(lv):
        levels[i, :, 0] = (y, cr, cb, 255 - y)
    rgb = sstv.color_host(levels)
    clip = lambda v: max(0, min(255, v))
    for i, (y, cr, cb) in enumerate(lv):
        for row, yy in enumerate((y, 255 - y)):
            want = (clip((100 * yy + 140 * cr - 17850) // 100), clip((100 * yy - 71 * cr - 33 * cb + 13260) // 100),
                    clip((100 * yy + 178 * cb - 22695) // 100))
            assert tuple(int(v) for v in rgb[2 * i + row, 0]) == want, (y, cr, cb, row)
    assert tuple(int(v) for v in rgb[16, 0]) == (128, 127, 128)          # mid-grey


# ------------------------------------------------------------------------------------------------------------------ the synthesiser
@pytest.mark.parametrize("name", sorted(sstv.MODES))
def test_encode_durations(name):
    m = sstv.MODES[name]
    y, cr, cb = sstv.card(m, 2)
    f, s = sstv.tones(y, cr, cb, m)
    assert len(f) == 13 + 2 * (2 + 4 * m.width)
    assert abs(s.sum() - (sstv.VIS_S + 2 * sstv.line_time(m))) < 1e-9
    assert abs(m.height // 2 * sstv.line_time(m) - {"PD50": 49.68, "PD90": 89.99, "PD120": 126.1, "PD160": 160.9, "PD180": 187.1,
                                                    "PD240": 248.0, "PD290": 288.7}[name]) < 0.06
    f0, s0 = sstv.tones(y, cr, cb, m, vis=False)
    assert len(f0) == len(f) - 13 and abs(s0.sum() - 2 * sstv.line_time(m)) < 1e-9
    rgb = np.zeros((4, m.width, 3), dtype=np.uint8)
    x = sstv.encode(rgb, m, 8000, clock_error=1e-3)
    assert len(x) == int(math.floor(s.sum() * 1.001 * 8000 + 1e-9)) and np.abs(x).max() <= 1.0
    with pytest.raises(ValueError):
        sstv.encode(np.zeros((4, m.width + 1, 3), dtype=np.uint8), m, 8000)


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("mode", ["PD50", "PD120"])
@pytest.mark.parametrize("case", ["clean", "noisy"])
def test_restatement_against_sent_picture(mode, case):
    images, infos = sstv.decode_host(audio_of(mode, case), RATE)
    assert len(images) == 1 and images[0].shape == (2 * PAIRS, sstv.MODES[mode].width, 3)
    i = infos[0]
    assert i["mode"] == mode and i["vis"] == sstv.MODES[mode].vis and i["parity_ok"] is True and i["rows"] == 2 * PAIRS
    assert abs(i["start"] - sstv.VIS_S * RATE) <= 2 and i["syncs_expected"] == PAIRS and i["syncs_matched"] == PAIRS - 1
    assert abs(i["slant_ppm"]) < 100 and i["empty_pixels"] <= excluded(mode)
    check_errors(images[0], mode, case)


@pytest.mark.parametrize("mode", ["PD50", "PD120"])
def test_slant(mode):
    images, infos = sstv.decode_host(audio_of(mode, "slant"), RATE)
    assert len(images) == 1 and abs(infos[0]["slant_ppm"] - 1000.0) < 100
    assert abs(infos[0]["period"] - sstv.line_time(sstv.MODES[mode]) * RATE * 1.001) < 1.0
    got = check_errors(images[0], mode, "slant")
    clean = MEASURED[(mode, "clean")]
    assert got[0][0] <= 2 * clean[0][0] and got[0][1] <= 2 * clean[0][1]        # the unslanted case's bound


def test_forced_mode_without_header():
    images, infos = sstv.decode_host(audio_of("PD50", "clean", vis=False), RATE, "PD50")
    assert len(images) == 1 and infos[0]["vis"] is None and infos[0]["parity_ok"] is None and infos[0]["syncs_matched"] == PAIRS
    assert abs(infos[0]["start"]) <= 2
    check_errors(images[0], "PD50", "clean")
    assert sstv.decode_host(audio_of("PD50", "clean", vis=False), RATE) == ([], [])


# ------------------------------------------------------------------------------------------------------------------ image count
def test_two_images_noise_and_a_cut_recording():
    a, b = audio_of("PD50", "clean"), audio_of("PD120", "clean", pairs=2)
    images, infos = sstv.decode_host(np.concatenate((a, b)), RATE)
    assert [i["mode"] for i in infos] == ["PD50", "PD120"] and [i["rows"] for i in infos] == [2 * PAIRS, 4]
    assert abs(infos[1]["start"] - (len(a) + sstv.VIS_S * RATE)) <= 2
    check_errors(images[0], "PD50", "clean")
    noise = np.random.default_rng(9).standard_normal(3 * RATE)
    assert sstv.decode_host(noise, RATE) == ([], []) and sstv.decode_host(noise, RATE, "PD120") == ([], [])
    assert sstv.decode_host(np.zeros(0), RATE) == ([], [])
    cut = a[:int(len(a) - 1.5 * sstv.line_time(sstv.MODES["PD50"]) * RATE)]
    images, infos = sstv.decode_host(cut, RATE)
    assert len(images) == 1 and infos[0]["rows"] == 2 * (PAIRS - 2) < sstv.MODES["PD50"].height


def test_rate_limits(caplog):
    with pytest.raises(ValueError, match=r"8000.*1\.520"):
        sstv.decode_host(np.zeros(100), 8000, "PD120")                   # 8000 S/s * 0.19 ms = 1.52 samples
    for rate in (5999.0, 255001.0, float("nan")):
        with pytest.raises(ValueError, match="S/s"):
            sstv.check_rate(rate)
    with pytest.raises(ValueError, match="PD7"):
        sstv.mode_of("PD7")
    # the same mode found in a header: the image is skipped and logged, the decode goes on
    with caplog.at_level(logging.INFO):
        out = sstv.decode_host(audio_of("PD120", "clean", pairs=2, rate=8000), 8000)
    assert out == ([], []) and "below 2" in caplog.text
    assert sstv.tap_count(sstv.RATE_MAX) == sstv.MAX_K and sstv.tap_count(RATE) == 49


# ------------------------------------------------------------------------------------------------------------------ small restatements
def test_runs_host_against_a_plain_loop():
    rng = np.random.default_rng(12)
    for n, W, T in ((40, 5, 3), (200, 16, 9), (64, 1, 1), (30, 30, 10), (29, 30, 1)):
        cls = (rng.uniform(size=n) < 0.6).astype(np.int8) * 2
        cnt = [int((cls[i:i + W] == 2).sum()) for i in range(n - W + 1)]
        want, i = [], 0
        while i < len(cnt):
            if cnt[i] >= T:
                j = i
                while j < len(cnt) and cnt[j] >= T:
                    j += 1
                want.append(i + cnt[i:j].index(max(cnt[i:j])))
                i = j
            else:
                i += 1
        assert list(sstv.runs_host(cls, 2, W, T)) == want, (n, W, T)


def test_iq_recording_through_a_numpy_front_end():
    """the recording of the device's end-to-end test, FM-demodulated by the oracle's restatement of decode_fm's chunk loop: the
    figure that test doubles"""
    from oracle import dd_oracle as O
    raw, fs, offset = iq_recording()
    x = O.grid_c64(raw)
    audio, rate = O.audio_chain(lambda a, b: x[a:b], len(x), fs, float(offset), O.win_blackmanharris(151), 30000, audio_rate=RATE,
                                strict=True)
    assert rate == RATE
    images, infos = sstv.decode_host(audio, rate)
    assert len(images) == 1 and infos[0]["mode"] == "PD50" and infos[0]["rows"] == 2 * PAIRS
    check_errors(images[0], "PD50", "iq")


def iq_recording(fs=240000, offset=12500, dev=3000.0, amp=60.0, sigma=2.0, seed=41):
    """-> (u8 IQ pairs, fs, offset): a VIS header and 4 line pairs of PD50 as FM on a carrier `offset` Hz up, Gaussian noise"""
    y, cr, cb, _ = sent("PD50")
    a = sstv.synth(*sstv.tones(y, cr, cb, "PD50"), fs)
    n = len(a)
    rng = np.random.default_rng(seed)
    ph = 2 * np.pi * dev * np.cumsum(a) / fs + 2 * np.pi * ((offset / fs * np.arange(n)) % 1.0)
    s = amp * np.exp(1j * ph) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    raw = np.empty((n, 2), dtype=np.uint8)
    raw[:, 0] = np.clip(np.round(s.real + 127.5), 0, 255).astype(np.uint8)
    raw[:, 1] = np.clip(np.round(s.imag + 127.5), 0, 255).astype(np.uint8)
    return raw, fs, offset
