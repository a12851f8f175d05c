"""
CPU checks of the APT image decoder's surface and host logic (directdemod_amd.decode_noaa): the class imports without a GPU
and has the reference's property surface; the sync filling and the telemetry state machine reproduce the reference's results
stored in tests/golden/apt_image_*.npz (tools/gen_golden.py --apt-image).
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gold(name):
    return np.load(os.path.join(GOLD, name))


def test_decode_noaa_surface():
    import directdemod_amd
    from directdemod_amd import decode_noaa, noaa_sync
    assert "decode_noaa" in directdemod_amd.__all__
    cls = decode_noaa.decode_noaa
    assert issubclass(cls, noaa_sync.noaa_sync)
    for name in ("getImage", "getImageA", "getImageB", "channelID", "getColor", "getAudio", "useful"):
        assert isinstance(getattr(cls, name), property), name
    for name in ("getCrudeSync", "getAccurateSync", "getMapImage"):
        assert callable(getattr(cls, name)), name


def test_fill_sync_matches_golden():
    from directdemod_amd import decode_noaa as dn
    g = _gold("apt_image_plain.npz")
    rate, n = int(g["rate"]), int(g["n_env"])
    for key, crude in (("fill_syncA", g["crude_syncA"]), ("fill_syncB", g["crude_syncB"])):
        got = np.asarray(dn.fill_sync(dn.to_rate(crude, rate, rate), n), dtype=np.float64)
        assert np.array_equal(got, g[key]), key


def test_calibration_state_machine_matches_golden():
    from directdemod_amd import decode_noaa as dn
    g = _gold("apt_image_telemetry.npz")
    params, low, high, slope, intercept, ch = dn.calibrate(g["low0"], g["high0"], g["line_strip_a"], g["line_strip_b"],
                                                          g["line_sync_low"], g["line_sync_high"], g["line_use"])
    assert slope is not None and intercept is not None
    assert abs(slope - g["slope"]) <= 1e-9 * abs(g["slope"])
    assert abs(intercept - g["intercept"]) <= 1e-9 * max(1.0, abs(g["intercept"]))
    assert ch == [int(v) for v in g["channel_id"]]
    assert len(params) == len(g["line_strip_a"]) and all(p[0] == 1.0 for p in params)


def test_calibration_without_telemetry_keeps_bounds():
    from directdemod_amd import decode_noaa as dn
    n = 12
    strip = np.full(n, 0.5)
    params, low, high, slope, intercept, ch = dn.calibrate(0.1, 0.9, strip, strip, np.full(n, 0.2), np.full(n, 0.8),
                                                          np.zeros(n, dtype=bool))
    assert slope is None and ch == [None, None]
    assert params == [(0.0, 0.1, 0.9)] * n and (low, high) == (0.1, 0.9)


def test_slice_bounds_follow_python_slices():
    from directdemod_amd import decode_noaa as dn
    x = np.arange(1000)
    for a, b in ((-579, 0), (-479, 100), (100, 679), (421, 1000), (999, 1200), (0, 0)):
        s, n = dn.slice_bounds(a, b, len(x))
        assert np.array_equal(x[a:b], x[s:s + n]), (a, b)
