#!/usr/bin/env python3
"""
Generate tests/golden/doppler_<case>.npz by running the REFERENCE's sandbox/frequency_shift.py, imported read-only and
unmodified, on the seeded recordings of tests/_doppler.py.  Only data is written: the reference's outputs and the recording's
sha256.  Runs where the reference is (REF below, or DD_REFERENCE); the tests never need it.

Two shims, made before the import (the reference is untouched):
  scipy.fft := scipy.fft.fft       `from scipy import fft` (frequency_shift.py:2) meant the function; today it yields the module
  raw bytes handed over as int16   `-127 + uint8` (:16) was promoted by the NumPy of the reference's day and overflows today

A file holds, per case: the band columns of every waterfall row (float64), a few dozen seeded columns outside the band, the raw
per-row argmax, the smoothed track and correct() at the positions of _doppler.POSITIONS.

For the carrier cases the generator asserts that the relative gap between the best and the second-best band bin is at least
1e-3 in every row (tests/test_gpu_doppler.py relies on it for exact argmax equality).
"""
import importlib.util
import os
import sys
import time

import numpy as np
import scipy
import scipy.fft

REF = os.environ.get("DD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _doppler  # noqa: E402

N_SEEDED = 48
MIN_GAP = 1e-3


def load_reference():
    scipy.fft = scipy.fft.fft
    spec = importlib.util.spec_from_file_location("ref_frequency_shift", os.path.join(REF, "sandbox", "frequency_shift.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case(ref, name):
    raw = _doppler.case(name)
    stream = np.ascontiguousarray(raw).reshape(-1).astype(np.int16)
    fs, window = _doppler.FS, 2048 * 2 * 2
    xf = np.fft.fftshift(np.fft.fftfreq(window, 1.0 / fs))
    df = xf[1] - xf[0]
    every = (len(stream) / (fs * 2.0)) * 8192.0 / window
    with np.errstate(divide="ignore"):
        rows = np.array(ref.make_fft(window, fs, df, every, stream), dtype=np.float64)
        track = np.asarray(ref.find_shift(stream, fs, _doppler.CENTER, _doppler.CHANNEL, _doppler.BANDWIDTH), dtype=np.float64)
    center = (fs / 2 + (_doppler.CHANNEL - _doppler.CENTER)) / df
    band_start = int(center - _doppler.BANDWIDTH / (2 * df))
    band_stop = int(center + _doppler.BANDWIDTH / (2 * df))
    band = rows[:, band_start:band_stop]
    argmax = np.argmax(band, axis=1).astype(np.int32)
    srt = np.sort(band, axis=1)
    gap = 1.0 - np.exp(srt[:, -2] - srt[:, -1])
    rng = np.random.Generator(np.random.PCG64(_doppler.CASES[name]["seed"]))
    outside = np.concatenate((np.arange(0, band_start), np.arange(band_stop, window)))
    cols = np.sort(rng.choice(outside, size=N_SEEDED, replace=False)).astype(np.int32)
    corr = np.array([ref.correct_shift(track, c / k) for c, k in _doppler.POSITIONS], dtype=np.float64)
    with np.errstate(divide="ignore"):
        c, k = _doppler.POSITIONS[2]
        assert ref.correct(stream, fs, _doppler.CENTER, _doppler.CHANNEL, _doppler.BANDWIDTH, c, k) == corr[2]
    print("doppler_%s: %d samples, every %.6f, %d rows, band [%d, %d), min gap %.3g, track %.1f..%.1f Hz" %
          (name, raw.shape[0], every, len(rows), band_start, band_stop, gap.min(), track.min(), track.max()))
    if "baud" not in _doppler.CASES[name]:
        assert gap.min() >= MIN_GAP, "case %s: best/second-best gap %.3g < %g: tune its amplitude or seed" % (name, gap.min(), MIN_GAP)
    np.savez_compressed(os.path.join(OUT, "doppler_%s.npz" % name), sha256=_doppler.sha(raw), every=every, rows=len(rows),
                        band_start=band_start, band_stop=band_stop, band=band, cols=cols, seeded=rows[:, cols], argmax=argmax,
                        track=track, correct=corr, min_gap=gap.min())


def main():
    ref = load_reference()
    for name in (sys.argv[1:] or sorted(_doppler.CASES)):
        t0 = time.time()
        run_case(ref, name)
        print("   %.1f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
