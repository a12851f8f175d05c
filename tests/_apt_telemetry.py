"""
Synthetic NOAA APT recording with telemetry wedges (test helper, shared by tools/gen_golden.py --apt-image and the tests).

Same signal model as the oracle's synth_apt_iq (2 lines/s of 2 080 words at 4 160 words/s, sync A at words 0-39 and sync B at
1040-1079 mapped (bit * 233 + 11) / 255, AM on a 2 400 Hz subcarrier, FM at +f_offset, u8 grid), but with a smooth image and the
telemetry columns filled: words 1000-1039 (before sync B: channel A's telemetry) and 2040-2079 (before the next sync A: channel
B's).  A telemetry frame is 16 wedges of 8 lines; wedges 1-8 rise in steps of 1/8 of full scale, wedge 9 is zero, wedge 16
carries the channel ID as id/8 (and so does wedge 15 here).  The recording starts in wedge 15, so that the decoder sees wedge 16, the staircase 1-8 and
the drop to wedge 9 -- what its calibration state machine needs -- within WEDGE_LINES * 11 lines.
"""
import math

import numpy as np

NOAA_SYNCA = [0, 0, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0,
              1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
NOAA_SYNCB = [0, 0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 1,
              1, 1, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0]
WEDGE_LINES = 8
CHANNEL_A, CHANNEL_B = 2, 1          # channel B's ID wedge must sit within 1/16 of full scale of wedge 1 (the state machine's entry)


def wedge_value(wedge, channel_id):
    """full-scale fraction of telemetry wedge 1..16"""
    if 1 <= wedge <= 8:
        return wedge / 8.0
    if wedge == 9:
        return 0.0
    if wedge >= 15:                 # 15 (back scan) held at the ID wedge's level: no step before wedge 1 but the staircase's
        return channel_id / 8.0
    return 0.3 + 0.02 * (wedge - 10)        # 10-14: temperatures, anything


def telemetry_words(duration_s, first_wedge=15, lead_lines=6):
    """word values of the whole recording (float64, one per word)"""
    nwords = int(math.ceil(duration_s * 4160)) + 1
    nlines = nwords // 2080 + 1
    w = np.arange(2080, dtype=np.float64)
    words = np.empty(nlines * 2080)
    for ln in range(nlines):
        row = 0.5 + 0.3 * np.sin(2 * np.pi * (w / 1040.0 + ln / 60.0))           # smooth image content
        row[:40] = (np.array(NOAA_SYNCA) * 233 + 11) / 255.0
        row[1040:1080] = (np.array(NOAA_SYNCB) * 233 + 11) / 255.0
        # wedge index of this line: `lead_lines` lines of first_wedge, then 8 lines per wedge
        k = 0 if ln < lead_lines else 1 + (ln - lead_lines) // WEDGE_LINES
        wedge = (first_wedge - 1 + k) % 16 + 1
        row[1000:1040] = wedge_value(wedge, CHANNEL_A)
        row[2040:2080] = wedge_value(wedge, CHANNEL_B)
        words[ln * 2080:(ln + 1) * 2080] = row
    return words[:nwords]


def synth_apt_telemetry_iq(duration_s, fs=2048000, seed=3, f_offset=30000.0, dev=17000.0, amp=60.0, sigma=2.0):
    """u8[N, 2] IQ of the telemetry recording (the oracle's synth_apt_iq model with telemetry_words)"""
    rng = np.random.default_rng(seed)
    n = int(duration_s * fs)
    words = telemetry_words(duration_s)
    nwords = len(words)
    out = np.empty((n, 2), dtype=np.uint8)
    blk = 1 << 20
    phase = 0.0
    for s0 in range(0, n, blk):
        s1 = min(n, s0 + blk)
        idx = np.arange(s0, s1)
        t = idx / fs
        env = words[np.minimum((idx * 4160) // fs, nwords - 1)]
        audio = env * np.sin(2 * np.pi * 2400.0 * t)
        ph = phase + 2 * np.pi * dev * np.cumsum(audio) / fs
        phase = ph[-1]
        s = amp * np.exp(1j * (2 * np.pi * f_offset * t + ph))
        s = s + sigma * (rng.standard_normal(s1 - s0) + 1j * rng.standard_normal(s1 - s0))
        out[s0:s1, 0] = np.clip(np.round(s.real + 127.5), 0, 255).astype(np.uint8)
        out[s0:s1, 1] = np.clip(np.round(s.imag + 127.5), 0, 255).astype(np.uint8)
    return out
