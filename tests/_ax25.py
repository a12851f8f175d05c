"""Test helper: synthetic AX.25 UI frames as AFSK1200 recordings.

frame_bytes -> AX.25 UI frame (addresses with SSIDs, optional digipeater path, control 0x03, PID 0xF0, info, FCS LSB first);
hdlc_bits -> bit stuffing between flags; nrzi -> line levels; afsk_iq -> phase-continuous 1200/2200 Hz AFSK, FM-modulated to
u8 IQ at a given rate and carrier offset.  recording() chains them, with options to corrupt one frame's CRC and to put noise-only
stretches (random line levels) between frames; write_wav() stores the C1 shape (8-bit stereo IQ.wav) through tests/_wav.py.
Deterministic for a seed (numpy PCG64)."""
import numpy as np

C1_NAME = "synth_20180101_120000Z_145825000Hz_IQ.wav"


def _crc16(data):
    fcs = 0xFFFF
    for byte in data:
        for j in range(8):
            bit = (byte >> j) & 1
            s = fcs & 1
            fcs >>= 1
            if s != bit:
                fcs ^= 0x8408
    return fcs ^ 0xFFFF


def _addr(call, ssid, last):
    c = (call.upper() + "      ")[:6]
    return bytes(ord(ch) << 1 for ch in c) + bytes([0x60 | ((ssid & 15) << 1) | (1 if last else 0)])


def frame_bytes(dst, src, info, path=(), control=0x03, pid=0xF0, bad_crc=False):
    """dst / src / path entries: (call, ssid); info: bytes or str (latin-1) -> the frame with its FCS"""
    calls = [dst, src] + list(path)
    body = b"".join(_addr(c, s, k == len(calls) - 1) for k, (c, s) in enumerate(calls))
    body += bytes([control, pid]) + (info.encode("latin-1") if isinstance(info, str) else bytes(info))
    fcs = _crc16(body) ^ (0x0101 if bad_crc else 0)
    return body + bytes([fcs & 0xFF, fcs >> 8])


def hdlc_bits(frame, n_flags_after=2):
    """bytes LSB first, a 0 stuffed after five ones, then flags"""
    out, run = [], 0
    for byte in frame:
        for j in range(8):
            b = (byte >> j) & 1
            out.append(b)
            run = run + 1 if b else 0
            if run == 5:
                out.append(0)
                run = 0
    return out + [0, 1, 1, 1, 1, 1, 1, 0] * n_flags_after


def nrzi(bits, level=1):
    """a 0 toggles the line, a 1 keeps it"""
    out = []
    for b in bits:
        if b == 0:
            level ^= 1
        out.append(level)
    return out


def afsk_iq(levels, fs, seed, baud=1200, mark=1200, space=2200, dev=3000.0, amp=60.0, sigma=2.0, f_carrier=0.0):
    """line levels (1 mark, 0 space) -> phase-continuous AFSK -> FM -> u8 IQ pairs at fs"""
    rng = np.random.default_rng(seed)
    levels = np.asarray(levels)
    spb = fs / baud
    n = int(len(levels) * spb)
    t = np.arange(n)
    tone = np.where(levels[np.minimum((t / spb).astype(np.int64), len(levels) - 1)] == 1, mark, space).astype(np.float64)
    audio = np.cos(2 * np.pi * np.cumsum(tone) / fs)
    ph = 2 * np.pi * dev * np.cumsum(audio) / fs
    if f_carrier:
        ph = ph + 2 * np.pi * ((f_carrier / fs * t) % 1.0)
    s = amp * np.exp(1j * ph) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    raw = np.empty((n, 2), dtype=np.uint8)
    raw[:, 0] = np.clip(np.round(s.real + 127.5), 0, 255).astype(np.uint8)
    raw[:, 1] = np.clip(np.round(s.imag + 127.5), 0, 255).astype(np.uint8)
    return raw


def recording(frames, fs, seed, lead_flags=30, bad=(), noise_bits=(), f_carrier=0.0, tail_bits=64):
    """frames: list of (dst, src, info, path); bad: indices whose CRC is corrupted; noise_bits[i]: random line levels after frame i.
    Returns (raw u8 IQ, the frames' bytes)."""
    rng = np.random.default_rng(seed + 1000)
    bits = [0, 1, 1, 1, 1, 1, 1, 0] * lead_flags
    fb = []
    for i, (dst, src, info, path) in enumerate(frames):
        f = frame_bytes(dst, src, info, path, bad_crc=i in bad)
        fb.append(f)
        bits += hdlc_bits(f)
        if i < len(noise_bits) and noise_bits[i]:
            bits += rng.integers(0, 2, int(noise_bits[i])).tolist() + [0, 1, 1, 1, 1, 1, 1, 0] * 4
    levels = nrzi(bits) + [1] * tail_bits
    return afsk_iq(levels, fs, seed, f_carrier=f_carrier), fb


def write_wav(path, raw, fs):
    from _wav import write_iq_wav
    write_iq_wav(path, raw, fs)


# ---------------------------------------------------------------- the recordings behind tests/golden/afsk_frames_*.npz
INFO = "!4903.50N/07201.75W-Test k"


def fixture_a():
    """882 kS/s at the centre: four frames, the third with a corrupted CRC -> (raw, fs, offset, frame bytes)"""
    fs = 882000
    frames = [(("APRS", 0), ("N0CALL", 7), INFO, ()),
              (("APZ001", 0), ("DL1ABC", 9), "=5230.00N/01320.00E>first", (("WIDE1", 1),)),
              (("APRS", 0), ("K1XYZ", 0), INFO + " bad", ()),
              (("CQ", 0), ("VK2ZZ", 15), ">status text " + "x" * 20, (("WIDE1", 1), ("WIDE2", 2)))]
    raw, fb = recording(frames, fs, 21, lead_flags=30, bad=(2,), noise_bits=(0, 40))
    return raw, fs, 0, fb


def fixture_b():
    """config 1's shape: 2.4 MS/s, the signal 10 kHz above the centre the file name carries -> (raw, fs, offset, frame bytes)"""
    fs, offset = 2400000, 10000
    frames = [(("APRS", 0), ("N0CALL", 7), INFO, ()),
              (("APRS", 0), ("W1AW", 2), "!4140.00N/07240.00W#digi", (("WIDE2", 2),))]
    raw, fb = recording(frames, fs, 22, lead_flags=20, f_carrier=float(offset))
    return raw, fs, offset, fb


# ---------------------------------------------------------------- host restatements the tests compare the device against
def peakdetect_host(y, lookahead, delta=0.0):
    """the billauer lookahead machine of peakdetect.peakdetect, restated: -> (max [(i, v)], min [(i, v)]) after the pop"""
    y = np.asarray(y, dtype=np.float64)
    n, L = len(y), int(lookahead)
    inf = np.inf
    mx, mn, mxpos, mnpos = -inf, inf, -1, -1
    mxs, mns, first = [], [], None
    for i in range(max(n - L, 0)):
        v = y[i]
        if v > mx:
            mx, mxpos = v, i
        if v < mn:
            mn, mnpos = v, i
        if v < mx - delta and mx != inf and y[i:i + L].max() < mx:
            mxs.append((mxpos, mx))
            first = "max" if first is None else first
            mx = mn = inf
            continue
        if v > mn + delta and mn != -inf and y[i:i + L].min() > mn:
            mns.append((mnpos, mn))
            first = "min" if first is None else first
            mn = mx = -inf
    if first == "max":
        mxs.pop(0)
    elif first == "min":
        mns.pop(0)
    return mxs, mns


def np_mean_model(x):
    """np.mean of a contiguous float64 slice of at most 128 elements, in NumPy's own summation order"""
    n = len(x)
    if n == 0:
        return np.nan
    if n < 8:
        r = 0.0
        for v in x:
            r += v
        return r / n
    r = [float(x[j]) for j in range(8)]
    i = 8
    while i < n - (n % 8):
        for j in range(8):
            r[j] += x[i + j]
        i += 8
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for k in range(i, n):
        s += x[k]
    return s / n


def bits_host(bf, peaks, bw):
    """decode_afsk1200.py:189-229 restated: -> (means, bits, marks, flags)"""
    spb = bw // 1200
    px = np.asarray(peaks, dtype=np.int64)
    rep = np.round(np.diff(px) / (bw / 1200))
    means = []
    for i in range(len(rep)):
        for r in range(int(rep[i])):
            means.append(np.mean(bf[px[i] + r * spb: px[i] + (r + 1) * spb]) if px[i] + r * spb < len(bf) else np.nan)
    s = np.sign(np.array(means, dtype=np.float64))
    bits = [1] + [1 if s[k - 1] == s[k] else 0 for k in range(1, len(s))] if len(s) else []
    b = np.array(bits, dtype=np.int8)
    flags = [k for k in range(len(b) - 8) if tuple(b[k:k + 8]) == (0, 1, 1, 1, 1, 1, 1, 0)]
    marks = np.zeros(len(b), dtype=np.int8)
    run = 0
    for k in range(len(b)):
        if run == 5:
            marks[k] = 2 if b[k] == 1 else 1
        run = run + 1 if b[k] == 1 else 0
    return np.array(means, dtype=np.float64), b, marks, np.array(flags, dtype=np.int64)


def frames_host(bits, marks, flags):
    """decode_afsk1200.py:236-269 restated: -> (info[npairs, 2] = (unstuffed count, accepted), [message bytes of accepted pairs])"""
    info, out = [], []
    for f in range(len(flags) - 1):
        a, b = flags[f] + 8, flags[f + 1]
        seg = [int(x) for x, m in zip(bits[a:b], marks[a:b]) if m == 0]
        msg = seg[:-16]
        ok = len(seg) % 8 == 0 and len(msg) > 128
        if ok:
            fcs = 0xFFFF
            for x in msg:
                s = fcs & 1
                fcs >>= 1
                if s != x:
                    fcs ^= 0x8408
            fcs ^= 0xFFFF
            ok = all(((fcs >> j) & 1) == seg[len(msg) + j] for j in range(16))
        info.append((len(seg), int(ok)))
        if ok:
            out.append(bytes(sum(msg[k + j] << j for j in range(8)) for k in range(0, len(msg), 8)))
    return np.array(info, dtype=np.int64).reshape(-1, 2), out
