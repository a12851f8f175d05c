"""
AIS: 9600 baud GMSK bursts that carry HDLC frames (beyond the reference; DESIGN.md section 4.23 defines every stage; device side:
dd_ais.h): the constants, a NumPy restatement `candidates_host` / `demod_host` of the two kernels, the device wrappers over the C
entries, `decode`, the chain behind decode_ais, which runs over either set of stages (`DeviceOps`, `HostOps`) so that the host logic
is one piece of code for both, the burst merge, the CRC, the six-bit NMEA armour and the !AIVDM sentences, the field parser, and
`encode` / `encode_audio`, a synthesiser.

The audio is the FM discriminator's output in radians per sample.  q = rint(audio * (2^20 / pi)) makes integers of it; everything
behind the quantiser is integer.  Bit k of the start t is read around sample floor(t + (k + 0.5) sps): v(t, k) is the sum of the w
samples q around it, samples outside the audio counting 0.

The format is taken from public descriptions of AIS (ITU-R M.1371, the AIVDM sentence descriptions); INTEGRATION.md lists the limits.
"""
import math

import numpy as np

from . import _burst
from ._burst import Laps, need
from ._hip import DevArray, check, lib

BAUD = 9600
SPS_MIN, SPS_MAX = 4.0, 16.0
W_MAX = 15
SLACK_MAX = 11
TEMPLATE = 24                         # bits of the template: the last 16 training bits and the start flag
TRAINING = 16                         # of which S sums the first
RAW_BITS = 1280                       # raw bits behind the start flag that dd_ais_demod reads
FRAME_BYTES = 160
TILE = 256                            # DD_AIS_TILE
SCALE = 1048576.0 / math.pi           # DD_FM_SCALE (dd_candidates.h)
CLIP = 2097152.0
PLUS = np.array([(0x80CCCC >> k) & 1 for k in range(TEMPLATE)], dtype=bool)      # (- - + +) x 4, seven -, one +
OK, NO_END, ABORT, STUFFING, LENGTH, CRC = range(6)
STATUS = ("accepted", "no_end_flag", "abort", "stuffing_violation", "bad_length", "bad_crc")
MERGE_BITS = 8                        # accepted candidates with the same bytes within this many bit times are one burst
GOOD = 0xF0B8
FLAG = (0, 1, 1, 1, 1, 1, 1, 0)
BT, DEVIATION = 0.4, 2400.0           # the Gaussian pulse; h = 0.5 at 9600 baud
CUT = 7000.0                          # the audio-rate channel filter's cut-off, Hz

_F64 = np.dtype(np.float64)


def params(rate, w=None, slack=0):
    """(sps, w, slack) for an audio rate: sps = rate / 9600 must lie in 4 .. 16; w None: the odd number nearest 0.6 sps"""
    sps = float(rate) / BAUD
    if not SPS_MIN <= sps <= SPS_MAX:              # (also false for a NaN)
        raise ValueError("ais: an audio rate of %r S/s at %d baud is %r samples per bit; %g to %g are supported (%g to %g S/s)"
                         % (rate, BAUD, sps, SPS_MIN, SPS_MAX, SPS_MIN * BAUD, SPS_MAX * BAUD))
    if w is None:
        w = 2 * int(math.floor((0.6 * sps - 1.0) / 2.0 + 0.5)) + 1
    if int(w) != w or not 1 <= w <= W_MAX or not int(w) & 1:
        raise ValueError("ais: w must be an odd number from 1 to %d, got %r" % (W_MAX, w))
    if int(slack) != slack or not 0 <= slack <= SLACK_MAX:
        raise ValueError("ais: slack must be from 0 to %d, got %r" % (SLACK_MAX, slack))
    return sps, int(w), int(slack)


def reach(sps, w):
    """samples from a start to past the last one its template reads"""
    return int(math.floor(23.5 * sps)) + w // 2 + 1


def n_starts(n, sps, w):
    return max(0, int(n) - reach(sps, w) + 1)


# ------------------------------------------------------------------------------------------------------------------ the CRC
def _ztable():
    z = np.zeros(RAW_BITS, dtype=np.int64)
    v = 0x8408
    for m in range(RAW_BITS):
        z[m] = v
        v = (v >> 1) ^ 0x8408 if v & 1 else v >> 1
    return z


ZTABLE = _ztable()                    # the register m zero bits after a lone one bit entered an empty register


def crc_register(bits):
    """The CRC-16 register (reflected 0x8408, preset 0xFFFF, nothing inverted at the end) after the bits, first sent first: GOOD
    after a frame with its FCS.  From 16 bits up by the kernel's route, the XOR of lone-bit remainders with the first 16 bits
    inverted for the preset; below that bit by bit."""
    b = np.asarray(bits, dtype=np.int64).reshape(-1)
    n = len(b)
    if 16 <= n <= RAW_BITS:
        c = b.copy()
        c[:16] ^= 1
        return int(np.bitwise_xor.reduce(ZTABLE[n - 1 - np.flatnonzero(c)])) if c.any() else 0
    reg = 0xFFFF
    for bit in b:
        low = (reg ^ int(bit)) & 1
        reg >>= 1
        if low:
            reg ^= 0x8408
    return reg


def crc(data):
    """the FCS of the bytes: the inverted register, sent low byte first, each byte lowest bit first"""
    return crc_register(np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8), bitorder="little")) ^ 0xFFFF


def stuff(bits):
    """a 0 behind every five 1s"""
    out, run = [], 0
    for b in bits:
        out.append(int(b))
        run = run + 1 if b else 0
        if run == 5:
            out.append(0)
            run = 0
    return np.array(out, dtype=np.uint8)


def destuff(bits):
    """the bits less every 0 that follows five 1s (a sixth 1 stays: a flag or an abort, which the caller looks for)"""
    b = np.asarray(bits, dtype=bool)
    five = np.ones(len(b), dtype=bool)
    for s in range(1, 6):
        five &= np.concatenate((np.zeros(s, dtype=bool), b[:len(b) - s]))[:len(b)]
    return b[~(~b & five)].astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def quantise(audio):
    """q = rint(audio * SCALE) as int64; 0 for a NaN and beyond +-2^21"""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(audio, dtype=np.float64) * SCALE)
        return np.where((r >= -CLIP) & (r <= CLIP), r, 0.0).astype(np.int64)


def positions(ts, ks, sps):
    """int64[len(ts), len(ks)]: floor(t + (k + 0.5) sps), the product and the sum each rounded to float64"""
    t = np.asarray(ts, dtype=np.int64).astype(np.float64).reshape(-1, 1)
    k = np.asarray(ks, dtype=np.int64).astype(np.float64).reshape(1, -1)
    return np.floor(t + (k + 0.5) * sps).astype(np.int64)


def values(q, ts, ks, sps, w):
    """v(t, k) for every t of ts and k of ks, int64"""
    n, h = len(q), w // 2
    cum = np.concatenate((np.zeros(1, dtype=np.int64), np.cumsum(np.asarray(q, dtype=np.int64))))
    at = positions(ts, ks, sps)
    return cum[np.clip(at + h + 1, 0, n)] - cum[np.clip(at - h, 0, n)]


def template_of(q, ts, sps, w):
    """(levels bool[m, 24], S int64[m], score int64[m]) of the starts ts"""
    v = values(q, ts, np.arange(TEMPLATE), sps, w)
    S = v[:, :TRAINING].sum(axis=1)
    return 16 * v > S.reshape(-1, 1), S, np.abs(16 * v - S.reshape(-1, 1)).sum(axis=1)


def masks_host(audio, sps, w, slack=0, block=1 << 16):
    """the mask byte of every start: bit 0 pass, bit 1 the negated template; uint8[n_starts]"""
    q = quantise(audio)
    total = n_starts(len(q), sps, w)
    out = np.zeros(total, dtype=np.uint8)
    for a in range(0, total, block):
        ts = np.arange(a, min(total, a + block), dtype=np.int64)
        mis = (template_of(q, ts, sps, w)[0] != PLUS.reshape(1, -1)).sum(axis=1)
        out[a:a + len(ts)] = np.where(mis <= slack, 1, np.where(TEMPLATE - mis <= slack, 3, 0))
    return out


def candidates_host(audio, sps, w, slack=0):
    """the ordered starts that pass the preamble test, int64"""
    return np.flatnonzero(masks_host(audio, sps, w, slack) & 1).astype(np.int64)


def _empty_det(m=0):
    return {"t": np.zeros(m, np.int64), "frames": np.zeros((m, FRAME_BYTES), np.uint8), "status": np.full(m, NO_END, np.int32),
            "nbits": np.zeros(m, np.int32), "rem": np.zeros(m, np.int32), "polarity": np.zeros(m, np.int32),
            "score": np.zeros(m, np.int64)}


def demod_host(audio, sps, w, ts):
    """the listed starts' frames: a dict of t, frames uint8[m, 160] (zero beyond nbits), status, nbits, rem, polarity, score"""
    q = quantise(audio)
    n = len(q)
    ts = np.asarray(ts, dtype=np.int64).reshape(-1)
    det = _empty_det(len(ts))
    det["t"] = ts
    for c, t in enumerate(ts):
        if t < 0 or t >= n:
            continue
        lev, S, score = template_of(q, [t], sps, w)
        det["score"][c] = score[0]
        det["polarity"][c] = int((lev[0] != PLUS).sum() > TEMPLATE // 2)
        raw = 16 * values(q, [t], TEMPLATE + np.arange(RAW_BITS), sps, w)[0] > S[0]
        b = np.concatenate((lev[0, -1:], raw[:-1])) == raw                    # NRZI: 1 where the level repeats
        bp = np.concatenate((b, np.zeros(6, dtype=bool)))
        six = np.ones(RAW_BITS, dtype=bool)
        for s in range(6):
            six &= bp[s:s + RAW_BITS]
        if not six.any() or int(np.argmax(six)) + 6 >= RAW_BITS:
            continue                                                          # (NO_END)
        e = int(np.argmax(six))
        if b[e + 6]:
            det["status"][c] = ABORT
            continue
        status = STUFFING if e >= 6 and b[e - 6:e - 1].all() else OK
        kept = destuff(b[:max(e - 1, 0)])
        nbits = len(kept)
        if status == OK and (nbits < 40 or nbits % 8):
            status = LENGTH
        if status == OK:
            det["rem"][c] = crc_register(kept)
            if det["rem"][c] != GOOD:
                status = CRC
        packed = np.packbits(kept, bitorder="little")
        det["frames"][c, :len(packed)] = packed
        det["status"][c], det["nbits"][c] = status, nbits
    return det


# ------------------------------------------------------------------------------------------------------------------ the device stages
def candidates(audio, sps, w, slack=0, cap=None):
    """float64 device audio -> (the survivors as a device int64 array, how many) (dd_ais_candidates); a list that proves too small
    is asked for again at the true count"""
    need(audio, _F64, "ais.candidates")
    cap = 1024 + audio.n // 1024 if cap is None else int(cap)
    def call(lst, cap, count):
        return lib().dd_ais_candidates(audio.ptr, audio.n, float(sps), int(w), int(slack), lst, cap, count, None)
    return _burst.candidates("dd_ais_candidates", cap, call)


def demod(audio, sps, w, lst, m):
    """the first m starts of the device list -> the dict of demod_host, on the host (dd_ais_demod)"""
    need(audio, _F64, "ais.demod")
    if not isinstance(lst, DevArray):
        lst = DevArray.from_host(np.ascontiguousarray(lst, dtype=np.int64))
    det = _empty_det(m)
    if m == 0 or audio.n == 0:
        return det
    frames, meta, score = DevArray(FRAME_BYTES * m, np.uint8), DevArray(4 * m, np.int32), DevArray(m, np.int64)
    check(lib().dd_ais_demod(audio.ptr, audio.n, float(sps), int(w), lst.ptr, m, frames.ptr, meta.ptr, score.ptr, None), "dd_ais_demod")
    meta = meta.to_host().reshape(m, 4)
    det.update(t=lst.view(0, m).to_host(), frames=frames.to_host().reshape(m, FRAME_BYTES), status=meta[:, 0].copy(),
               nbits=meta[:, 1].copy(), rem=meta[:, 2].copy(), polarity=meta[:, 3].copy(), score=score.to_host())
    return det


class HostOps(Laps):
    """the stages of `decode` in NumPy"""

    def detect(self, audio, sps, w, slack):
        ts = candidates_host(audio, sps, w, slack)
        return demod_host(audio, sps, w, ts)


class DeviceOps(Laps):
    """the stages of `decode` on the device; `laps` collects seconds per stage, with a synchronisation after each"""

    def detect(self, audio, sps, w, slack):
        lst, m = candidates(audio, sps, w, slack)
        self.lap("candidates")
        det = demod(audio, sps, w, lst, m)
        self.lap("demod")
        return det


# ------------------------------------------------------------------------------------------------------------------ the host logic
def merge(det, sps):
    """The accepted candidates of one channel -> (the kept indices in time order, how many duplicates were dropped): candidates with
    the same bytes whose starts lie within MERGE_BITS bit times of the group's first are one burst; the largest score stays, the
    earliest on a tie."""
    acc = [int(i) for i in np.flatnonzero(det["status"] == OK)]
    acc.sort(key=lambda i: (int(det["t"][i]), i))
    keep, dup = [], 0
    used = [False] * len(acc)
    for a, i in enumerate(acc):
        if used[a]:
            continue
        group = [i]
        for b in range(a + 1, len(acc)):
            j = acc[b]
            if det["t"][j] - det["t"][i] > MERGE_BITS * sps:
                break
            if not used[b] and det["nbits"][j] == det["nbits"][i] and np.array_equal(det["frames"][j], det["frames"][i]):
                used[b] = True
                group.append(j)
        keep.append(min(group, key=lambda j: (-int(det["score"][j]), int(det["t"][j]))))
        dup += len(group) - 1
    return keep, dup


def decode(audios, rate, channels, slack=0, w=None, ops=None):
    """The chain behind decode_ais over one audio per channel (float64 device arrays for DeviceOps, NumPy for HostOps) at `rate`
    S/s -> (messages in time order, frameInfo, the candidates' dict per channel)."""
    ops = HostOps() if ops is None else ops
    sps, w, slack = params(rate, w, slack)
    msgs, cands = [], {}
    info = {"samples": 0, "candidates": 0, "accepted": 0, "duplicates": 0}
    info.update({name: 0 for name in STATUS[1:]})
    for ch, audio in zip(channels, audios):
        det = ops.detect(audio, sps, w, slack)
        cands[ch] = det
        keep, dup = merge(det, sps)
        info["samples"] = max(info["samples"], len(audio))
        info["candidates"] += len(det["t"])
        info["accepted"] += len(keep)
        info["duplicates"] += dup
        for s in range(1, len(STATUS)):
            info[STATUS[s]] += int(np.count_nonzero(det["status"] == s))
        for i in keep:
            nbytes = int(det["nbits"][i]) // 8
            raw = bytes(det["frames"][i][:nbytes - 2])                        # (without the FCS)
            t = int(det["t"][i])
            start = int(math.floor(t + TRAINING * sps))
            m = {"t": start / float(rate), "start": start, "channel": ch, "nbits": 8 * len(raw), "raw": raw,
                 "score": int(det["score"][i])}
            m.update(parse(raw))
            msgs.append(m)
        ops.lap("host")
    msgs.sort(key=lambda m: (m["start"], m["channel"]))
    seq = 0
    for m in msgs:                                                            # sentences: a sequence id per multi-sentence message
        bits = np.unpackbits(np.frombuffer(m["raw"], dtype=np.uint8))
        many = -(-len(bits) // 6) > 60
        m["nmea"] = nmea(bits, m["channel"], seq % 10 if many else None)
        seq += 1 if many else 0
    return msgs, info, cands


def vessels(msgs):
    """messages in time order -> {mmsi: {shipname, callsign, shiptype, destination, track}}: track is a list of
    (t, lat, lon, sog, cog) from the position reports whose position is given"""
    out = {}
    for m in msgs:
        v = out.setdefault(m["mmsi"], {"shipname": None, "callsign": None, "shiptype": None, "destination": None, "track": []})
        for key in ("shipname", "callsign", "shiptype", "destination"):
            if m.get(key) is not None:
                v[key] = m[key]
        if m.get("lat") is not None and m.get("lon") is not None:
            v["track"].append((m["t"], m["lat"], m["lon"], m.get("sog"), m.get("cog")))
    return out


# ------------------------------------------------------------------------------------------------------------------ sentences
def armor(bits):
    """(payload characters, fill bits): six bits per character, most significant first, zero filled at the end"""
    b = np.asarray(bits, dtype=np.uint8).reshape(-1)
    fill = -len(b) % 6
    v = np.concatenate((b, np.zeros(fill, dtype=np.uint8))).reshape(-1, 6) @ np.array([32, 16, 8, 4, 2, 1])
    return "".join(chr(x + 48) if x < 40 else chr(x + 56) for x in v.tolist()), fill


def dearmor(payload, fill=0):
    """payload characters -> bits (uint8), the last `fill` dropped"""
    vals = []
    for ch in payload:
        x = ord(ch) - 48
        if not (0 <= x < 40 or 48 <= x < 72):                     # '0' .. 'W' and '`' .. 'w'
            raise ValueError("ais.dearmor: %r is no payload character" % ch)
        vals.append(x if x < 40 else x - 8)
    b = ((np.array(vals, dtype=np.int64).reshape(-1, 1) >> np.arange(5, -1, -1)) & 1).astype(np.uint8).reshape(-1)
    return b[:len(b) - fill] if fill else b


def checksum(body):
    """the XOR of the characters, two hex digits"""
    c = 0
    for ch in body:
        c ^= ord(ch)
    return "%02X" % c


def nmea(payload_bits, channel, seq=None, width=60):
    """!AIVDM sentences of at most `width` payload characters (60; some receivers cut at 56); `seq` is the sequence id of a
    multi-sentence message"""
    payload, fill = armor(payload_bits)
    parts = [payload[a:a + width] for a in range(0, max(len(payload), 1), width)]
    out = []
    for i, part in enumerate(parts):
        body = "AIVDM,%d,%d,%s,%s,%s,%d" % (len(parts), i + 1, "" if len(parts) == 1 or seq is None else seq, channel, part,
                                            fill if i == len(parts) - 1 else 0)
        out.append("!%s*%s" % (body, checksum(body)))
    return out


def from_nmea(sentences):
    """the sentences of ONE message -> (payload bits, channel); ValueError on a bad checksum or a part out of order"""
    bits, channel = [], None
    for i, s in enumerate(sentences):
        body, _, cs = s.strip().lstrip("!").partition("*")
        if checksum(body) != cs.upper():
            raise ValueError("ais.from_nmea: checksum of %r" % s)
        f = body.split(",")
        if f[0] != "AIVDM" or int(f[1]) != len(sentences) or int(f[2]) != i + 1:
            raise ValueError("ais.from_nmea: %r is not part %d of %d" % (s, i + 1, len(sentences)))
        channel = f[4]
        bits.append(dearmor(f[5], int(f[6])))
    return np.concatenate(bits), channel


# ------------------------------------------------------------------------------------------------------------------ the fields
def _u(bits, first, count):
    v = 0
    for b in bits[first:first + count]:
        v = (v << 1) | int(b)
    return v


def _s(bits, first, count):
    v = _u(bits, first, count)
    return v - (1 << count) if v >> (count - 1) else v


def _text(bits, first, count):
    """six-bit text; trailing @ and spaces stripped"""
    out = []
    for a in range(first, first + count, 6):
        v = _u(bits, a, 6)
        out.append(chr(v + 64) if v < 32 else chr(v))
    return "".join(out).rstrip("@ ")


def _position(bits, first):
    """(lon, lat) of a 28 and a 27 bit field in 1/10000 minute; 181 and 91 degrees mean none"""
    lon, lat = _s(bits, first, 28) / 600000.0, _s(bits, first + 28, 27) / 600000.0
    return (None if lon == 181.0 else lon), (None if lat == 91.0 else lat)


def _speed(bits, first):
    v = _u(bits, first, 10)
    return None if v == 1023 else v / 10.0


def _course(bits, first):
    v = _u(bits, first, 12)
    return None if v == 3600 else v / 10.0


def _heading(bits, first):
    v = _u(bits, first, 9)
    return None if v == 511 else v


def _dimensions(bits, first, out):
    out["to_bow"], out["to_stern"] = _u(bits, first, 9), _u(bits, first + 9, 9)
    out["to_port"], out["to_starboard"] = _u(bits, first + 18, 6), _u(bits, first + 24, 6)


def parse(message):
    """The fields of a message (bytes, or an array of its bits, most significant first): type, repeat, mmsi and, by type, the
    fields of DESIGN.md section 4.23's table; a message shorter than its type's table, and every other type, has those three only."""
    if isinstance(message, (bytes, bytearray)):
        bits = np.unpackbits(np.frombuffer(bytes(message), dtype=np.uint8))
    else:
        bits = np.asarray(message, dtype=np.uint8).reshape(-1)
    n = len(bits)
    out = {"type": _u(bits, 0, 6), "repeat": _u(bits, 6, 2), "mmsi": _u(bits, 8, 30)}
    ty = out["type"]
    if ty in (1, 2, 3) and n >= 168:
        out["status"], out["rot"], out["sog"], out["accuracy"] = _u(bits, 38, 4), _s(bits, 42, 8), _speed(bits, 50), _u(bits, 60, 1)
        out["lon"], out["lat"] = _position(bits, 61)
        out["cog"], out["heading"], out["second"] = _course(bits, 116), _heading(bits, 128), _u(bits, 137, 6)
        out["raim"], out["radio"] = _u(bits, 148, 1), _u(bits, 149, 19)
    elif ty == 4 and n >= 168:
        out["year"], out["month"], out["day"] = _u(bits, 38, 14), _u(bits, 52, 4), _u(bits, 56, 5)
        out["hour"], out["minute"], out["second"] = _u(bits, 61, 5), _u(bits, 66, 6), _u(bits, 72, 6)
        out["accuracy"] = _u(bits, 78, 1)
        out["lon"], out["lat"] = _position(bits, 79)
        out["epfd"] = _u(bits, 134, 4)
    elif ty == 5 and n >= 424:
        out["imo"], out["callsign"], out["shipname"] = _u(bits, 40, 30), _text(bits, 70, 42), _text(bits, 112, 120)
        out["shiptype"] = _u(bits, 232, 8)
        _dimensions(bits, 240, out)
        out["epfd"] = _u(bits, 270, 4)
        out["eta_month"], out["eta_day"], out["eta_hour"], out["eta_minute"] = (_u(bits, 274, 4), _u(bits, 278, 5), _u(bits, 283, 5),
                                                                              _u(bits, 288, 6))
        out["draught"], out["destination"] = _u(bits, 294, 8) / 10.0, _text(bits, 302, 120)
    elif ty == 18 and n >= 168:
        out["sog"], out["accuracy"] = _speed(bits, 46), _u(bits, 56, 1)
        out["lon"], out["lat"] = _position(bits, 57)
        out["cog"], out["heading"], out["second"] = _course(bits, 112), _heading(bits, 124), _u(bits, 133, 6)
    elif ty == 24 and n >= 160:
        out["partno"] = _u(bits, 38, 2)
        if out["partno"] == 0:
            out["shipname"] = _text(bits, 40, 120)
        elif out["partno"] == 1 and n >= 168:
            out["shiptype"], out["vendorid"], out["callsign"] = _u(bits, 40, 8), _text(bits, 48, 42), _text(bits, 90, 42)
            _dimensions(bits, 132, out)
    return out


# ------------------------------------------------------------------------------------------------------------------ the synthesiser
RAMP_BITS, TRAIN_BITS, TAIL_BITS = 8, 24, 4


def burst_bits(message):
    """the bits a transmitter sends for a message of whole bytes, before NRZI: 8 ramp-up bits and 24 training bits 0101.., the
    flag, the stuffed message and FCS (each byte lowest bit first), the flag, a short tail"""
    data = bytes(message)
    fcs = crc(data)
    stream = np.unpackbits(np.frombuffer(data + bytes((fcs & 0xFF, fcs >> 8)), dtype=np.uint8), bitorder="little")
    lead = np.arange(RAMP_BITS + TRAIN_BITS) & 1
    return np.concatenate((lead, FLAG, stuff(stream), FLAG, np.zeros(TAIL_BITS))).astype(np.uint8)


def nrzi(bits, level=1):
    """levels +-1: a 0 changes the level, a 1 keeps it"""
    flips = np.cumsum(1 - np.asarray(bits, dtype=np.int64))
    return np.where(flips & 1, -level, level).astype(np.float64)


def _gauss(rate):
    """the Gaussian pulse of BT 0.4 over +-3 bits at `rate`, unit sum"""
    spb = rate / float(BAUD)
    m = int(math.ceil(3 * spb))
    sigma = math.sqrt(math.log(2.0)) / (2.0 * math.pi * BT) * spb
    g = np.exp(-0.5 * (np.arange(-m, m + 1) / sigma) ** 2)
    return g / g.sum()


def frequency(message, rate, start, n, level=1):
    """(float64[n] instantaneous frequency in Hz of the burst that starts at the fractional sample `start`, float64[n] its envelope):
    the ramp-up bits raise the envelope from 0 to 1, the tail lowers it"""
    bits = burst_bits(message)
    lv = nrzi(bits, level)
    spb = rate / float(BAUD)
    pos = (np.arange(n, dtype=np.float64) - start) / spb
    idx = np.floor(pos).astype(np.int64)
    on = (idx >= 0) & (idx < len(lv))
    sq = np.where(on, lv[np.clip(idx, 0, len(lv) - 1)], 0.0)
    f = np.convolve(sq, _gauss(rate), mode="same") * DEVIATION
    env = np.clip(np.minimum(pos / RAMP_BITS, (len(lv) - pos) / TAIL_BITS), 0.0, 1.0)
    return f, env


def burst_len(message, rate):
    return int(math.ceil(len(burst_bits(message)) * rate / float(BAUD))) + 1


def flag_start(rate, start):
    """the fractional sample at which the start flag of a burst encoded at `start` begins"""
    return start + (RAMP_BITS + TRAIN_BITS) * rate / float(BAUD)


def encode(payloads, rate, starts, channel_offsets=0.0, amplitudes=40.0, sigma=0.0, seed=0, carrier_offsets=0.0, n=None, levels=1):
    """A recording uint8[n, 2] at `rate` S/s that holds one GMSK burst per payload (bytes) from the fractional samples `starts` on:
    frequency +-2400 Hz through the Gaussian pulse, around the burst's channel offset plus its carrier error (Hz), from a seeded random
    phase; Gaussian noise of `sigma` per rail; the u8 value is clip(rint(z + 127.5), 0, 255).  n None: long enough for the last burst."""
    starts = np.atleast_1d(np.asarray(starts, dtype=np.float64))
    chans = np.broadcast_to(np.asarray(channel_offsets, dtype=np.float64), starts.shape)
    amps = np.broadcast_to(np.asarray(amplitudes, dtype=np.float64), starts.shape)
    offs = np.broadcast_to(np.asarray(carrier_offsets, dtype=np.float64), starts.shape)
    lvs = np.broadcast_to(np.asarray(levels), starts.shape)
    if len(payloads) != len(starts):
        raise ValueError("ais.encode: one start per payload")
    if n is None:
        n = max([int(s) + burst_len(p, rate) + 1 for p, s in zip(payloads, starts)] + [0])
    rng = np.random.default_rng(seed)
    z = np.zeros(n, dtype=np.complex128)
    for p, s, c, a, o, lv in zip(payloads, starts, chans, amps, offs, lvs):
        lo = max(int(math.floor(s)) - 1, 0)
        hi = min(n, lo + burst_len(p, rate) + 3)
        if hi <= lo:
            continue
        f, env = frequency(p, rate, s - lo, hi - lo, int(lv))
        phase = rng.uniform(0.0, 2.0 * np.pi) + 2.0 * np.pi * np.cumsum(f + c + o) / rate
        z[lo:hi] += a * env * np.exp(1j * phase)
    noise = rng.normal(0.0, 1.0, (n, 2)) * sigma
    v = np.stack((z.real, z.imag), axis=1) + noise + 127.5
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def encode_audio(payloads, rate, starts, sigma=0.0, seed=0, carrier_offsets=0.0, n=None, levels=1):
    """The discriminator's view of `encode` without the radio: float64[n] audio at `rate` S/s in radians per sample,
    2 pi (f + carrier error) / rate inside a burst and 0 outside, plus Gaussian noise of `sigma` radians"""
    starts = np.atleast_1d(np.asarray(starts, dtype=np.float64))
    offs = np.broadcast_to(np.asarray(carrier_offsets, dtype=np.float64), starts.shape)
    lvs = np.broadcast_to(np.asarray(levels), starts.shape)
    if n is None:
        n = max([int(s) + burst_len(p, rate) + 1 for p, s in zip(payloads, starts)] + [0])
    x = np.zeros(n)
    for p, s, o, lv in zip(payloads, starts, offs, lvs):
        lo = max(int(math.floor(s)) - 1, 0)
        hi = min(n, lo + burst_len(p, rate) + 3)
        if hi <= lo:
            continue
        f, env = frequency(p, rate, s - lo, hi - lo, int(lv))
        x[lo:hi] += 2.0 * np.pi * (f + o * (env > 0)) / rate
    if sigma:
        x = x + np.random.default_rng(seed).normal(0.0, sigma, n)
    return x


# ------------------------------------------------------------------------------------------------------------------ the front end, restated
def lowpass_taps(rate, cut=CUT):
    """the audio-rate channel filter's taps (filters.lowpass): a Hamming-windowed sinc of cut-off `cut` Hz and unit sum,
    2 int(rate / 2400) + 1 taps (eight bit times and a half)"""
    from . import filters
    return np.asarray(filters.lowpass(rate, cut).getB, dtype=np.float64)


def window_taps(fs):
    """the length of the front end's Blackman-Harris window: decode_afsk1200's 151 from 2.4 MS/s up; below that the odd number
    nearest 151 fs / 2 400 000 (at least 9), which keeps the window some +-60 kHz wide: at 240 kS/s 151 taps would be +-6 kHz from
    null to null and take the burst away with its neighbours"""
    if fs >= 2400000:
        return 151
    return max(9, 2 * int(round((151.0 * fs / 2400000.0 - 1.0) / 2.0)) + 1)


def audio_host(raw, fs, offset, bw=48000.0, cut=CUT):
    """(float64 audio, its rate) of one channel of a uint8[N, 2] recording in float64 NumPy: decode_ais's front end restated (the
    mixer, the Blackman-Harris window of window_taps(fs) taps started over ones, every int(fs / bw)-th sample, the channel filter started over zeros,
    the discriminator).  The device's float32 stages round differently: this is the same chain, not the same bits."""
    from . import filters
    a = np.asarray(raw, dtype=np.uint8).reshape(-1, 2).astype(np.float64) - 127.5
    x = (a[:, 0] + 1j * a[:, 1]) * np.exp(-2j * np.pi * offset * np.arange(len(a)) / float(fs))
    K = window_taps(fs)
    bh = filters._cosine_sum(K, [0.35875, 0.48829, 0.14128, 0.01168])
    y = np.convolve(np.concatenate((np.ones(K - 1), x)), bh)[K - 1:K - 1 + len(x)]
    step = int(fs / bw)
    y = y[::step]
    rate = fs / step
    h = lowpass_taps(rate, cut)
    y = np.convolve(y, h)[:len(y)]
    return np.angle(y[1:] * np.conj(y[:-1])), rate
