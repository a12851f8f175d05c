"""
1090 MHz Mode S / ADS-B squitters (beyond the reference; DESIGN.md section 4.22 defines every stage; device side: dd_adsb.h): an
all-integer NumPy restatement `power`, `chips`, `candidates_host`, `demod_host` of the kernels, the device wrappers over the C
entries, the acceptance and duplicate rules (`accept`, one piece of code over device and restatement output), the CRC, the parser
of DF 17/18 type codes, the CPR position arithmetic and `encode`, a synthesiser.

Positions are integers in units of 1/U sample (U = 2 000 000 chips per second): sample j covers [j U, (j + 1) U), candidate k
starts at k U / Q and its chip c covers R units from there on.  Divided by g = gcd(U / Q, R) these are u = U / g, xq = U / (Q g)
and r = R / g; a chip energy is the sum of overlap * power, an exact integer below 2^63.
"""
import math

import numpy as np

from . import _hip
from . import _burst
from ._hip import DevArray, check, lib

U = 2000000                           # chips per second
RATE_MIN, RATE_MAX = 2000000, 20000000
PHASES = (1, 2, 4, 8)
CHIPS, PREAMBLE = 240, 16             # chips of a candidate; of its preamble
GENERATOR = 0x1FFF409
TILE = 256                            # samples' worth of starts per workgroup of dd_adsb_candidates (DD_ADSB_TILE)
PULSES = (0, 2, 7, 9)                 # the preamble's high chips
QUIET = (4, 5, 11, 12, 13, 14)        # chips that must stay below a sixth of the pulses' sum
AP_FORMATS = (0, 4, 5, 16, 20, 21)    # address-overlaid parity
_CHARSET = "#ABCDEFGHIJKLMNOPQRSTUVWXYZ#####_###############0123456789######"


def check_rate(rate, phases=None):
    """(rate, Q) as integers; ValueError outside 2..20 MS/s or for a Q not in 1, 2, 4, 8.  phases None: the smallest Q with
    Q rate >= 8 000 000"""
    if int(rate) != rate or not RATE_MIN <= int(rate) <= RATE_MAX:
        raise ValueError("adsb: the sample rate must be an integer from %d to %d Hz, got %r" % (RATE_MIN, RATE_MAX, rate))
    rate = int(rate)
    if phases is None:
        phases = next(q for q in PHASES if q * rate >= 8000000)
    if phases not in PHASES:
        raise ValueError("adsb: phases must be one of %r, got %r" % (PHASES, phases))
    return rate, int(phases)


def grid(rate, Q):
    """(u, xq, r): units per sample, per candidate step and per chip, all divided by g = gcd(U / Q, rate)"""
    rate, Q = check_rate(rate, Q)
    g = math.gcd(U // Q, rate)
    return U // g, U // Q // g, rate // g


def n_candidates(n, rate, Q):
    """how many k >= 0 have k U / Q + 240 R <= n U"""
    rate, Q = check_rate(rate, Q)
    room = int(n) * U - CHIPS * rate
    return 0 if room < 0 else room // (U // Q) + 1


def reach(rate):
    """samples from a candidate's first to past its last: ceil(240 R / U)"""
    return -(-CHIPS * int(rate) // U)


# ------------------------------------------------------------------------------------------------------------------ the CRC
def _table():
    t = np.zeros(112, dtype=np.int64)
    v = 1
    for i in range(111, -1, -1):                    # position i is x^(111 - i); v = that power modulo the generator
        t[i] = v
        v <<= 1
        if v & (1 << 24):
            v ^= GENERATOR
    return t


TABLE = _table()                      # remainder of a lone bit at each position of a 112-bit word; the last 56 serve a 56-bit word


def as_bytes(frame):
    return bytes.fromhex(frame) if isinstance(frame, str) else bytes(frame)


def bits_of(frame):
    return np.unpackbits(np.frombuffer(as_bytes(frame), dtype=np.uint8))


def crc(frame):
    """the remainder of a 7 or 14 byte frame by the generator: 0 for a valid DF 11 / 17 / 18 frame, the address for
    address-overlaid parity"""
    b = bits_of(frame)
    if len(b) not in (56, 112):
        raise ValueError("adsb.crc: 7 or 14 bytes expected")
    return int(np.bitwise_xor.reduce(TABLE[112 - len(b):][b == 1])) if b.any() else 0


# ------------------------------------------------------------------------------------------------------------------ the restatement
def power(raw):
    """uint8[n, 2] -> int64[n]: (2 I - 255)^2 + (2 Q - 255)^2"""
    a = np.asarray(raw, dtype=np.uint8).reshape(-1, 2).astype(np.int64) * 2 - 255
    return a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]


def _integral(p, u):
    """x -> the integral of the power from 0 to position x (units of g), as uint64: differences are exact although the
    running sum itself may wrap"""
    p = np.concatenate((np.asarray(p, dtype=np.int64), [0])).astype(np.uint64)
    cum = np.concatenate((np.zeros(1, dtype=np.uint64), np.cumsum(p[:-1] * np.uint64(u), dtype=np.uint64)))

    def at(x):
        j = x // u
        return cum[j] + (x - j * u).astype(np.uint64) * p[j]
    return at


def chips(p, rate, Q, ks, count=CHIPS):
    """E_k[0 .. count) for the candidates ks, int64[len(ks), count]"""
    u, xq, r = grid(rate, Q)
    ks = np.asarray(ks, dtype=np.int64).reshape(-1)
    if len(ks) and (ks.min() < 0 or ks.max() >= n_candidates(len(p), rate, Q)):
        raise ValueError("adsb.chips: candidate outside the recording")
    at = _integral(p, u)
    edges = at(ks.reshape(-1, 1) * xq + np.arange(count + 1, dtype=np.int64).reshape(1, -1) * r)
    return (edges[:, 1:] - edges[:, :-1]).astype(np.int64)


def preamble_ok(E):
    """the thirteen strict inequalities over E[..., 0 .. 15)"""
    e = [E[..., c] for c in range(15)]
    ok = (e[0] > e[1]) & (e[2] > e[1]) & (e[2] > e[3]) & (e[7] > e[6]) & (e[7] > e[8]) & (e[9] > e[8]) & (e[9] > e[10])
    s = e[0] + e[2] + e[7] + e[9]
    for q in QUIET:
        ok &= 6 * e[q] < s
    return ok


def candidates_host(p, rate, Q, block=1 << 16):
    """the ordered candidates that pass the preamble test, int64"""
    total = n_candidates(len(p), rate, Q)
    out = []
    for a in range(0, total, block):
        ks = np.arange(a, min(total, a + block), dtype=np.int64)
        out.append(ks[preamble_ok(chips(p, rate, Q, ks, PREAMBLE))])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def _empty_det(m=0):
    return {"k": np.zeros(m, np.int64), "frames": np.zeros((m, 14), np.uint8), "L": np.zeros(m, np.int32), "df": np.zeros(m, np.int32),
            "rem": np.zeros(m, np.int32), "fixed": np.full(m, -1, np.int32), "score": np.zeros(m, np.int64)}


def demod_host(p, rate, Q, ks):
    """the listed candidates' frames: a dict of k, frames uint8[m, 14] (repaired, zero beyond L), L, df, rem, fixed, score"""
    ks = np.asarray(ks, dtype=np.int64).reshape(-1)
    det = _empty_det(len(ks))
    det["k"] = ks
    if not len(ks):
        return det
    E = chips(p, rate, Q, ks)
    hi, lo = E[:, 16::2], E[:, 17::2]
    bits = (hi > lo).astype(np.int64)
    df = bits[:, :5] @ np.array([16, 8, 4, 2, 1])
    L = np.where(df >= 16, 112, 56)
    live = np.arange(112).reshape(1, -1) < L.reshape(-1, 1)
    bits *= live
    det["score"] = (np.abs(hi - lo) * live).sum(axis=1)
    tab = np.where((L == 112).reshape(-1, 1), TABLE.reshape(1, -1), np.concatenate((TABLE[56:], np.zeros(56, np.int64))).reshape(1, -1))
    rem = np.bitwise_xor.reduce(tab * bits, axis=1)
    fixed = np.full(len(ks), -1, dtype=np.int64)
    for i in np.flatnonzero((L == 112) & ((df == 17) | (df == 18)) & (rem != 0)):
        pos = np.flatnonzero(TABLE == rem[i])
        if len(pos) == 1 and pos[0] >= 5:
            fixed[i] = pos[0]
            bits[i, pos[0]] ^= 1
    det["frames"] = np.packbits(bits.astype(np.uint8), axis=1)
    det["L"], det["df"], det["rem"], det["fixed"] = L.astype(np.int32), df.astype(np.int32), rem.astype(np.int32), fixed.astype(np.int32)
    return det


# ------------------------------------------------------------------------------------------------------------------ the device stages
def _need(a, what):
    if not isinstance(a, DevArray) or a.dtype != _hip.IQ8:
        raise TypeError("%s: a device array of raw uint8 pairs (_hip.IQ8) expected" % what)


def to_device(raw):
    """uint8 pairs (an [n, 2] array, or flat and interleaved) -> a device array of _hip.IQ8"""
    d = DevArray.from_host(np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1))
    return DevArray(d.n // 2, _hip.IQ8, ptr=d.ptr, base=d)


def candidates(iq, rate, Q, cap=None):
    """device IQ8 pairs -> (the survivors as a device int64 array, how many) (dd_adsb_candidates); a list that proves too small
    is asked for again at the true count"""
    _need(iq, "adsb.candidates")
    rate, Q = check_rate(rate, Q)
    cap = 1024 + n_candidates(iq.n, rate, Q) // 128 if cap is None else int(cap)
    def call(lst, cap, count):
        return lib().dd_adsb_candidates(iq.ptr, iq.n, rate, Q, lst, cap, count, None)
    return _burst.candidates("dd_adsb_candidates", cap, call)


def demod(iq, rate, Q, lst, m):
    """the first m candidates of the device list -> the dict of demod_host, on the host (dd_adsb_demod)"""
    _need(iq, "adsb.demod")
    rate, Q = check_rate(rate, Q)
    if not isinstance(lst, DevArray):
        lst = DevArray.from_host(np.ascontiguousarray(lst, dtype=np.int64))
    det = _empty_det(m)
    if m == 0:
        return det
    frames, meta, score = DevArray(14 * m, np.uint8), DevArray(4 * m, np.int32), DevArray(m, np.int64)
    check(lib().dd_adsb_demod(iq.ptr, iq.n, rate, Q, lst.ptr, m, frames.ptr, meta.ptr, score.ptr, None), "dd_adsb_demod")
    meta = meta.to_host().reshape(m, 4)
    det.update(k=lst.view(0, m).to_host(), frames=frames.to_host().reshape(m, 14), L=meta[:, 0].copy(), df=meta[:, 1].copy(),
               rem=meta[:, 2].copy(), fixed=meta[:, 3].copy(), score=score.to_host())
    return det


def chips_device(iq, rate, Q, ks):
    """E_k[0 .. 240) for the listed candidates, int64[m, 240] on the host (dd_debug_adsb_chips, a diagnostic)"""
    _need(iq, "adsb.chips_device")
    rate, Q = check_rate(rate, Q)
    ks = np.ascontiguousarray(ks, dtype=np.int64).reshape(-1)
    if not len(ks):
        return np.zeros((0, CHIPS), dtype=np.int64)
    lst, E = DevArray.from_host(ks), DevArray(len(ks) * CHIPS, np.int64)
    check(lib().dd_debug_adsb_chips(iq.ptr, iq.n, rate, Q, lst.ptr, len(ks), E.ptr, None), "dd_debug_adsb_chips")
    return E.to_host().reshape(len(ks), CHIPS)


def detect_host(raw, rate, Q):
    """(det, how many passed) of a host recording by the restatement"""
    p = power(raw)
    ks = candidates_host(p, rate, Q)
    return demod_host(p, rate, Q, ks), len(ks)


def concat_det(dets):
    dets = [d for d in dets if len(d["k"])]
    if not dets:
        return _empty_det()
    return {key: np.concatenate([d[key] for d in dets]) for key in dets[0]}


# ------------------------------------------------------------------------------------------------------------------ acceptance
def icao_of(frame):
    return (int(frame[1]) << 16) | (int(frame[2]) << 8) | int(frame[3])


def accept(det, rate, Q, fix=1):
    """The acceptance and duplicate rules over a recording's detections (start order) -> (messages, counts).  A message is a
    dict of k, df, icao (an int), raw (bytes), fixed, score; counts has clean, repaired, address_parity (of the messages kept)
    and duplicates."""
    rate, Q = check_rate(rate, Q)
    k, df, rem, fixed, L = det["k"], det["df"], det["rem"], det["fixed"], det["L"]
    fr = det["frames"]
    icao = (fr[:, 1].astype(np.int64) << 16) | (fr[:, 2].astype(np.int64) << 8) | fr[:, 3]
    squitter = (df == 17) | (df == 18)
    clean = (squitter | (df == 11)) & (rem == 0)
    known = np.unique(icao[clean])
    repaired = squitter & ~clean & (fixed >= 0) & np.isin(icao, known) & bool(fix)
    overlaid = np.isin(df, AP_FORMATS) & np.isin(rem, known)
    acc = []                                                         # (k, repaired bits, -score, index, kind, icao)
    for kind, mask, address in (("clean", clean, icao), ("repaired", repaired, icao), ("address_parity", overlaid, rem)):
        acc += [(int(k[i]), int(kind == "repaired"), -int(det["score"][i]), int(i), kind, int(address[i])) for i in np.flatnonzero(mask)]
    acc.sort()
    msgs, counts = [], {"clean": 0, "repaired": 0, "address_parity": 0, "duplicates": 0}
    at = 0
    while at < len(acc):
        end = at + 1
        while end < len(acc) and (acc[end][0] - acc[at][0]) * (U // Q) < 2 * rate:
            end += 1
        best = min(acc[at:end], key=lambda a: (a[1], a[2], a[0]))
        i = best[3]
        msgs.append({"k": best[0], "df": int(df[i]), "icao": best[5], "raw": bytes(det["frames"][i][:int(L[i]) // 8]),
                     "fixed": int(fixed[i]) if best[4] == "repaired" else -1, "score": int(det["score"][i])})
        counts[best[4]] += 1
        counts["duplicates"] += end - at - 1
        at = end
    return msgs, counts


# ------------------------------------------------------------------------------------------------------------------ the fields
def _field(v, nbits, first, count):
    """bits first .. first + count of an nbits-wide integer, the most significant bit being bit 0"""
    return (v >> (nbits - first - count)) & ((1 << count) - 1)


def parse(frame):
    """A frame's fields: df, icao (DF 11 / 17 / 18; None where the address is overlaid on the parity), tc (DF 17 / 18, else
    None) and, by type code: 1-4 callsign and category; 9-18 alt (feet; None unless the Q bit is set), alt_q, cpr_f, cpr_lat,
    cpr_lon; 19 subtype and, for subtypes 1-2, gs (knots), track (degrees), for 3-4 heading (None without its status bit),
    airspeed, airspeed_type; vr (feet per minute, None when not given).  Everything else is left raw."""
    raw = as_bytes(frame)
    out = {"df": raw[0] >> 3, "icao": None, "tc": None}
    if out["df"] in (11, 17, 18):
        out["icao"] = icao_of(raw)
    if out["df"] not in (17, 18) or len(raw) != 14:
        return out
    me = int.from_bytes(raw[4:11], "big")
    tc = out["tc"] = _field(me, 56, 0, 5)
    if 1 <= tc <= 4:
        out["category"] = _field(me, 56, 5, 3)
        out["callsign"] = "".join(_CHARSET[_field(me, 56, 8 + 6 * i, 6)] for i in range(8))
    elif 9 <= tc <= 18:
        a = _field(me, 56, 8, 12)
        out["alt_q"] = (a >> 4) & 1
        out["alt"] = 25 * (((a & 0xFE0) >> 1) | (a & 0xF)) - 1000 if out["alt_q"] else None
        out["cpr_f"], out["cpr_lat"], out["cpr_lon"] = _field(me, 56, 21, 1), _field(me, 56, 22, 17), _field(me, 56, 39, 17)
    elif tc == 19:
        st = out["subtype"] = _field(me, 56, 5, 3)
        scale = 4 if st in (2, 4) else 1
        if st in (1, 2):
            dew, vew, dns, vns = _field(me, 56, 13, 1), _field(me, 56, 14, 10), _field(me, 56, 24, 1), _field(me, 56, 25, 10)
            out["gs"] = out["track"] = None
            if vew and vns:
                we, sn = (vew - 1) * scale * (-1 if dew else 1), (vns - 1) * scale * (-1 if dns else 1)
                out["gs"] = math.hypot(we, sn)
                out["track"] = math.degrees(math.atan2(we, sn)) % 360.0
        elif st in (3, 4):
            out["heading"] = _field(me, 56, 14, 10) * 360.0 / 1024.0 if _field(me, 56, 13, 1) else None
            spd = _field(me, 56, 25, 10)
            out["airspeed"] = (spd - 1) * scale if spd else None
            out["airspeed_type"] = "TAS" if _field(me, 56, 24, 1) else "IAS"
        if st in (1, 2, 3, 4):
            vr = _field(me, 56, 37, 9)
            out["vr"] = (vr - 1) * 64 * (-1 if _field(me, 56, 36, 1) else 1) if vr else None
    return out


def NL(lat):
    """the number of longitude zones at a latitude (15 latitude zones per quadrant)"""
    lat = abs(float(lat))
    if lat == 0.0:
        return 59
    if lat == 87.0:
        return 2
    if lat > 87.0:
        return 1
    a = 1.0 - math.cos(math.pi / 30.0)
    return int(math.floor(2.0 * math.pi / math.acos(1.0 - a / math.cos(math.radians(lat)) ** 2)))


def _cpr(f):
    return f["cpr_lat"] / 131072.0, f["cpr_lon"] / 131072.0


def cpr_latitudes(even, odd):
    """the two latitudes of an even / odd pair of parsed position frames"""
    (le, _), (lo, _) = _cpr(even), _cpr(odd)
    j = math.floor(59.0 * le - 60.0 * lo + 0.5)
    lat_e, lat_o = 6.0 * (j % 60 + le), 360.0 / 59.0 * (j % 59 + lo)
    return (lat_e - 360.0 if lat_e >= 270.0 else lat_e), (lat_o - 360.0 if lat_o >= 270.0 else lat_o)


def cpr_global(even, odd, latest):
    """(lat, lon) from an even and an odd parsed position frame, `latest` 0 when the even one came last, else 1; None when the
    two latitudes lie in different longitude zones"""
    lat_e, lat_o = cpr_latitudes(even, odd)
    if NL(lat_e) != NL(lat_o):
        return None
    (_, ce), (_, co) = _cpr(even), _cpr(odd)
    nl = NL(lat_e)
    m = math.floor(ce * (nl - 1) - co * nl + 0.5)
    if latest == 0:
        ni, lat, c = max(nl, 1), lat_e, ce
    else:
        ni, lat, c = max(nl - 1, 1), lat_o, co
    lon = 360.0 / ni * (m % ni + c)
    return lat, (lon - 360.0 if lon >= 180.0 else lon)


def cpr_local(ref, frame):
    """(lat, lon) of one parsed position frame near the reference position ref = (lat, lon)"""
    f = frame["cpr_f"]
    cl, cn = _cpr(frame)
    dlat = 360.0 / (60 - f)
    j = math.floor(ref[0] / dlat) + math.floor(0.5 + (ref[0] % dlat) / dlat - cl)
    lat = dlat * (j + cl)
    nl = NL(lat) - f
    dlon = 360.0 / nl if nl > 0 else 360.0
    m = math.floor(ref[1] / dlon) + math.floor(0.5 + (ref[1] % dlon) / dlon - cn)
    return lat, dlon * (m + cn)


def aircraft(msgs):
    """messages in time order (each with t, icao and the parsed fields) -> {icao: {callsign, velocity, track}}: a track of
    (t, lat, lon, alt) starts from an even / odd pair at most 10 s apart in one longitude zone and goes on by local decoding
    against the previous fix"""
    out = {}
    pend = {}
    for m in msgs:
        a = out.setdefault(m["icao"], {"callsign": None, "velocity": None, "track": []})
        if m.get("callsign") is not None:
            a["callsign"] = m["callsign"]
        if m.get("tc") == 19 and "subtype" in m:
            a["velocity"] = {key: m[key] for key in ("subtype", "gs", "track", "heading", "airspeed", "airspeed_type", "vr") if key in m}
        if "cpr_f" not in m:
            continue
        fix = None
        if a["track"]:
            fix = cpr_local(a["track"][-1][1:3], m)
        else:
            two = pend.setdefault(m["icao"], [None, None])
            two[m["cpr_f"]] = m
            if two[0] is not None and two[1] is not None and abs(two[0]["t"] - two[1]["t"]) <= 10.0:
                fix = cpr_global(two[0], two[1], m["cpr_f"])
        if fix is not None:
            a["track"].append((m["t"], fix[0], fix[1], m["alt"]))
    return out


# ------------------------------------------------------------------------------------------------------------------ the synthesiser
def pulse_chips(frame):
    """the chips at which a frame's carrier is on: the four preamble pulses, then chip 16 + 2 b for a one and 17 + 2 b for a zero"""
    b = bits_of(frame).astype(np.int64)
    return np.concatenate((np.array(PULSES), PREAMBLE + 2 * np.arange(len(b)) + 1 - b))


def _cover_span(frame, rate, start):
    """(first sample, the covered fraction of each sample from there on) of a frame that starts at the fractional sample `start`"""
    spc = float(rate) / U                                            # samples per chip
    a = start + pulse_chips(frame).reshape(-1, 1) * spc
    j0 = int(math.floor(start))
    j = np.arange(j0, j0 + reach(rate) + 2, dtype=np.float64).reshape(1, -1)
    return j0, (np.clip(j + 1.0 - a, 0.0, spc) - np.clip(j - a, 0.0, spc)).sum(axis=0)


def cover(frame, rate, start, n):
    """float64[n]: the fraction of each sample covered by the pulses of a frame that starts at the fractional sample `start`"""
    j0, part = _cover_span(frame, rate, start)
    out = np.zeros(n)
    lo, hi = max(j0, 0), min(n, j0 + part.size)
    if hi > lo:
        out[lo:hi] = part[lo - j0:hi - j0]
    return out


def encode(frames, rate, starts, amplitudes=40.0, sigma=0.0, seed=0, carrier_offsets=0.0, n=None):
    """A recording uint8[n, 2] that holds the frames (hex strings or bytes) at the fractional samples `starts`: each sample's
    complex amplitude is the frame's amplitude times the fraction of the sample its pulses cover, turned by a phase that starts at
    a seeded random angle and advances by the frame's carrier offset (Hz); Gaussian noise of `sigma` per rail; the u8 value is
    clip(rint(z + 127.5), 0, 255).  n None: long enough for the last frame's 240 chips."""
    rate, _ = check_rate(rate, None)
    starts = np.atleast_1d(np.asarray(starts, dtype=np.float64))
    amps = np.broadcast_to(np.asarray(amplitudes, dtype=np.float64), starts.shape)
    offs = np.broadcast_to(np.asarray(carrier_offsets, dtype=np.float64), starts.shape)
    if len(frames) != len(starts):
        raise ValueError("adsb.encode: one start per frame")
    if n is None:
        n = int(math.ceil(starts.max() + CHIPS * rate / U)) + 1 if len(starts) else 0
    rng = np.random.default_rng(seed)
    z = np.zeros(n, dtype=np.complex128)
    for f, s, a, o in zip(frames, starts, amps, offs):
        j0, part = _cover_span(f, rate, s)
        lo, hi = max(j0, 0), min(n, j0 + part.size)
        turn = np.exp(1j * (rng.uniform(0.0, 2.0 * np.pi) + 2.0 * np.pi * o * np.arange(lo, hi, dtype=np.float64) / rate))
        if hi > lo:
            z[lo:hi] += a * part[lo - j0:hi - j0] * turn
    noise = rng.normal(0.0, 1.0, (n, 2)) * sigma
    v = np.stack((z.real, z.imag), axis=1) + noise + 127.5
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)
