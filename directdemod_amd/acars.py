"""
ACARS on VHF: 2400 baud MSK on 1200 / 2400 Hz over double-sideband AM, blocks of parity-protected characters closed by a CRC-16
(beyond the reference; DESIGN.md section 4.25 defines every stage; device side: dd_acars.h): the constants, the block check
sequence, a NumPy restatement `candidates_host` / `blocks_host` of the two kernels, the device wrappers over the C entries, `decode`,
the chain behind decode_acars, which runs over either set of stages (`DeviceOps`, `HostOps`) so that the host logic is one piece of
code for both, the candidate merge, the block parser, the reassembly of multi-block downlinks, and `encode` / `encode_audio`, a
synthesiser.

The audio is the AM envelope.  q = rint(audio * 2^12) makes integers of it; everything behind the quantiser is integer.  Bit k of
the start t is decided at the bit's END, the boundary B(t, k) = floor(t + (k + 1) sps): v(t, k) is the sum of the w samples q from
B on less the sum of the w samples before it.  The MSK audio passes through zero at every boundary, downwards into it after a 0 and
upwards after a 1 (polarity 0), so v > 0 reads 1; the carrier's level cancels in the difference, and no mean is taken.

The format is taken from public descriptions of ARINC 618 VHF ACARS; it was not checked against an off-air recording.
INTEGRATION.md lists the limits.
"""
import math

import numpy as np

from . import _burst
from ._burst import Laps, need
from ._hip import DevArray, check, lib

BAUD = 2400
SPS_MIN, SPS_MAX = 8.0, 64.0
W_MAX = 32                            # DD_ACARS_W_MAX
SLACK_MAX = 5                         # DD_ACARS_SLACK_MAX: slid over a block's own pre-key the template stays 6 or more places off
FIX_MAX = 2
TEMPLATE = 0x54686880                 # * SYN SYN SOH, each character lowest bit first, the first-sent bit in bit 31
TEMPLATE_BITS = np.array([(TEMPLATE >> (31 - k)) & 1 for k in range(32)], dtype=bool)
CHARS = 240                           # characters demodulated behind SOH
BLOCK_BITS = 8 * CHARS
FIRST_END = 12                        # mode, address (7), ack, label (2), block id come before the first place ETX / ETB can take
TEXT_MAX = 220
TILE = 256                            # DD_ACARS_TILE
SCALE = 4096.0                        # DD_ACARS_SCALE
CLIP = 2097152.0
CUT = 5000.0                          # the audio-rate channel filter's cut-off, Hz
OK, OUTSIDE, NO_END, BAD_BCS = range(4)
STATUS = ("accepted", "outside", "no_end", "bad_bcs")
ROUTES = ("clean", "one_character", "bcs", "two_characters")     # how an accepted block passed: by parity-flagged characters
MERGE_BITS = 8                        # accepted candidates with the same bytes within this many bit times are one block
CHAIN_SECONDS = 30.0                  # blocks of one message follow each other within this
PLUS, STAR, SYN, SOH, STX, ETX, ETB, DEL, NAK = 0xAB, 0x2A, 0x16, 0x01, 0x02, 0x83, 0x97, 0x7F, 0x15

_F64 = np.dtype(np.float64)


def params(rate, w=None, slack=2, fix=2):
    """(sps, w, slack, fix) for an audio rate: sps = rate / 2400 must lie in 8 .. 64; w None: floor(sps / 2)"""
    sps = float(rate) / BAUD
    if not SPS_MIN <= sps <= SPS_MAX:              # (also false for a NaN)
        raise ValueError("acars: an audio rate of %r S/s at %d baud is %r samples per bit; %g to %g are supported (%g to %g S/s)"
                         % (rate, BAUD, sps, SPS_MIN, SPS_MAX, SPS_MIN * BAUD, SPS_MAX * BAUD))
    if w is None:
        w = int(math.floor(sps / 2.0))
    if int(w) != w or not 1 <= w <= W_MAX:
        raise ValueError("acars: w must be from 1 to %d, got %r" % (W_MAX, w))
    if int(slack) != slack or not 0 <= slack <= SLACK_MAX:
        raise ValueError("acars: slack must be from 0 to %d, got %r" % (SLACK_MAX, slack))
    if int(fix) != fix or not 0 <= fix <= FIX_MAX:
        raise ValueError("acars: fix must be from 0 to %d, got %r" % (FIX_MAX, fix))
    return sps, int(w), int(slack), int(fix)


def reach(sps, w):
    """samples from a start to past the last one its template reads"""
    return int(math.floor(32.0 * sps)) + w


def n_starts(n, sps, w):
    return max(0, int(n) - reach(sps, w) + 1)


# ------------------------------------------------------------------------------------------------------------------ the block check
def _ztable():
    z = np.zeros(BLOCK_BITS, dtype=np.int64)
    v = 0x8408
    for m in range(BLOCK_BITS):
        z[m] = v
        v = (v >> 1) ^ 0x8408 if v & 1 else v >> 1
    return z


ZTABLE = _ztable()                    # the register m zero bits after a lone one bit entered an empty register


def crc_bitwise(data):
    """the CRC-16 register (reflected 0x8408, preset 0, nothing inverted) after the bytes, each lowest bit first, bit by bit"""
    reg = 0
    for byte in bytes(data):
        for b in range(8):
            low = (reg ^ (byte >> b)) & 1
            reg >>= 1
            if low:
                reg ^= 0x8408
    return reg


def residual(data):
    """the same register by the kernel's route: the XOR of the lone-bit registers Z[N - 1 - p] of the one bits p of the N"""
    bits = np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8), bitorder="little")
    if len(bits) > BLOCK_BITS:
        raise ValueError("acars.residual: at most %d bytes" % CHARS)
    ones = np.flatnonzero(bits)
    return int(np.bitwise_xor.reduce(ZTABLE[len(bits) - 1 - ones])) if len(ones) else 0


def odd(values):
    """the characters with their parity bit: bit 7 makes the number of ones odd"""
    v = np.asarray(values, dtype=np.int64) & 0x7F
    ones = ((v[..., None] >> np.arange(7)) & 1).sum(axis=-1)
    return v | np.where(ones & 1, 0, 0x80)


def flagged(data):
    """bool per byte: an even number of ones"""
    return (np.unpackbits(np.asarray(data, dtype=np.uint8).reshape(-1, 1), axis=1).sum(axis=1) & 1) == 0


# ------------------------------------------------------------------------------------------------------------------ the restatement
def quantise(audio):
    """q = rint(audio * 2^12) as int64; 0 for a NaN and beyond +-2^21"""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(audio, dtype=np.float64) * SCALE)
        return np.where((r >= -CLIP) & (r <= CLIP), r, 0.0).astype(np.int64)


def boundaries(ts, ks, sps):
    """int64[len(ts), len(ks)]: floor(t + (k + 1) sps), the product and the sum each rounded to float64"""
    t = np.asarray(ts, dtype=np.int64).astype(np.float64).reshape(-1, 1)
    k = np.asarray(ks, dtype=np.int64).astype(np.float64).reshape(1, -1)
    return np.floor(t + (k + 1.0) * sps).astype(np.int64)


def values(q, ts, ks, sps, w):
    """v(t, k) for every t of ts and k of ks, int64; samples outside the audio count 0"""
    n = len(q)
    cum = np.concatenate((np.zeros(1, dtype=np.int64), np.cumsum(np.asarray(q, dtype=np.int64))))
    at = boundaries(ts, ks, sps)
    return cum[np.clip(at + w, 0, n)] - 2 * cum[np.clip(at, 0, n)] + cum[np.clip(at - w, 0, n)]


def masks_host(audio, sps, w, slack=2, block=1 << 14):
    """the mask byte of every start: 1 the template within `slack` places, 3 its inverse; uint8[n_starts]"""
    q = quantise(audio)
    total = n_starts(len(q), sps, w)
    out = np.zeros(total, dtype=np.uint8)
    for a in range(0, total, block):
        ts = np.arange(a, min(total, a + block), dtype=np.int64)
        mis = ((values(q, ts, np.arange(32), sps, w) > 0) != TEMPLATE_BITS.reshape(1, -1)).sum(axis=1)
        out[a:a + len(ts)] = np.where(mis <= slack, 1, np.where(32 - mis <= slack, 3, 0))
    return out


def candidates_host(audio, sps, w, slack=2):
    """the ordered starts that pass the sync test in either polarity, int64"""
    return np.flatnonzero(masks_host(audio, sps, w, slack) & 1).astype(np.int64)


def find_end(data):
    """the least index from 12 on that holds ETX or ETB with the two BCS bytes behind it inside the 240, or -1"""
    d = np.asarray(data, dtype=np.uint8)[:CHARS - 2]
    hits = np.flatnonzero((d == ETX) | (d == ETB))
    hits = hits[hits >= FIRST_END]
    return int(hits[0]) if len(hits) else -1


def repair(data, e, fix=2):
    """(the bytes, repaired where accepted; accepted; bits repaired; parity-flagged bytes among 0 .. e; the residual as received)
    of 240 received bytes whose end is e: the rule of DESIGN.md section 4.25"""
    d = np.array(data, dtype=np.uint8)
    N = 8 * (e + 3)
    s = residual(d[:e + 3])
    bad = np.flatnonzero(flagged(d[:e + 1]))
    c = len(bad)
    if s == 0:
        return d, True, 0, c, s
    if fix >= 1 and c <= 1:
        first = 8 * int(bad[0]) if c else 8 * (e + 1)
        hit = np.flatnonzero(ZTABLE[N - 1 - (first + np.arange(8 if c else 16))] == s)
        if len(hit) == 1:
            p = first + int(hit[0])
            d[p >> 3] ^= 1 << (p & 7)
            return d, True, 1, c, s
    if fix >= 2 and c == 2:
        pi, pj = 8 * int(bad[0]) + np.arange(8), 8 * int(bad[1]) + np.arange(8)
        i, j = np.nonzero((ZTABLE[N - 1 - pi].reshape(8, 1) ^ ZTABLE[N - 1 - pj].reshape(1, 8)) == s)
        if len(i) == 1:
            d[bad[0]] ^= 1 << int(i[0])
            d[bad[1]] ^= 1 << int(j[0])
            return d, True, 2, c, s
    return d, False, 0, c, s


def judge(data, fix=2):
    """240 received bytes -> (the bytes, repaired where accepted; status; end, -1 without; parity-flagged bytes among 0 .. end; bits
    repaired; whether byte end + 3 is DEL; the residual as received): what the block kernel does behind its bit decisions"""
    e = find_end(data)
    if e < 0:
        return np.array(data, dtype=np.uint8), NO_END, -1, 0, 0, 0, 0
    fixed, ok, nfix, flags, s = repair(data, e, fix)
    return fixed, OK if ok else BAD_BCS, e, flags, nfix, int(e + 3 < CHARS and data[e + 3] == DEL), s


def _empty_det(m=0):
    return {"t": np.zeros(m, np.int64), "bytes": np.zeros((m, CHARS), np.uint8), "status": np.full(m, OUTSIDE, np.int32),
            "polarity": np.zeros(m, np.int32), "mis": np.zeros(m, np.int32), "end": np.full(m, -1, np.int32),
            "flags": np.zeros(m, np.int32), "repaired": np.zeros(m, np.int32), "del": np.zeros(m, np.int32),
            "residual": np.zeros(m, np.int32), "score": np.zeros(m, np.int64)}


META = ("status", "polarity", "mis", "end", "flags", "repaired", "del", "residual")      # meta[8 c ..] of dd_acars_blocks


def blocks_host(audio, sps, w, fix, ts):
    """the listed starts' blocks: a dict of t, bytes uint8[m, 240], status, polarity, mis, end (-1: none), flags (parity-flagged
    bytes among 0 .. end), repaired (bits), del (byte end + 3 is DEL), residual (the register over 0 .. end + 2 as received), score"""
    q = quantise(audio)
    n = len(q)
    ts = np.asarray(ts, dtype=np.int64).reshape(-1)
    det = _empty_det(len(ts))
    det["t"] = ts
    for c, t in enumerate(ts):
        if t < 0 or t >= n:
            continue
        v = values(q, [t], np.arange(32 + BLOCK_BITS), sps, w)[0]
        far = int(((v[:32] > 0) != TEMPLATE_BITS).sum())
        inv = far > 16
        det["polarity"][c], det["mis"][c], det["score"][c] = inv, 32 - far if inv else far, np.abs(v[:32]).sum()
        (det["bytes"][c], det["status"][c], det["end"][c], det["flags"][c], det["repaired"][c], det["del"][c],
         det["residual"][c]) = judge(np.packbits((v[32:] > 0) ^ inv, bitorder="little"), fix)
    return det


# ------------------------------------------------------------------------------------------------------------------ the device stages
def capacity(n, sps):
    """the default list capacity: a clean block passes at about sps / 2 adjacent starts of the 300 sps samples the shortest block
    with its pre-key takes; some four times that share of the audio, and 1024"""
    return 1024 + int(n) // 128


def candidates(audio, sps, w, slack=2, cap=None):
    """float64 device audio -> (the survivors as a device int64 array, how many) (dd_acars_candidates); a list that proves too
    small is asked for again at the true count"""
    need(audio, _F64, "acars.candidates")
    cap = capacity(audio.n, sps) if cap is None else int(cap)
    def call(lst, cap, count):
        return lib().dd_acars_candidates(audio.ptr, audio.n, float(sps), int(w), int(slack), lst, cap, count, None)
    return _burst.candidates("dd_acars_candidates", cap, call)


def blocks(audio, sps, w, fix, lst, m):
    """the first m starts of the device list -> the dict of blocks_host, on the host (dd_acars_blocks)"""
    need(audio, _F64, "acars.blocks")
    if not isinstance(lst, DevArray):
        lst = DevArray.from_host(np.ascontiguousarray(lst, dtype=np.int64))
    det = _empty_det(m)
    if m == 0 or audio.n == 0:
        return det
    data, meta, score = DevArray(CHARS * m, np.uint8), DevArray(len(META) * m, np.int32), DevArray(m, np.int64)
    check(lib().dd_acars_blocks(audio.ptr, audio.n, float(sps), int(w), int(fix), lst.ptr, m, data.ptr, meta.ptr, score.ptr, None),
          "dd_acars_blocks")
    meta = meta.to_host().reshape(m, len(META))
    det.update(t=lst.view(0, m).to_host(), bytes=data.to_host().reshape(m, CHARS), score=score.to_host())
    det.update({key: meta[:, i].copy() for i, key in enumerate(META)})
    return det


def masks_device(audio, sps, w, slack=2):
    """the mask byte of every sample, uint8[n] on the host, 0 past the last start (dd_debug_acars_masks, a diagnostic)"""
    need(audio, _F64, "acars.masks_device")
    return _burst.masks("dd_debug_acars_masks", audio.n,
                        lambda mask: lib().dd_debug_acars_masks(audio.ptr, audio.n, float(sps), int(w), int(slack), mask, None))


class HostOps(Laps):
    """the stages of `decode` in NumPy"""

    def detect(self, audio, sps, w, slack, fix):
        return blocks_host(audio, sps, w, fix, candidates_host(audio, sps, w, slack))


class DeviceOps(Laps):
    """the stages of `decode` on the device; `laps` collects seconds per stage, with a synchronisation after each"""

    def detect(self, audio, sps, w, slack, fix):
        lst, m = candidates(audio, sps, w, slack)
        self.lap("candidates")
        det = blocks(audio, sps, w, fix, lst, m)
        self.lap("blocks")
        return det


# ------------------------------------------------------------------------------------------------------------------ the host logic
def merge(det, sps):
    """The accepted candidates of one channel -> (the kept indices in time order, how many duplicates were dropped): candidates with
    equal bytes 0 .. end + 2 whose starts lie within MERGE_BITS bit times of the group's first are one block; the one with the
    fewest repaired bits stays, then the largest score, then the earliest."""
    acc = [int(i) for i in np.flatnonzero(det["status"] == OK)]
    acc.sort(key=lambda i: (int(det["t"][i]), i))
    body = {i: bytes(det["bytes"][i][:int(det["end"][i]) + 3]) for i in acc}
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
            if not used[b] and body[j] == body[i]:
                used[b] = True
                group.append(j)
        keep.append(min(group, key=lambda j: (int(det["repaired"][j]), -int(det["score"][j]), int(det["t"][j]))))
        dup += len(group) - 1
    return keep, dup


def _show(values):
    return "".join(chr(v) if 32 <= v < 127 else "." for v in values)


def route_of(flags, repaired):
    """the name of the route by which an accepted block passed"""
    return ROUTES[0] if repaired == 0 else (ROUTES[3] if repaired == 2 else ROUTES[1 if flags else 2])


def parse(data, e):
    """The fields of a block's bytes 0 .. e + 2 (mode first, the parity bits still on): mode, address (leading dots stripped), ack
    (None for NAK), label, block_id, downlink (the block id is a digit), text (the characters behind STX; non-printing ones as .),
    msgno and flight (the first 4 and the next 6 characters of a downlink's text, else None), more (ETB), bytes (0 .. e + 2)."""
    raw = bytes(bytearray(data[:e + 3]))
    ch = [b & 0x7F for b in raw]
    text = _show(ch[FIRST_END + 1:e]) if e > FIRST_END and ch[FIRST_END] == STX else ""
    block_id = _show(ch[11:12])
    down = block_id.isdigit()
    return {"mode": _show(ch[0:1]), "address": _show(ch[1:8]).lstrip("."), "ack": None if ch[8] == NAK else _show(ch[8:9]),
            "label": _show(ch[9:11]), "block_id": block_id, "downlink": down, "msgno": text[:4] if down and len(text) >= 10 else None,
            "flight": text[4:10] if down and len(text) >= 10 else None, "text": text, "more": raw[e] == ETB, "bytes": raw}


def messages(found):
    """Blocks in time order -> messages: downlink blocks of one channel and address whose message numbers agree in the first three
    characters, whose block letters (the fourth) are consecutive, of which each but the last carries ETB and each lies within 30 s
    of the one before, are one message; its text is the first block's with the others' behind it less their msgno and flight.
    Anything else is a message of one block.  A message: t, channel, address, label, msgno, flight, text, blocks (how many),
    complete (the last block carries ETX)."""
    out, open_ = [], {}
    for b in found:
        key = (b["channel"], b["address"])
        m = open_.get(key)
        if (m is not None and b["msgno"] is not None and m["msgno"] is not None and m["_more"] and b["msgno"][:3] == m["msgno"][:3]
                and ord(b["msgno"][3]) == m["_letter"] + 1 and 0.0 <= b["t"] - m["_t"] <= CHAIN_SECONDS):
            m["text"] += b["text"][10:]
            m["blocks"] += 1
        else:
            m = {"t": b["t"], "channel": b["channel"], "address": b["address"], "label": b["label"], "msgno": b["msgno"],
                 "flight": b["flight"], "text": b["text"], "blocks": 1}
            out.append(m)
            open_[key] = m
        m["_more"], m["_t"], m["complete"] = b["more"], b["t"], not b["more"]
        m["_letter"] = ord(b["msgno"][3]) if b["msgno"] is not None else -1
    for m in out:
        for key in ("_more", "_t", "_letter"):
            del m[key]
    return out


def line(block):
    """the block as a line of text"""
    return "ACARS %s: Mode: %s Reg: %-7s Ack: %s Label: %s Block: %s%s%s Text: %s" % (
        block["channel"], block["mode"], block["address"], "!" if block["ack"] is None else block["ack"], block["label"],
        block["block_id"], " Msg: %s Flight: %s" % (block["msgno"], block["flight"]) if block["msgno"] is not None else "",
        " (more)" if block["more"] else "", block["text"])


def decode(audios, rate, channels, slack=2, fix=2, w=None, ops=None):
    """The chain behind decode_acars over one audio per channel (float64 device arrays for DeviceOps, NumPy for HostOps) at `rate`
    S/s -> (blocks in time order, frameInfo, the candidates' dict per channel)."""
    ops = HostOps() if ops is None else ops
    sps, w, slack, fix = params(rate, w, slack, fix)
    found, cands = [], {}
    info = {"samples": 0, "blocks": 0, "channels": {}}
    for ch, audio in zip(channels, audios):
        det = ops.detect(audio, sps, w, slack, fix)
        cands[ch] = det
        keep, dup = merge(det, sps)
        info["samples"] = max(info["samples"], len(audio))
        per = {"candidates": len(det["t"]), "accepted": len(keep), "duplicates": dup}
        per.update({name: int(np.count_nonzero(det["status"] == s)) for s, name in enumerate(STATUS) if s})
        per.update({name: 0 for name in ROUTES})
        for i in np.flatnonzero(det["status"] == OK):
            per[route_of(int(det["flags"][i]), int(det["repaired"][i]))] += 1
        info["channels"][ch] = per
        for i in keep:
            t, e = int(det["t"][i]), int(det["end"][i])
            b = {"t": t / float(rate), "start": t, "channel": ch}
            b.update(parse(det["bytes"][i], e))
            b.update(corrected=int(det["repaired"][i]), parity_errors=int(det["flags"][i]), polarity=int(det["polarity"][i]),
                     score=int(det["score"][i]), closed=bool(det["del"][i]))
            found.append(b)
        ops.lap("host")
    found.sort(key=lambda b: (b["start"], b["channel"]))
    info["blocks"] = len(found)
    return found, info, cands


# ------------------------------------------------------------------------------------------------------------------ the synthesiser
PREKEY = 16
RAMP_BITS, TAIL_BITS = 2, 4


def block_bytes(mode, address, ack, label, block_id, text=None, more=False):
    """One block's characters from the mode to DEL, parity bits on: mode, the address right-aligned in seven places behind dots,
    ack (None: NAK), the two label characters, the block id, STX and the text (None: neither), ETX or ETB (`more`), the BCS low byte
    first, DEL"""
    reg = str(address)
    if len(mode) != 1 or len(reg) > 7 or len(label) != 2 or len(block_id) != 1 or (ack is not None and len(ack) != 1):
        raise ValueError("acars.block_bytes: one mode character, at most 7 of address, one of ack, two of label, one of block id")
    if text is not None and len(text) > TEXT_MAX:
        raise ValueError("acars.block_bytes: at most %d characters of text" % TEXT_MAX)
    body = mode + reg.rjust(7, ".") + (chr(NAK) if ack is None else ack) + label + block_id
    if text is not None:
        body += chr(STX) + text
    vals = [ord(ch) for ch in body] + [ETB if more else ETX]
    if any(v > 127 for v in vals[:-1]):
        raise ValueError("acars.block_bytes: 7-bit characters only")
    data = bytes(odd(vals).astype(np.uint8).tolist())
    bcs = crc_bitwise(data)
    return data + bytes((bcs & 0xFF, bcs >> 8, DEL))


def block_bits(block, prekey=PREKEY, flips=None):
    """the bits on the air: `prekey` characters 0xFF, + * SYN SYN SOH, the block (block_bytes), each character lowest bit first;
    flips {index into the block's bytes: XOR mask} spoils characters on their way"""
    data = bytearray(block)
    for i, mask in (flips or {}).items():
        data[i] ^= int(mask)
    frame = bytes([0xFF] * int(prekey) + [PLUS, STAR, SYN, SYN, SOH]) + bytes(data)
    return np.unpackbits(np.frombuffer(frame, dtype=np.uint8), bitorder="little")


def block_start(rate, start, prekey=PREKEY):
    """the fractional sample at which the template (the * behind the +) of a block encoded at `start` begins"""
    return start + (8 * prekey + 8) * rate / float(BAUD)


def msk(bits, rate, start, n, polarity=0):
    """(float64[n] the MSK audio sin(phase) of the bits from the fractional sample `start` on, 0 outside them; float64[n] the
    carrier's envelope): a bit that equals the one before is a full cycle of 2400 Hz, one that differs half a cycle of 1200 Hz, the
    bit before the first counting 1 and the phase starting at 0; polarity 1 negates the audio.  The carrier rises over the first two
    bits and falls over four bit times behind the last."""
    b = np.asarray(bits, dtype=np.int64)
    same = np.concatenate(([1], b[:-1])) == b
    step = np.where(same, 2.0, 1.0)                                          # half cycles per bit
    at = np.concatenate(([0.0], np.cumsum(step)[:-1]))                       # half cycles before bit k
    spb = rate / float(BAUD)
    pos = (np.arange(n, dtype=np.float64) - start) / spb
    idx = np.floor(pos).astype(np.int64)
    on = (idx >= 0) & (idx < len(b))
    k = np.clip(idx, 0, max(len(b) - 1, 0))
    audio = np.where(on, np.sin(np.pi * (at[k] + (pos - k) * step[k])), 0.0) if len(b) else np.zeros(n)
    env = np.clip(np.minimum(pos / RAMP_BITS, (len(b) + TAIL_BITS - pos) / TAIL_BITS), 0.0, 1.0)
    return (-audio if polarity else audio), env


def _plan(blocks_, rate, starts, prekey, polarity, flips, n):
    starts = np.atleast_1d(np.asarray(starts, dtype=np.float64))
    if len(blocks_) != len(starts):
        raise ValueError("acars.encode: one start per block")
    pres = np.broadcast_to(np.asarray(prekey), starts.shape)
    pols = np.broadcast_to(np.asarray(polarity), starts.shape)
    flips = flips if flips is not None else [None] * len(starts)
    plan = []
    for blk, s, pre, pol, fl in zip(blocks_, starts, pres, pols, flips):
        bits = block_bits(blk, int(pre), fl)
        lo = max(int(math.floor(s)) - 1, 0)
        plan.append((bits, float(s), int(pol), lo, lo + int(math.ceil((len(bits) + TAIL_BITS) * rate / float(BAUD))) + 4))
    if n is None:
        n = max([p[4] for p in plan] + [0])
    return plan, int(n)


def encode(blocks_, rate, starts, offsets=0.0, depth=0.8, amplitudes=40.0, sigma=0.0, seed=0, prekey=PREKEY, polarity=0, flips=None,
           n=None):
    """A recording uint8[n, 2] at `rate` S/s that holds one block (block_bytes) per fractional sample of `starts`: a carrier at the
    block's offset (Hz) from a seeded random phase, of amplitude a (1 + depth m) with m the MSK audio (msk); Gaussian noise of
    `sigma` per rail; the u8 value is clip(rint(z + 127.5), 0, 255).  flips: per block None or {byte index: XOR mask}.  offsets,
    amplitudes, prekey and polarity: one value, or one per block.  n None: long enough for the last block."""
    plan, n = _plan(blocks_, rate, starts, prekey, polarity, flips, n)
    offs = np.broadcast_to(np.asarray(offsets, dtype=np.float64), (len(plan),))
    amps = np.broadcast_to(np.asarray(amplitudes, dtype=np.float64), (len(plan),))
    rng = np.random.default_rng(seed)
    z = np.zeros(n, dtype=np.complex128)
    for (bits, s, pol, lo, hi), off, a in zip(plan, offs, amps):
        hi = min(n, hi)
        if hi <= lo:
            continue
        m, env = msk(bits, rate, s - lo, hi - lo, pol)
        phase = rng.uniform(0.0, 2.0 * np.pi) + 2.0 * np.pi * off * np.arange(lo, hi) / rate
        z[lo:hi] += a * env * (1.0 + depth * m) * np.exp(1j * phase)
    v = np.stack((z.real, z.imag), axis=1) + rng.normal(0.0, 1.0, (n, 2)) * sigma + 127.5
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def encode_audio(blocks_, rate, starts, depth=0.8, amplitudes=40.0, sigma=0.0, seed=0, prekey=PREKEY, polarity=0, flips=None, n=None):
    """The envelope detector's view of `encode` without the radio: float64[n] at `rate` S/s, a (1 + depth m) inside a block and 0
    outside, plus Gaussian noise of `sigma`"""
    plan, n = _plan(blocks_, rate, starts, prekey, polarity, flips, n)
    amps = np.broadcast_to(np.asarray(amplitudes, dtype=np.float64), (len(plan),))
    x = np.zeros(n)
    for (bits, s, pol, lo, hi), a in zip(plan, amps):
        hi = min(n, hi)
        if hi <= lo:
            continue
        m, env = msk(bits, rate, s - lo, hi - lo, pol)
        x[lo:hi] += a * env * (1.0 + depth * m)
    if sigma:
        x = x + np.random.default_rng(seed).normal(0.0, sigma, n)
    return x


# ------------------------------------------------------------------------------------------------------------------ the front end, restated
def audio_host(raw, fs, offset, bw=48000.0, cut=CUT):
    """(float64 envelope, its rate) of the channel at `offset` Hz of a uint8[N, 2] recording in float64 NumPy: decode_acars's front
    end restated (the mixer, the Blackman-Harris window of ais.window_taps(fs) taps started over ones, every int(fs / bw)-th sample,
    the channel filter started over zeros, the magnitude).  The device's float32 stages round differently: this is the same chain,
    not the same bits."""
    from . import ais, filters
    a = np.asarray(raw, dtype=np.uint8).reshape(-1, 2).astype(np.float64) - 127.5
    x = (a[:, 0] + 1j * a[:, 1]) * np.exp(-2j * np.pi * offset * np.arange(len(a)) / float(fs))
    K = ais.window_taps(fs)
    bh = filters._cosine_sum(K, [0.35875, 0.48829, 0.14128, 0.01168])
    y = np.convolve(np.concatenate((np.ones(K - 1), x)), bh)[K - 1:K - 1 + len(x)]
    step = int(fs / bw)
    y = y[::step]
    rate = fs / step
    y = np.convolve(y, ais.lowpass_taps(rate, cut))[:len(y)]
    return np.abs(y), rate
