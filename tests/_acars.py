"""What the two ACARS test files share: the recording of the end-to-end tests, the short block of the repair tests with its
error patterns, and builders of crafted audio whose quantised values are chosen integers."""
import functools

import numpy as np

from directdemod_amd import acars

# ---------------------------------------------------------------------------------------------------------------- the recording
FS = 240000
OFFSETS = (25000.0, -50000.0)         # channel A and channel B; 75 kHz apart, three channel spacings
AMPLITUDE, SIGMA = 40.0, 2.0
CHAIN = ("M07A", "BA0123")            # the message number (block letter last) and the flight id of channel B's downlink

LONG_TEXT = "".join(chr(33 + (7 * i) % 90) for i in range(acars.TEXT_MAX))
CHAIN_TEXT = ("POS N51289W000271,", "1542,350,ETA 1630", "/FUEL 0123")


@functools.lru_cache(maxsize=None)
def blocks():
    """(the blocks' bytes, their channel's index, their starts in seconds, their polarity): channel A holds a block with no text,
    one with one character and one with 220; channel B, inverted, a downlink of three blocks, the first two closed by ETB"""
    a = [acars.block_bytes("2", "G-ABCD", None, "Q0", "1"),
         acars.block_bytes("2", "N123AB", "A", "_\x7f", "S", "x"),
         acars.block_bytes("E", "OH-LVA", None, "H1", "7", LONG_TEXT)]
    b = [acars.block_bytes("2", "G-EUPJ", None, "10", str(3 + i), CHAIN[0][:3] + "ABC"[i] + CHAIN[1] + text, more=i < 2)
         for i, text in enumerate(CHAIN_TEXT)]
    return (a + b, [0, 0, 0, 1, 1, 1], [0.0101, 0.15, 0.3, 0.020003, 0.32, 0.61], [0, 0, 0, 1, 1, 1])


@functools.lru_cache(maxsize=None)
def recording():
    """uint8[N, 2] at 240 kS/s, about 1.2 s: the blocks of `blocks` on two channels at once, over noise"""
    blks, chans, starts, pols = blocks()
    raw = acars.encode(blks, FS, [s * FS for s in starts], [OFFSETS[c] for c in chans], 0.8, AMPLITUDE, SIGMA, seed=11, polarity=pols)
    raw.setflags(write=False)
    return raw


def expected():
    """(channel, bytes from the mode through the block check) of every block of the recording in time order"""
    blks, chans, starts, _ = blocks()
    order = sorted(range(len(blks)), key=lambda i: starts[i])
    return [("AB"[chans[i]], blks[i][:-1]) for i in order]


# ---------------------------------------------------------------------------------------------------------------- the short block
SHORT = acars.block_bytes("2", "N123AB", None, "Q0", "5")             # no text: ETX is byte 12, the block check bytes 13 and 14


def received(block=SHORT, flips=()):
    """uint8[240] as the block kernel would see the block: its bytes, then zeros; `flips` are bit positions (8 byte + bit)"""
    d = np.zeros(acars.CHARS, dtype=np.uint8)
    d[:len(block)] = np.frombuffer(block, dtype=np.uint8)
    for p in flips:
        d[p >> 3] ^= 1 << (p & 7)
    return d


@functools.lru_cache(maxsize=None)
def twin_pairs(e=236):
    """For a block whose end is e: (f1, i, f2, j, i2, j2) such that flipping bit i of byte f1 and bit j of byte f2 leaves the same
    residual as flipping bits i2 and j2 of the same bytes -- a codeword of the block check of weight four that lies across two
    characters, found by search over the lone-bit registers.  With those two bits wrong the pair search has two hits."""
    N = 8 * (e + 3)
    z = acars.ZTABLE[N - 1 - np.arange(8 * (e + 1))].reshape(-1, 8)
    pair = {}                                                        # z[f, i] ^ z[f, i2] of one byte -> (f, i, i2)
    for f in range(e):
        for i in range(8):
            for i2 in range(i + 1, 8):
                key = int(z[f, i] ^ z[f, i2])
                if key in pair and pair[key][0] != f:
                    g, j, j2 = pair[key]
                    return g, j, f, i, j2, i2
                pair.setdefault(key, (f, i, i2))
    raise AssertionError("no weight-four codeword across two characters below byte %d" % e)


# ---------------------------------------------------------------------------------------------------------------- crafted audio
UNIT = 1.0 / 4096.0                   # audio of k UNIT quantises to k


def as_audio(k):
    return np.asarray(k, dtype=np.float64) * UNIT


def integer_audio(blks, sps, starts, amp=1000, n=None, **kw):
    """integer audio: the synthesiser's envelope of the blocks at `sps` samples per bit, rounded to whole units"""
    return np.rint(acars.encode_audio(blks, sps * 2400.0, starts, amplitudes=float(amp), n=n, **kw)).astype(np.int64)


def text_block(chars, more=False):
    """a block whose end is 13 + chars (12 for chars None: no STX)"""
    text = None if chars is None else "".join(chr(65 + i % 26) for i in range(chars))
    return acars.block_bytes("2", "D-AIMA", None, "5Z", "2", text, more)


def block_ending_at(e, more=False):
    """a block's bytes whose ETX / ETB is byte e, 233 < e: the 220-character block with e - 233 more characters of text than a
    transmitter may send, and as much of the block check and DEL behind it as the 240 characters hold"""
    long = np.frombuffer(text_block(acars.TEXT_MAX), dtype=np.uint8)
    body = np.concatenate((long[:233], np.full(e - 233, 0x20, dtype=np.uint8), [acars.ETB if more else acars.ETX])).astype(np.uint8)
    bcs = acars.crc_bitwise(body.tobytes())
    return np.concatenate((body, [bcs & 0xFF, bcs >> 8, acars.DEL])).astype(np.uint8)[:acars.CHARS].tobytes()
