"""What the two AIS test files share: published sentences with their published decodes, the recording of the end-to-end tests, and
builders of crafted audio whose quantised values are chosen integers."""
import functools
import math

import numpy as np

from directdemod_amd import ais

# (sentences, type, mmsi, expected fields); positions are held to 1e-6 degree by the tests
VECTORS = [
    (["!AIVDM,1,1,,B,177KQJ5000G?tO`K>RA1wUbN0TKH,0*5C"], 1, 477553000,
     {"status": 5, "sog": 0.0, "lon": -122.345833, "lat": 47.582833, "cog": 51.0, "heading": 181, "second": 15}),
    (["!AIVDM,1,1,,A,13u?etPv2;0n:dDPwUM1U1Cb069D,0*24"], 1, 265547250,
     {"rot": -8, "sog": 13.9, "lon": 11.832977, "lat": 57.660353, "cog": 40.4, "heading": 41, "second": 53}),
    (["!AIVDM,1,1,,B,15NG6V0P01G?cFhE`R2IU?wn28R>,0*05"], 1, 367380120,
     {"rot": -128, "sog": 0.1, "lon": -122.404333, "lat": 37.806948, "cog": 245.2, "heading": None, "second": 59}),
    (["!AIVDM,1,1,,A,403OviQuMGCqWrRO9>E6fE700@GO,0*4D"], 4, 3669702,
     {"year": 2007, "month": 5, "day": 14, "hour": 19, "minute": 57, "second": 39, "lon": -76.352362, "lat": 36.883767}),
    (["!AIVDM,2,1,3,B,55P5TL01VIaAL@7WKO@mBplU@<PDhh000000001S;AJ::4A80?4i@E53,0*3E", "!AIVDM,2,2,3,B,1@0000000000000,2*55"], 5, 369190000,
     {"imo": 6710932, "callsign": "WDA9674", "shipname": "MT.MITCHELL", "shiptype": 99, "to_bow": 90, "to_stern": 90, "to_port": 10,
      "to_starboard": 10, "eta_month": 1, "eta_day": 2, "eta_hour": 8, "eta_minute": 0, "draught": 6.0, "destination": "SEATTLE"}),
    (["!AIVDM,1,1,,A,B52K>;h00Fc>jpUlNV@ikwpUoP06,0*4C"], 18, 338087471,
     {"sog": 0.1, "lon": -74.072132, "lat": 40.68454, "cog": 79.6, "heading": None, "second": 49}),
    (["!AIVDM,1,1,,A,H42O55i18tMET00000000000000,2*6D"], 24, 271041815, {"partno": 0, "shipname": "PROGUY"}),
    (["!AIVDM,1,1,,A,H42O55lti4hhhilD3nink000?050,0*40"], 24, 271041815,
     {"partno": 1, "shiptype": 60, "vendorid": "1D00014", "callsign": "TC6163", "to_bow": 0, "to_stern": 15, "to_port": 0,
      "to_starboard": 5}),
]
NBITS = [168, 168, 168, 168, 424, 168, 160, 168]


def payload_bits(i):
    return ais.from_nmea(VECTORS[i][0])[0]


def payloads():
    """the eight messages as bytes"""
    return [np.packbits(payload_bits(i)).tobytes() for i in range(len(VECTORS))]


def channel_of(i):
    return VECTORS[i][0][0].split(",")[4]


# ---------------------------------------------------------------------------------------------------------------- the recording
FS = 240000
OFFSETS = {"A": -25000.0, "B": 25000.0}
AMPLITUDE, SIGMA = 50.0, 8.0          # Eb / N0 = A^2 fs / (2 sigma^2 9600) = 488 = 26.9 dB


def ebn0_db(amplitude, sigma, fs):
    return 10.0 * math.log10(amplitude ** 2 * fs / (2.0 * sigma ** 2 * ais.BAUD))


@functools.lru_cache(maxsize=None)
def recording():
    """(uint8[N, 2] at 240 kS/s, the burst starts): the eight messages 35 ms apart, each on the channel its sentence names, with
    carrier errors within +-500 Hz, at an Eb / N0 of 26.9 dB"""
    rng = np.random.default_rng(31)
    starts = 2000.7 + np.arange(8) * FS * 0.035 + rng.uniform(0.0, 1.0, 8)
    chans = [OFFSETS[channel_of(i)] for i in range(8)]
    raw = ais.encode(payloads(), FS, starts, chans, AMPLITUDE, SIGMA, seed=32, carrier_offsets=rng.uniform(-500.0, 500.0, 8))
    raw.setflags(write=False)
    return raw, starts


# ---------------------------------------------------------------------------------------------------------------- crafted audio
UNIT = math.pi / 1048576.0            # audio of k UNIT quantises to k (test_ais_host checks that)
TRAIN16 = [0, 1] * 8                  # the last 16 training bits


def frame_raw(message, extra=()):
    """the raw bits behind the start flag for a message of whole bytes: the stuffed message, `extra` bits and FCS, the end flag"""
    data = bytes(message)
    fcs = ais.crc(data)
    stream = np.unpackbits(np.frombuffer(data + bytes((fcs & 0xFF, fcs >> 8)), dtype=np.uint8), bitorder="little")
    return np.concatenate((ais.stuff(np.concatenate((stream, np.array(extra, dtype=np.uint8)))), ais.FLAG)).astype(np.uint8)


def rect(raw_bits, sps, t=0, amp=1000, level=1, tail=8, n=None):
    """(integer audio, the start t): rectangular levels of +-amp, `sps` (an integer) samples per bit, for the 16 training bits from
    sample t on, the start flag, the raw bits and `tail` zeros bits; cut or zero-padded to n samples"""
    bits = np.concatenate((TRAIN16, ais.FLAG, np.asarray(raw_bits, dtype=np.uint8), np.zeros(tail, dtype=np.uint8)))
    lv = ais.nrzi(bits, -level)                                      # the first training bit changes the level to `level`
    body = np.repeat(lv * amp, int(sps)).astype(np.int64)
    x = np.concatenate((np.zeros(t, dtype=np.int64), body))
    if n is not None:
        x = np.concatenate((x, np.zeros(max(0, n - len(x)), dtype=np.int64)))[:n]
    return x


def as_audio(k):
    return np.asarray(k, dtype=np.float64) * UNIT


def message_with_stuffed_length(target, seed=0):
    """a message whose stuffed bits with FCS number exactly `target`: mostly zero bytes, a seeded few varied"""
    rng = np.random.default_rng(seed)
    for stuffs in range(0, 64):
        if (target - stuffs) % 8:
            continue
        L = (target - stuffs) // 8 - 2
        for _ in range(400):
            m = np.zeros(L, dtype=np.uint8)
            m[:4] = rng.integers(0, 256, 4)
            m[4:4 + stuffs] = 0x1F
            if len(frame_raw(m.tobytes())) - 8 == target:
                return m.tobytes()
    raise AssertionError("no message of %d stuffed bits" % target)


def tie_cases():
    """per template bit k: (integer audio whose bit k makes 16 v = S exactly, the same nudged up by one unit, whether the template
    has + at k).  sps 4, w 3: a bit's three samples are its own, its value sits on the middle one.  Levels +-240 give S = 0; a
    training bit changed from v to x moves S to x - v, so 16 x = S at x = -v / 15 = -+16; behind the training bits x = 0."""
    out = []
    for k in range(ais.TEMPLATE):
        v = np.where(ais.PLUS, 240, -240).astype(np.int64)
        x = -v[k] // 15 if k < ais.TRAINING else 0
        pair = []
        for step in (0, 1):
            u = v.copy()
            u[k] = x + step
            a = np.zeros(4 * ais.TEMPLATE + 8, dtype=np.int64)
            a[2 + 4 * np.arange(ais.TEMPLATE)] = u
            pair.append(a)
        out.append((pair[0], pair[1], bool(ais.PLUS[k])))
    return out
