"""The NumPy restatement of DESIGN.md section 4.16 (lrpt.py: huffman_tables, quantiser, jpeg_blocks_np, idct_np, image_header,
place, image_np) against known answers, against PIL's JPEG codec and against the encoder of _jpeg.py.  No GPU."""
import hashlib
import io

import numpy as np
import pytest

import _jpeg
from directdemod_amd import lrpt


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ------------------------------------------------------------------ known answers
def test_table_hashes_and_code_counts():
    assert hashlib.sha256(bytes(lrpt.DC_BITS) + lrpt.DC_VALUES).hexdigest().startswith("2f66814c875b5317")
    assert hashlib.sha256(bytes(lrpt.AC_BITS) + lrpt.AC_VALUES).hexdigest().startswith("a6283a08f5d97906")
    t = lrpt.huffman_tables()
    assert len(t["dc"]) == 12 and len(t["ac"]) == 162
    assert t["dc"][(2, 0)] == 0 and t["dc"][(9, 0x1FE)] == 11                  # T.81 table K.3
    assert t["ac"][(4, 0b1010)] == 0x00 and t["ac"][(11, 0x7F9)] == 0xF0 and t["ac"][(16, 0xFFFE)] == 0xFA   # T.81 table K.5
    # the decoder's table and the encoder's, built the other way round, are one assignment
    assert {v: (c, n) for (n, c), v in t["ac"].items()} == _jpeg.AC and {v: (c, n) for (n, c), v in t["dc"].items()} == _jpeg.DC


def test_transform_matrix_and_zigzag():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    m = np.rint(8192 * np.where(k == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * n + 1) * k * np.pi / 16))
    assert np.array_equal(lrpt.IDCT_M, m.astype(np.int64))
    assert np.abs(lrpt.IDCT_M).sum(axis=0).max() == 21641
    assert sorted(lrpt.ZIGZAG.tolist()) == list(range(64))
    assert lrpt.ZIGZAG[:10].tolist() == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and lrpt.ZIGZAG[-3:].tolist() == [55, 62, 63]


def test_quantiser_known_values():
    assert np.array_equal(lrpt.quantiser(50), lrpt.QUANT_STD)
    first_row = {0: [32, 22, 20, 32, 48, 80, 102, 122],            # F = 200: twice the standard table
                 20: [26, 18, 16, 26, 38, 64, 82, 98],             # F = 160: (160 S + 50) // 100
                 21: [38, 26, 24, 38, 57, 95, 121, 145],           # (100 S + 21) // 42
                 49: [16, 11, 10, 16, 24, 41, 52, 62],             # (100 S + 49) // 98
                 100: [1] * 8, 255: [1] * 8}
    last = {0: 198, 20: 158, 21: 236, 49: 101, 100: 1, 255: 1}
    for q, row in first_row.items():
        t = lrpt.quantiser(q)
        assert t.shape == (64,) and t[:8].tolist() == row and t[63] == last[q], q
    for q in range(256):
        assert lrpt.quantiser(q).min() >= 1


def test_extend():
    assert [lrpt.extend(v, 3) for v in range(8)] == [-7, -6, -5, -4, 4, 5, 6, 7]
    assert lrpt.extend(0, 0) == 0 and lrpt.extend(0, 11) == -2047 and lrpt.extend(2047, 11) == 2047


def test_idct_against_float64():
    rng = _rng(3)
    coef = rng.integers(-300, 301, size=(200, 64))
    coef[:, 8:] //= 8
    ones = np.ones(64, dtype=np.int64)
    got = lrpt.idct_np(coef, ones).astype(np.int64)
    c = _jpeg._C
    want = np.clip(np.floor(np.einsum("uy,nuv,vx->nyx", c, np.clip(coef, -2048, 2047).reshape(-1, 8, 8).astype(np.float64), c) + 128.5), 0, 255)
    assert np.abs(got - want).max() <= 1
    # the clamp: a coefficient times its step beyond 12 bits is held at -2048 / 2047
    big = np.zeros((2, 64), dtype=np.int64)
    big[0, 0], big[1, 0] = 5000, -5000
    assert np.array_equal(lrpt.idct_np(big, ones), lrpt.idct_np(np.clip(big, -2048, 2047), ones))


# ------------------------------------------------------------------ PIL's codec
def _pil_strip(strip, quality):
    """PIL's baseline JPEG of an 8 x 112 greyscale strip -> (its quantiser table row-major, its scan data un-stuffed, its decode)"""
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(strip, "L").save(buf, "JPEG", quality=quality, optimize=False)
    b = buf.getvalue()
    i, table, huff = 2, None, b""
    while True:
        assert b[i] == 0xFF
        marker, n = b[i + 1], (b[i + 2] << 8) | b[i + 3]
        if marker == 0xDB:
            assert b[i + 4] == 0 and n == 67
            table = np.zeros(64, dtype=np.int64)
            table[lrpt.ZIGZAG] = list(b[i + 5:i + 69])
        if marker == 0xC4:
            huff += b[i + 4:i + 2 + n]
        if marker == 0xDA:
            scan = b[i + 2 + n:b.rindex(b"\xff\xd9")].replace(b"\xff\x00", b"\xff")
            break
        i += 2 + n
    # the tables PIL writes are section 4.16's, byte for byte
    assert bytes([0x00]) + bytes(lrpt.DC_BITS) + lrpt.DC_VALUES in huff and bytes([0x10]) + bytes(lrpt.AC_BITS) + lrpt.AC_VALUES in huff
    return table, scan, np.asarray(Image.open(io.BytesIO(b)))


def test_against_pil():
    """40 strips (waves plus noise of sigma 0, 4, 16, 48), qualities 15..98, PIL's own quantiser tables: the restatement decodes
    PIL's scan data to within 1 grey level of PIL's decoder.  Measured with these seeds: max 1, 4.47 % of the pixels differ."""
    pytest.importorskip("PIL.Image")
    differ = total = 0
    x, y = np.arange(112)[None, :], np.arange(8)[:, None]
    for s in range(40):
        noise = (0, 4, 16, 48)[s % 4] * _rng(100 + s).standard_normal((8, 112))
        strip = np.clip(128 + 80 * np.sin(x / (5.0 + s) + s) * np.cos(y / 3.0) + noise, 0, 255).astype(np.uint8)
        table, scan, want = _pil_strip(strip, 15 + (s * 83) // 39)
        coef, mcus = lrpt.jpeg_blocks_np(scan)
        assert mcus == 14
        got = _jpeg.strip_of(lrpt.idct_np(coef, table))
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        assert d.max() <= 1, (s, int(d.max()))
        differ += int(np.sum(d > 0))
        total += d.size
    print("share of differing pixels: %.4f" % (differ / total))
    assert differ / total < 2 * 0.0447


# ------------------------------------------------------------------ encoder -> restatement
@pytest.mark.parametrize("q", [0, 20, 21, 49, 50, 80, 100, 255])
def test_round_trip(q):
    rng = _rng(200 + q)
    strip = np.clip(128 + 60 * rng.standard_normal((8, 112)), 0, 255).astype(np.uint8)
    payload, sent = _jpeg.encode_strip(strip, q)
    coef, mcus = lrpt.jpeg_blocks_np(payload)
    assert mcus == 14 and np.array_equal(coef, sent)
    pix = _jpeg.strip_of(lrpt.idct_np(coef, lrpt.quantiser(q)))
    # each coefficient is off by at most half its step, each pixel by no more than the steps' sum (and the transform's own rounding)
    assert np.abs(pix.astype(np.int64) - strip).max() <= int(lrpt.quantiser(q).sum())


def test_failures_and_ends():
    w = _jpeg.Writer()
    for m in range(14):
        w.dc(3 if m == 0 else 0).eob()
    good = w.bytes()
    coef, mcus = lrpt.jpeg_blocks_np(good)
    assert mcus == 14 and np.all(coef[:, 0] == 3) and not coef[:, 1:].any()
    assert lrpt.jpeg_blocks_np(b"")[1] == 0
    assert lrpt.jpeg_blocks_np(good[:-1])[1] < 14
    assert lrpt.jpeg_blocks_np(good + b"\xff\xff")[1] == 14                       # bits after the 14th block are ignored
    # a block whose coefficient at position 63 ends it needs no end-of-block
    w = _jpeg.Writer().dc(1).zrl().zrl().zrl().ac(14, -5)
    for m in range(13):
        w.dc(0).eob()
    coef, mcus = lrpt.jpeg_blocks_np(w.bytes())
    assert mcus == 14 and coef[0, 63] == -5 and coef[0, 0] == 1 and np.count_nonzero(coef[0]) == 2
    # (size 0 with a run other than 0 and 15 is a failure by definition; none of the 162 values is such a symbol, so no stream says it)
    assert not [v for v in lrpt.AC_VALUES if v & 15 == 0 and v >> 4 not in (0, 15)]
    for bad in (_jpeg.Writer().dc(1).zrl().zrl().zrl().zrl(),                     # k = 65 after a run of sixteen
                _jpeg.Writer().dc(1).zrl().zrl().zrl().ac(15, 1),                 # 49 + 15 = 64
                _jpeg.Writer().dc(1).raw(0xFFFF, 16)):                            # sixteen ones: no such code
        assert lrpt.jpeg_blocks_np(bad.bytes() + b"\xff" * 4)[1] == 0


# ------------------------------------------------------------------ image_header, place
def test_image_header():
    p = _jpeg.packet(65, 1234, b"\x12\x34", mcun=28, q=77, time=(7001, 123456789, 999))
    assert lrpt.image_header(p) == dict(apid=65, count=1234, day=7001, ms=123456789, us=999, mcun=28, q=77)
    assert len(_jpeg.packet(65, 0, b"\x00")) == 21 and lrpt.image_header(_jpeg.packet(65, 0, b"\x00")) is not None
    assert lrpt.image_header(_jpeg.packet(65, 0, b"")) is None                                    # 20 bytes
    assert lrpt.image_header(_jpeg.packet(70, 0, b"\x00" * 9)) is None                            # telemetry
    assert lrpt.image_header(_jpeg.packet(65, 0, b"\x00", secondary=0)) is None
    assert lrpt.image_header(_jpeg.packet(65, 0, b"\x00", mcun=15)) is None
    assert lrpt.image_header(_jpeg.packet(65, 0, b"\x00", mcun=196)) is None
    assert lrpt.image_header(_jpeg.packet(65, 0, b"\x00", mcun=182))["mcun"] == 182
    assert lrpt.image_header(_jpeg.packet(68, 0, b"\x00"), apids=(68, 64, 65))["apid"] == 68


def _heads(first_count, strips, apids=lrpt.IMAGE_APIDS):
    """the image headers of whole strip cycles from sequence count first_count, with (channel, strip, mcun) beside each"""
    out, count = [], first_count
    for s in range(strips):
        for j, apid in enumerate(apids):
            for m in range(0, 196, 14):
                out.append((dict(apid=apid, count=count & 0x3FFF, mcun=m), (j, s, m)))
                count += 1
        count += 1                                                             # the cycle's 43rd packet is not an image packet
    return out


def test_place_whole_cycles_and_a_wrap():
    hs = _heads(16384 - 50, 3)                                                 # the counter wraps inside the second cycle
    strips = lrpt.place([h for h, _ in hs])
    assert strips.tolist() == [s for _, (_, s, _) in hs]
    assert any(h["count"] == 0 for h, _ in hs)


def test_place_first_packet_is_channel_twos():
    hs = _heads(100, 3)[28 + 5:]                                               # channel 2's sixth packet comes first
    assert hs[0][1] == (2, 0, 70)
    assert lrpt.place([h for h, _ in hs]).tolist() == [s for _, (_, s, _) in hs]


def test_place_a_lost_strip_a_stray_count_and_a_duplicate():
    hs = _heads(7, 4)
    kept = [(h, w) for h, w in hs if w[1] != 2]                                # strip 2 is lost whole
    strips = lrpt.place([h for h, _ in kept])
    assert strips.tolist() == [s for _, (_, s, _) in kept] and 2 not in strips and strips.max() == 3
    stray = [dict(h) for h, _ in hs]
    stray[50]["count"] = (stray[50]["count"] + 5) & 0x3FFF                     # its base is 5 past a multiple of 43
    got = lrpt.place(stray)
    want = [s for _, (_, s, _) in hs]
    # the count is unwrapped packet by packet: the packet after the stray one steps back, which reads as a whole turn of 16384
    assert got[50] == -1 and got[:50].tolist() == want[:50] and np.all(got[51:] == -1) and 16384 % 43 != 0
    twice = [h for h, _ in hs]
    twice.insert(4, dict(twice[3]))                                            # the same count again at once: one (channel, strip, mcun)
    got = lrpt.place(twice)
    assert got[3] == -1 and got[4] == 0 and np.sum(got == -1) == 1 and got[5:].tolist() == want[4:]


def test_image_np_places_blocks_and_leaves_the_rest_zero():
    rng = _rng(5)
    pic = _jpeg.picture(rng, 2)
    sent = _jpeg.cycles(rng, pic, q=70, first_count=16384 - 60)
    pkts = [p["data"] for p in sent]
    lose = {4, 50, 85}
    img, info = lrpt.image_np([p for i, p in enumerate(pkts) if i not in lose])
    assert img.shape == (16, 1568, 3) and info.dtype == lrpt.IMAGE_INFO and len(info) == 84 - 2       # packet 85 is telemetry
    assert np.all(info["mcus"] == 14) and np.all(info["q"] == 70) and set(info["apid"]) == {64, 65, 66}
    want = np.zeros_like(img)
    for i, p in enumerate(sent):
        if p["image"] is None or i in lose:
            continue
        j, s, m = p["image"]
        coef, _ = lrpt.jpeg_blocks_np(p["data"][20:])
        want[8 * s:8 * s + 8, 8 * m:8 * m + 112, j] = _jpeg.strip_of(lrpt.idct_np(coef, lrpt.quantiser(70)))
    assert np.array_equal(img, want)
    assert not img[0:8, 8 * 56:8 * 70, 0].any() and img[0:8, 8 * 70:8 * 84, 0].any()                  # packet 4: channel 0, mcun 56
    assert np.abs(img[8:, :, 2].astype(np.int64) - pic[8:, :, 2]).max() <= int(lrpt.quantiser(70).sum())
    # nothing to place: 0 rows
    img, info = lrpt.image_np([_jpeg.packet(70, 1, b"\x00" * 30)])
    assert img.shape == (0, 1568, 3) and len(info) == 0
    # other APIDs in another order
    img2, info2 = lrpt.image_np(pkts, apids=(66, 64, 65), period=43)
    assert info2["strip"][0] == 0 and img2.shape[2] == 3
