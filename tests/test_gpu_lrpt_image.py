"""The image packets' payload on the device (dd_lrpt_jpeg, lrpt.jpeg_decode / image) against lrpt.py's NumPy restatement of DESIGN.md
section 4.16, and decode_meteorm2.getImage / getChannel / imageInfo end to end.  Every quantity is an integer and every comparison is
exact.  A packet is one wave, so the shapes are packets that take different ways through the kernel -- flat, dense, with runs of
sixteen, failing in each defined way, empty -- side by side in one call, and payloads longer than the kernel's 256-byte window."""
import itertools

import numpy as np
import pytest

import _jpeg
import _rs
from directdemod_amd import lrpt

pytestmark = pytest.mark.gpu

PITCH, STRIP = 112, 896


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _call(hip, data, offsets, q, dst, pitch, out):
    """dd_lrpt_jpeg over host arrays -> (out's bytes after the call, mcus); `out` is the output's initial content"""
    n = len(offsets) - 1
    d = hip.DevArray.from_host(np.frombuffer(bytes(data) or b"\0", dtype=np.uint8))
    o = hip.DevArray.from_host(out)
    m = hip.DevArray.from_host(np.full(n + 4, -77, dtype=np.int32))
    offsets, q, dst = np.asarray(offsets, dtype=np.int64), np.asarray(q, dtype=np.uint8), np.asarray(dst, dtype=np.int64)
    assert len(q) == n and len(dst) == n and offsets[-1] <= len(data)
    assert n == 0 or dst.max() + 7 * pitch + 112 <= len(out)
    hip.check(hip.lib().dd_lrpt_jpeg(d.ptr, offsets.ctypes.data, q.ctypes.data, dst.ctypes.data, n, pitch, o.ptr, m.ptr, None), "dd_lrpt_jpeg")
    mcus = m.to_host()
    assert np.all(mcus[n:] == -77)
    return o.to_host(), mcus[:n]


def _want(payloads, q):
    """the restatement: (strips uint8[n, 8, 112], zero from the first failed block on; mcus)"""
    strips = np.zeros((len(payloads), 8, PITCH), dtype=np.uint8)
    mcus = np.zeros(len(payloads), dtype=np.int32)
    for i, (p, qi) in enumerate(zip(payloads, q)):
        coef, mcus[i] = lrpt.jpeg_blocks_np(p)
        if mcus[i]:
            strips[i, :, :8 * mcus[i]] = _jpeg.strip_of(lrpt.idct_np(coef[:mcus[i]], lrpt.quantiser(qi)))
    return strips, mcus


def _both(hip, payloads, q, data=None):
    """packets side by side in a zeroed output of pitch 112, held to the restatement; `data`: what lies in memory (by default the
    payloads back to back), of which packet i is the range that starts where the payloads before it end"""
    n = len(payloads)
    q = [q] * n if np.isscalar(q) else list(q)
    offsets = np.concatenate(([0], np.cumsum([len(p) for p in payloads]))).astype(np.int64)
    got, mcus = _call(hip, b"".join(payloads) if data is None else data, offsets, q, STRIP * np.arange(n), PITCH,
                      np.zeros(max(n, 1) * STRIP, dtype=np.uint8))
    strips, want = _want(payloads, q)
    assert np.array_equal(mcus, want), (mcus.tolist(), want.tolist())
    assert np.array_equal(got[:n * STRIP].reshape(n, 8, PITCH), strips)
    return strips, want


def _noise_payload(rng, q, sigma=60.0):
    return _jpeg.encode_strip(np.clip(128 + sigma * rng.standard_normal((8, PITCH)), 0, 255).astype(np.uint8), q)[0]


def _flat(levels):
    w, pred = _jpeg.Writer(), 0
    for v in levels:
        w.dc(v - pred).eob()
        pred = v
    return w


def _symbol_lengths(coef):
    """the code lengths of the AC symbols _jpeg.write_block emits for one block"""
    z = [int(coef[lrpt.ZIGZAG[k]]) for k in range(64)]
    out, run = [], 0
    for k in range(1, 64):
        if z[k] == 0:
            run += 1
            continue
        out += [_jpeg.AC[0xF0][1]] * (run // 16) + [_jpeg.AC[((run % 16) << 4) | _jpeg.category(z[k])][1]]
        run = 0
    return out


# ------------------------------------------------------------------ packet counts, kinds of content
@pytest.mark.parametrize("n", [0, 1, 3, 65])
def test_packet_counts(hip, n):
    rng = _rng(300 + n)
    payloads = [_noise_payload(rng, 80, sigma=float(rng.integers(2, 60))) for _ in range(n)]
    _, mcus = _both(hip, payloads, 80)
    assert np.all(mcus == 14)


def test_no_packets_touches_nothing(hip):
    hip.check(hip.lib().dd_lrpt_jpeg(None, None, None, None, 0, 112, None, None, None))


def test_flat_strip(hip):
    payload = _flat([5] * 14).bytes()
    assert len(payload) <= 2 + 14 * 6 // 8 + 1                                   # one DC symbol and an end-of-block per block
    strips, mcus = _both(hip, [payload, _flat(range(-7, 7)).bytes()], 50)
    assert mcus.tolist() == [14, 14] and np.all(strips[0] == 128 + 10) and len(np.unique(strips[1])) == 14


def test_noise_strip_at_q100(hip):
    rng = _rng(310)
    payload = _noise_payload(rng, 100)
    coef, mcus = lrpt.jpeg_blocks_np(payload)
    assert mcus == 14 and len(payload) > 1024 and np.count_nonzero(coef[:, 63]) >= 3      # blocks that end at position 63
    # sparse large coefficients: the 16-bit codes, runs beyond fifteen
    sparse = np.where(rng.random((14, 64)) < 0.12, rng.integers(-1023, 1024, size=(14, 64)), 0)
    sparse[:, 0] = rng.integers(-1000, 1000, 14)
    sparse[3, 63], sparse[9, 63], sparse[5, 1:] = 700, -1, 0
    lengths = sum((_symbol_lengths(c) for c in sparse), [])
    assert lengths.count(16) >= 20 and lengths.count(11) >= 1
    _both(hip, [payload, _jpeg.encode(sparse)], [100, 100])
    _both(hip, [_jpeg.encode(sparse)], 21)                                              # the clamp to 12 bits after dequantisation


def test_hand_built_runs_of_sixteen_and_dc_category_11(hip):
    w = _jpeg.Writer()
    w.dc(2047).zrl().zrl().zrl().ac(14, -5)                       # position 63 after three runs of sixteen: no end-of-block
    w.dc(-2047).zrl().ac(0, 1023).eob()                           # back to 0
    w.dc(-2047).ac(15, 1).zrl().ac(0, -1).zrl().eob()             # a run of sixteen before an end-of-block, k = 50
    w.dc(2047).zrl().zrl().zrl().ac(14, 1)
    for m in range(10):
        w.dc((-1) ** m * 1024).ac(m, m + 1).eob()
    payload = w.bytes()
    coef, mcus = lrpt.jpeg_blocks_np(payload)
    assert mcus == 14 and coef[:4, 0].tolist() == [2047, 0, -2047, 0] and coef[0, 63] == -5 and coef[1, lrpt.ZIGZAG[17]] == 1023
    for q in (100, 50, 0):
        _both(hip, [payload], q)


@pytest.mark.parametrize("q", [0, 20, 21, 49, 50, 100, 255])
def test_quality_factors(hip, q):
    rng = _rng(320 + q)
    _, mcus = _both(hip, [_noise_payload(rng, q), _noise_payload(rng, q, sigma=8.0)], q)
    assert mcus.tolist() == [14, 14]


# ------------------------------------------------------------------ failures
def _good(rng, blocks=14):
    """a valid stream of `blocks` blocks -> (writer, the bit at which each block ends)"""
    w, ends, pred = _jpeg.Writer(), [], 0
    coef = np.where(rng.random((blocks, 64)) < 0.3, rng.integers(-40, 41, size=(blocks, 64)), 0)
    coef[:, 63] = 0
    for c in coef:
        pred = _jpeg.write_block(w, c, pred)
        ends.append(len(w))
    return w, ends


def test_truncations(hip):
    rng = _rng(330)
    w, ends = _good(rng)
    full = w.bytes()
    # a cut at every byte of the stream: in the middle of codes, of values' bits, and wherever a block happens to end; what lies
    # behind the cut in memory completes the packet validly, so a read past the packet's end shows as mcus = 14
    cuts = list(range(len(full)))
    payloads = [full[:c] for c in cuts]
    strips, want = _want(payloads, [70] * len(cuts))
    assert want.tolist() == [sum(e <= 8 * c for e in ends) for c in cuts] and want.max() == 13 and lrpt.jpeg_blocks_np(full)[1] == 14
    # each packet in a call of its own range of the one full stream
    for group in (cuts[:7], cuts[len(cuts) // 2:len(cuts) // 2 + 7], cuts[-7:]):
        for c in group:
            got, mcus = _call(hip, full, [0, c], [70], [0], PITCH, np.zeros(STRIP, dtype=np.uint8))
            assert mcus[0] == want[c] and np.array_equal(got.reshape(8, PITCH), strips[c]), c
    # and all of them in one call, back to back: each one's successor is what lies behind it
    _both(hip, payloads, 70)


def test_truncation_exactly_at_a_blocks_end(hip):
    # blocks whose ends fall on byte boundaries: fewer than 14 blocks and not a bit more
    w = _jpeg.Writer()
    for m in range(9):
        w.dc(1 if m == 0 else 0).ac(0, 1)                          # 3 or 2 bits, then 2 + 1 bits
        while len(w) % 8 != 4:
            w.ac(0, 1)
        w.eob()                                                    # 4 bits: the block ends with the byte
        assert len(w) % 8 == 0
    payload = w.bytes()
    tail = _flat([1] * 5).bytes()                                  # five more blocks lie behind it in memory
    assert lrpt.jpeg_blocks_np(payload)[1] == 9 and lrpt.jpeg_blocks_np(payload + tail)[1] == 14
    got, mcus = _call(hip, payload + tail, [0, len(payload)], [50], [0], PITCH, np.zeros(STRIP, dtype=np.uint8))
    strips, want = _want([payload], [50])
    assert mcus.tolist() == [9] and np.array_equal(got.reshape(8, PITCH), strips[0]) and not got.reshape(8, PITCH)[:, 72:].any()


def test_invalid_streams(hip):
    rng = _rng(340)
    head, _ = _good(rng, 4)

    def after(extend):
        w = _jpeg.Writer()
        w.bits = list(head.bits)
        extend(w)
        return w.bytes() + b"\xff" * 8
    cases = [after(lambda w: w.dc(1).raw(0xFFFF, 16)),                                  # sixteen ones: no such code
             after(lambda w: w.raw(0x1FF, 9)),                                          # nor a DC code of nine ones
             after(lambda w: w.dc(1).ac(3, 1).zrl().zrl().zrl().ac(11, 1)),             # 5 + 48 + 11 = 64: a run past 63
             after(lambda w: w.dc(1).zrl().zrl().zrl().zrl()),                          # k = 65 after a run of sixteen
             after(lambda w: w.dc(1).zrl().zrl().zrl().ac(15, 1))]                      # 49 + 15 = 64
    # (size 0 with a run other than 0 and 15 is a failure by definition; no code of the table carries such a symbol)
    strips, mcus = _both(hip, cases, 60)
    assert mcus.tolist() == [4] * len(cases) and not strips[:, :, 32:].any() and strips[:, :, :32].any()


def test_good_failed_and_empty_in_every_order(hip):
    rng = _rng(350)
    good = _noise_payload(rng, 90)
    failed = _noise_payload(rng, 90)[:200]
    assert 0 < lrpt.jpeg_blocks_np(failed)[1] < 14
    for order in itertools.permutations((good, failed, b"")):
        _, mcus = _both(hip, list(order), 90)
        assert sorted(mcus.tolist()) == sorted([14, lrpt.jpeg_blocks_np(failed)[1], 0])


# ------------------------------------------------------------------ where the pixels go
def test_dst_minus_one_writes_nothing(hip):
    rng = _rng(360)
    payloads = [_noise_payload(rng, 70) for _ in range(3)]
    offsets = np.concatenate(([0], np.cumsum([len(p) for p in payloads])))
    got, mcus = _call(hip, b"".join(payloads), offsets, [70] * 3, [-1, 0, -1], PITCH, np.full(STRIP + 64, 0xA5, dtype=np.uint8))
    strips, want = _want(payloads, [70] * 3)
    assert mcus.tolist() == [14, 14, 14] and np.array_equal(got[:STRIP].reshape(8, PITCH), strips[1]) and np.all(got[STRIP:] == 0xA5)


def test_pitch_1568_touches_its_regions_only(hip):
    rng = _rng(370)
    payloads = [_noise_payload(rng, 70), _noise_payload(rng, 70)[:150], _noise_payload(rng, 70)]
    offsets = np.concatenate(([0], np.cumsum([len(p) for p in payloads])))
    where = [(0, 8 * 42), (0, 8 * 56), (8, 8 * 182)]                          # two side by side, one a strip below at the right edge
    plane = np.full((24, 1568), 0xA5, dtype=np.uint8)
    got, mcus = _call(hip, b"".join(payloads), offsets, [70] * 3, [r * 1568 + c for r, c in where], 1568, plane.ravel())
    strips, want = _want(payloads, [70] * 3)
    assert np.array_equal(mcus, want) and 0 < want[1] < 14
    for (r, c), s, m in zip(where, strips, want):
        plane[r:r + 8, c:c + 8 * m] = s[:, :8 * m]
    assert np.array_equal(got.reshape(24, 1568), plane)


def test_random_bytes(hip):
    rng = _rng(380)
    payloads = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(1, 301, 4096)]
    _, mcus = _both(hip, payloads, rng.integers(0, 256, 4096).tolist())
    assert mcus.max() >= 2 and mcus.min() == 0


def test_payloads_beyond_the_window(hip):
    # 14 dense blocks at q = 100 are several refills of the 256 staged bytes; streams that end right at and around a refill
    rng = _rng(390)
    full = _noise_payload(rng, 100)
    assert len(full) > 1024
    _both(hip, [full[:n] for n in (251, 252, 253, 255, 256, 257, 259, 260, 261, 508, 512, 516)] + [full], 100)


def test_bad_arguments(hip):
    d = hip.DevArray.from_host(np.zeros(16, dtype=np.uint8))
    out = hip.DevArray(STRIP, np.uint8)
    m = hip.DevArray(4, np.int32)
    off, q, dst = np.array([0, 4], dtype=np.int64), np.array([50], dtype=np.uint8), np.array([0], dtype=np.int64)
    good = (d.ptr, off.ctypes.data, q.ctypes.data, dst.ctypes.data, 1, 112, out.ptr, m.ptr)
    hip.check(hip.lib().dd_lrpt_jpeg(*good, None))
    down = np.array([4, 0], dtype=np.int64)
    bad = [good[:4] + (-1,) + good[5:], good[:5] + (111,) + good[6:], (d.ptr, down.ctypes.data) + good[2:]]
    bad += [good[:i] + (None,) + good[i + 1:] for i in (0, 1, 2, 3, 6, 7)]
    for args in bad:
        with pytest.raises(ValueError):
            hip.check(hip.lib().dd_lrpt_jpeg(*args, None))
    with pytest.raises(ValueError):
        lrpt.jpeg_decode([b"\x00"], [50], [8], out, 112)                      # the strip would end past the output
    with pytest.raises(ValueError):
        lrpt.jpeg_decode([b"\x00"], [50, 60], [0], out, 112)


# ------------------------------------------------------------------ decode_meteorm2.getImage / getChannel / imageInfo
def test_image_end_to_end_case_c(hip):
    from directdemod_amd import decode_meteorm2, source
    raw, built, start, pic = _jpeg.case("c")
    obj = decode_meteorm2.decode_meteorm2(source.IQarray(raw, _jpeg.FS), 0)
    pkts, pinfo, rs = obj.getPackets, obj.packetInfo, obj.rsInfo
    img, info = obj.getImage, obj.imageInfo
    want_img, want_info = lrpt.image_np(pkts)
    assert img.dtype == np.uint8 and img.shape == want_img.shape and img.shape[1:] == (1568, 3) and np.array_equal(img, want_img)
    assert info.dtype == lrpt.IMAGE_INFO and np.array_equal(info, want_info)
    assert obj.getImage is img and obj.imageInfo is info
    for j, apid in enumerate((64, 65, 66)):
        assert np.array_equal(obj.getChannel(apid), img[:, :, j])
    with pytest.raises(ValueError):
        obj.getChannel(70)
    # against what was sent: which packets arrive follows from the frames' fates
    rows, state = _rs.match(built, rs["vcid"], rs["counter"], rs["ok"])
    arrived = _rs.expected(built, state)
    assert pkts == [p["data"] for p in arrived]
    assert state[_jpeg.FADE[0]] != "ok" and state[_jpeg.FLIP[0]] == "ok" and rs["errors"][rows.index(_jpeg.FLIP[0])].max() == 1
    whole = (len(raw) * 9 // 256 - (lrpt.FRAME_BITS - start)) // lrpt.FRAME_BITS           # frames 1 .. whole lie wholly in the recording
    sent = [p for p in built["packets"] if p["image"] is not None and p["first"] >= 1 and p["last"] is not None and p["last"] <= whole]
    here = [p for p in arrived if p["image"] is not None]
    assert len(sent) >= 120 and 3 * len(here) >= 2 * len(sent), (len(here), len(sent))
    assert [int(r["packet"]) for r in info] == [i for i, p in enumerate(arrived) if p["image"] is not None]
    first = here[0]["image"][1]
    want = np.zeros((8 * (max(p["image"][1] for p in here) - first + 1), 1568, 3), dtype=np.uint8)
    for p in here:
        j, s, m = p["image"]
        coef, mcus = lrpt.jpeg_blocks_np(p["data"][20:])
        assert mcus == 14
        want[8 * (s - first):8 * (s - first) + 8, 8 * m:8 * m + 112, j] = _jpeg.strip_of(lrpt.idct_np(coef, lrpt.quantiser(60)))
    assert np.array_equal(img, want) and img.shape[0] >= 16
    assert [(int(r["apid"]), int(r["strip"]), int(r["mcun"])) for r in info] == [(64 + p["image"][0], p["image"][1] - first, p["image"][2]) for p in here]
    assert np.all(info["mcus"] == 14) and np.all(info["q"] == 60) and np.all(info["day"] == 7000)
    # the picture itself, to within the quantiser's steps, where it arrived; zero where it did not
    got = np.zeros(img.shape[:2] + (3,), dtype=bool)
    for p in here:
        j, s, m = p["image"]
        got[8 * (s - first):8 * (s - first) + 8, 8 * m:8 * m + 112, j] = True
    assert not img[~got].any() and (~got).any()
    sent_pic = pic[8 * first:8 * first + img.shape[0]].astype(np.int64)
    assert np.abs(img.astype(np.int64) - sent_pic)[got].max() <= int(lrpt.quantiser(60).sum())
    # the sequence counter wraps inside the recording and a telemetry packet per cycle is passed over
    counts = [lrpt.packet_header(p)["count"] for p in pkts]
    assert max(counts) > 16000 and min(counts) < 100 and any(lrpt.packet_header(p)["apid"] == 70 for p in pkts)
    for k in ("lrpt_jpeg", "lrpt_image_host", "lrpt_rs", "lrpt_packets"):
        assert obj.timings[k] >= 0.0
    # the earlier layers are what they were
    fixed, errors = lrpt.rs_frames_np(obj.getFrames)
    assert np.array_equal(obj.getVCDUs, fixed[:, :892]) and obj.getPackets is pkts and obj.packetInfo is pinfo


def test_random_packets_case_b(hip):
    from directdemod_amd import decode_meteorm2, source
    raw, _, _ = _rs.case("b")
    obj = decode_meteorm2.decode_meteorm2(source.IQarray(raw, _rs.FS), 0)
    pkts = obj.getPackets
    img, info = obj.getImage, obj.imageInfo
    want_img, want_info = lrpt.image_np(pkts)
    assert np.array_equal(img, want_img) and np.array_equal(info, want_info) and img.shape[1:] == (1568, 3)
    # its packets have no secondary header: none is an image packet; with the flag set on, their random bytes are payloads
    assert len(info) == 0 and img.shape[0] == 0
    flagged = [bytes([p[0] | 0x08]) + p[1:14] + bytes([14 * (p[14] % 14)]) + p[15:] for p in pkts]
    img, info = lrpt.image(flagged, apids=(64, 65, 68))
    want_img, want_info = lrpt.image_np(flagged, apids=(64, 65, 68))
    assert len(info) >= 1 and np.array_equal(info, want_info) and np.array_equal(img, want_img)
