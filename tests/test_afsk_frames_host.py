"""AFSK1200 frame logic on the host (no GPU): decode_afsk1200's static helpers, fcs_crc16 and the restatements the GPU tests
compare against, all against what the reference's own getMsg run recorded (tests/golden/afsk_frames_*.npz, gen_golden.py
--afsk-frames)."""
import os

import numpy as np
import pytest

import _ax25
from directdemod_amd import decode_afsk1200 as dmod

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D = dmod.decode_afsk1200


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def _accepted(bs, flags):
    """the reference's pair loop over bitstream, with the host helpers"""
    marks = D.find_bit_stuffing(bs)
    out = []
    for f in range(len(flags) - 1):
        bits = D.reduce_stuffed_bit(bs[flags[f] + 8:flags[f + 1]], marks[flags[f] + 8:flags[f + 1]])
        msg = bits[:-16]
        if len(bits) % 8 == 0 and len(msg) > 128 and "".join(map(str, bits[-16:])) == dmod.fcs_crc16("".join(map(str, msg))):
            out.append((f, int(flags[f]), np.array(msg, dtype=np.int8)))
    return out


@pytest.mark.parametrize("name", ["afsk_frames_a.npz", "afsk_frames_b.npz"])
def test_helpers_reproduce_the_reference_frames(name):
    g = _load(name)
    bs = D.decode_nrzi(g["nrzi_sign"])
    assert np.array_equal(np.array(bs, dtype=np.int8), g["bitstream"])
    b = np.asarray(bs)
    flags = [k for k in range(len(b) - 8) if tuple(b[k:k + 8]) == dmod.FLAG]
    assert np.array_equal(flags, g["bit_startflag"])
    acc = _accepted(list(bs), flags)
    assert [a[0] for a in acc] == g["frame_flag"].tolist() and [a[1] for a in acc] == g["frame_start"].tolist()
    got_bits = np.concatenate([a[2] for a in acc])
    assert np.array_equal(got_bits, g["frame_bits"])
    # bits_to_msg's information field is what the reference printed
    infos = [D.bits_to_msg(a[2].tolist()) for a in acc]
    for s in infos:
        assert ("information:\t " + s + "\n") in str(g["stdout"])
    assert str(g["msg"]) == (dmod.MSG if acc else "") and int(g["useful"]) == (1 if acc else 0)


def test_fixture_a_rejects_the_corrupted_frame():
    g = _load("afsk_frames_a.npz")
    _, _, _, fb = _ax25.fixture_a()
    texts = [D.bits_to_msg([(byte >> j) & 1 for byte in f[:-2] for j in range(8)]) for f in fb]
    printed = str(g["stdout"])
    assert len(g["frame_flag"]) == 3 and texts[2] not in [t for t in texts[:2] + texts[3:]]
    assert all(("information:\t " + t) in printed for t in (texts[0], texts[1]))
    assert ("information:\t " + texts[2]) not in printed


def test_fcs_crc16_matches_the_reference():
    g = _load("afsk_frames_a.npz")
    offs = np.concatenate([[0], np.cumsum(g["crc_lens"])])
    for k, want in enumerate(g["crc_values"]):
        bits = g["crc_bits"][offs[k]:offs[k + 1]]
        assert dmod.fcs_crc16("".join(map(str, bits))) == str(want)


def test_helper_quirks():
    assert D.decode_nrzi([]) == [1] and D.decode_nrzi([-1.0]) == [1]
    assert D.decode_nrzi([1.0, np.nan, np.nan, 1.0, 1.0, -1.0]) == [1, 0, 0, 0, 1, 0]
    # a run of exactly five ones marks the next bit; the count goes on after a marked 1
    m = D.find_bit_stuffing([1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1])
    assert m.tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 2]
    assert D.reduce_stuffed_bit([1, 0, 1], [0, 1, 0]) == [1, 1]
    # fewer than two bytes after the address field: empty info instead of the reference's IndexError
    addr = [(0x82 >> j) & 1 for j in range(8)] + [(0x83 >> j) & 1 for j in range(8)]
    assert D.bits_to_msg(addr + [(0x03 >> j) & 1 for j in range(8)]) == ""
    assert dmod._fields(bytes([0x82, 0x83, 0x03, 0xF0]) + b"hi") == ("AA", "", "", "0x3", "0xf0", "hi")


def test_numpy_mean_model():
    rng = np.random.default_rng(3)
    for _ in range(3000):
        n = int(rng.integers(1, 129))
        x = rng.standard_normal(n + 3) * 10.0 ** rng.integers(-3, 4)
        s = int(rng.integers(0, 3))
        assert _ax25.np_mean_model(x[s:s + n]) == np.mean(x[s:s + n])


@pytest.mark.parametrize("name", ["afsk_frames_a.npz", "afsk_frames_b.npz"])
def test_peak_machine_restatement_reproduces_the_reference(name):
    g = _load(name)
    y = np.abs(g["edge_sums"].astype(np.float64) / (22050 // 1200))
    mx, mn = _ax25.peakdetect_host(y, int(g["pd_lookahead"]))
    assert [p for p, _ in mx] == g["pd_max_x"].tolist() and [v for _, v in mx] == g["pd_max_y"].tolist()
    assert [p for p, _ in mn] == g["pd_min_x"].tolist() and [v for _, v in mn] == g["pd_min_y"].tolist()


def test_bit_restatement_reproduces_the_reference_bits():
    """the fixture's NRZI signs from its peaks; the binary filter itself is not stored, so only the slicer's integer logic is checked
    here (lengths and the flag list); the means are bit-exact on the device against NumPy (tests/test_gpu_afsk_frames.py)"""
    g = _load("afsk_frames_a.npz")
    px = g["pd_max_x"].astype(np.int64)
    rep = np.round(np.diff(px) / (22050 / 1200))
    assert int(rep.sum()) == len(g["bitstream"])
    info, raws = _ax25.frames_host(g["bitstream"], D.find_bit_stuffing(g["bitstream"]), g["bit_startflag"])
    assert np.nonzero(info[:, 1])[0].tolist() == g["frame_flag"].tolist()
