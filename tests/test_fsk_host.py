"""The G3RUH 9600 baud FSK chain's definition on the CPU: the scrambler pair of directdemod_amd.fsk, the
Python restatement (tests/_fsk.py walk_host -> bits_host -> _ax25.frames_host) on synthesised audio, the branch counters of the
walk's named cases, and the state record against the header's numbers."""
import os
import re

import numpy as np
import pytest

import _ax25
import _fsk as fk
from directdemod_amd import fsk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_descramble_undoes_scramble_from_any_state_after_17_bits():
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.integers(0, 2, 500).astype(np.uint8)
    assert np.array_equal(fsk.descramble(fsk.scramble(x)), x)
    for tx, rx in ((0, 0x1FFFF), (0x1FFFF, 0), (0x0A5A5, 0x15A5A), (1, 1 << 16), (0x12345, 0x12345)):
        got = fsk.descramble(fsk.scramble(x, tx), rx)
        assert np.array_equal(got[17:], x[17:]), (tx, rx)
        assert np.array_equal(got, x) == (tx == rx), (tx, rx)          # (these pairs differ in a tap the first 17 bits read)
    assert np.array_equal(fsk.scramble(x), np.array(fk.scramble_host(x), dtype=np.uint8))
    assert len(fsk.scramble([])) == 0 and len(fsk.descramble([])) == 0


def test_scrambler_impulse_response_is_the_polynomial_s():
    """1 / (1 + x^12 + x^17) over GF(2): the coefficient of x^k is the number of ways to write k as an ordered sum of 12s and 17s,
    modulo 2.  Below 40: 0, 12, 17, 24 = 12 + 12, 34 = 17 + 17 and 36 = 12 + 12 + 12 have one way each; 29 = 12 + 17 = 17 + 12
    has two and cancels."""
    x = np.zeros(40, dtype=np.uint8)
    x[0] = 1
    ways = [1] + [0] * 39
    for k in range(1, 40):
        ways[k] = (ways[k - 12] if k >= 12 else 0) + (ways[k - 17] if k >= 17 else 0)
    assert [k for k in range(40) if ways[k] % 2] == [0, 12, 17, 24, 34, 36]
    assert np.nonzero(fsk.scramble(x))[0].tolist() == [0, 12, 17, 24, 34, 36]
    assert np.nonzero(fsk.descramble(x))[0].tolist() == [0, 12, 17]


def test_constants_and_state_are_the_header_s():
    txt = open(os.path.join(ROOT, "directdemod_amd", "csrc", "dd_fsk.h")).read()
    body = re.search(r"struct DDFskState \{(.*?)\};", txt, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    doubles = [n.strip() for m in re.findall(r"double ([^;]*);", body) for n in m.split(",")]
    ints = [n.strip() for m in re.findall(r"int64_t ([^;]*);", body) for n in m.split(",")]
    assert tuple(doubles) == fk.FLOAT_FIELDS and tuple(ints) == fk.INT_FIELDS
    assert fsk.STATE.names == fk.FLOAT_FIELDS + fk.INT_FIELDS
    size = int(re.search(r"static_assert\(sizeof\(DDFskState\) == (\d+)", txt).group(1))
    assert fsk.STATE.itemsize == size == 64
    assert [fsk.STATE.fields[f][1] for f in fsk.STATE.names] == list(range(0, 64, 8))
    assert int(re.search(r"#define DD_FSK_TILE (\d+)", txt).group(1)) == fk.TILE
    assert int(re.search(r"static_assert\(sizeof\(DDFskParams\) == (\d+)", txt).group(1)) == 8 * len(fsk.params(48000))
    st = fsk.state0()
    assert st.tobytes() == fk.state_struct(fk.start_state(), fsk.STATE).tobytes()
    for rate in (48000, 2048000 / 42, 19200, 614400):
        assert np.array_equal(fsk.params(rate), fk.params_array(fk.params(rate / 9600)))
    assert (fsk.GAIN, fsk.AM0, fsk.BAUDRATE) == (fk.G, fk.AM0, fk.BAUD)
    for rate in (19199, 614401, float("nan")):
        with pytest.raises(ValueError, match="9600"):
            fsk.params(rate)


@pytest.mark.parametrize("name", sorted(fk.CASES))
def test_named_cases_reach_their_branches(name):
    prm, x, st = fk.case(name)
    s, arr, cnt = fk.walk_host(x, 0, st, prm)
    for key in fk.CASES[name]["reaches"]:
        assert cnt[key] > 0, (key, cnt)
    assert len(arr["sym"]) == s["ctr"] == cnt["eye_events"] > 0
    assert np.all(np.isfinite(arr["sym"])) and np.all(np.isfinite(arr["tmu"])) and np.all(np.diff(arr["sidx"]) > 0)
    if name == "am_tiny":                                   # am stalls above 0: the guard is for a state that starts at 0
        assert cnt["am_guard"] == 0 and cnt["am_tiny"] == fk.CASES[name]["signal"]["zeros"]
    if name == "am_zero":
        assert cnt["am_guard"] == fk.CASES[name]["signal"]["zeros"]
    if name == "eye_run":
        assert cnt["back_to_back"] > 2 * fk.TILE


def test_tiny_am_stalls_instead_of_reaching_zero():
    """(am * 1023) / 1024 in round-to-nearest: from the smallest subnormal it rounds back up, from above it stops at 512 units"""
    for am0 in (5e-324, 1e-320, 1e-310):
        s, _, cnt = fk.walk_host(np.zeros(300000), 0, fk.start_state(am=am0), fk.params(5.0))
        assert cnt["am_guard"] == 0 and 0.0 < s["am"] <= am0
    assert fk.walk_host(np.zeros(300000), 0, fk.start_state(am=1e-310), fk.params(5.0))[0]["am"] == 512 * 5e-324


def test_events_cannot_be_two_tiles_apart():
    """P <= 64 and a finite timing: the gaps between eye events stay below P + 2 samples whatever the input does to the loop"""
    for P, seed in ((64.0, 1), (2.0, 2), (fk.P_FRAC, 3)):
        x = fk.signal(P, 20000, seed, amp=300.0, noise=64)
        _, arr, _ = fk.walk_host(x, 0, fk.start_state(), fk.params(P))
        assert np.diff(arr["sidx"]).max() <= P + 2


@pytest.fixture(scope="module")
def line():
    return fk.line_bits()


@pytest.mark.parametrize("P", [5.0, fk.P_FRAC, 4.032])
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("ppm", [100.0, -100.0])
def test_restatement_chain_recovers_the_frames(line, P, invert, ppm):
    bits, fb = line
    a = fk.audio(bits, P, 5, ppm=ppm, invert=invert, offset=0.1)
    s, arr, _ = fk.walk_host(a, 0, fk.start_state(), fk.params(P))
    r, b, marks, flags = fk.bits_host(arr["sym"])
    info, out = _ax25.frames_host(b, marks, flags)
    assert out == [f[:-2] for i, f in enumerate(fb) if i not in fk.BAD]
    assert abs(len(arr["sym"]) - len(bits)) <= 2 and s["overflow"] == 0
    # the mean period over the second half (the loop may move by up to a symbol while it pulls in): either end's sidx is a whole
    # sample within one of the symbol's instant, two samples over the span
    sidx = arr["sidx"][len(arr["sidx"]) // 2:]
    period = (sidx[-1] - sidx[0]) / (len(sidx) - 1)
    assert abs(period / P - 1.0 / (1.0 + ppm * 1e-6)) < 2.0 / (sidx[-1] - sidx[0])


def test_inversion_changes_no_bit(line):
    """the line is descrambled, then NRZI-decoded: an inverted discriminator flips every r, the three-term xor flips every d, and
    d[k] == d[k-1] is what it was -- but for the first 18 bits, which read zeros before the start"""
    bits, _ = line
    a = fk.audio(bits, 5.0, 6, sigma=0.0)
    sym = fk.walk_host(a, 0, fk.start_state(), fk.params(5.0))[1]["sym"]
    up, down = fk.bits_host(sym), fk.bits_host(-sym)
    assert np.array_equal(up[0], 1 - down[0]) and np.array_equal(up[1][18:], down[1][18:])


def test_bits_host_decodes_what_symbols_for_encodes():
    rng = np.random.Generator(np.random.PCG64(2))
    for n in (1, 2, 12, 13, 17, 18, 19, 300):
        b = rng.integers(0, 2, n).astype(np.int8)
        b[0] = 1
        r, got, marks, flags = fk.bits_host(fk.symbols_for(b))
        assert np.array_equal(got, b) and np.array_equal(fsk.descramble(r.astype(np.uint8))[1:] ^ fsk.descramble(r.astype(np.uint8))[:-1], 1 - b[1:])
    assert [len(v) for v in fk.bits_host(np.zeros(0))] == [0, 0, 0, 0]
