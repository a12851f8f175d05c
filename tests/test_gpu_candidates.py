"""The candidate list driver the burst decoders share (dd_candidates.h: the sync kernel's counts, k_scan_tops, k_cand_list) on more
than 256 workgroups, where k_scan_tops takes a second round of 256 counts and carries the first round's total into it: once over a
one-bit mask through dd_pocsag_candidates and once over a mask of four phases per byte through dd_adsb_candidates, against the NumPy
restatements.  Everything is integer behind the quantiser, so every comparison is exact equality.  The two tests without a device
check that the restatement alone passes where the device tests need passes."""
import ctypes as C
import functools

import numpy as np
import pytest

import _adsb as A
import _pocsag as T
from directdemod_amd import adsb, pocsag

SENT = np.int64(-0x5A5A5A5A5A5A5A5B)
SPARE = 16
TILE = 256


@pytest.fixture(scope="module")
def hip():
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


# ---------------------------------------------------------------------------------------------------------------- a one-bit mask
SPS, W, SLACK = 4.0, 3, 0
N = 257 * TILE + pocsag.reach(SPS, W) + 600
LAID = (5, 65536, 259 * TILE + 40)    # where a sync codeword is laid
WANTED = (5, 65535, 65536, 65537)     # starts that must pass: the last of workgroup 255, the first two of workgroup 256


@functools.lru_cache(maxsize=None)
def pocsag_case():
    """(integer audio, the mask bytes of its starts, its candidates): sync codewords as rectangular audio at 4 samples per bit.  With
    w = 3 a bit's window lies inside the bit for the start laid and the one before it, and holds two of its three samples for the
    start behind it, so the codeword laid at 65536 passes at 65535, 65536 and 65537 as well."""
    x = sum(T.sync_rect(4, t=t, n=N) for t in LAID)
    x.setflags(write=False)
    masks = pocsag.masks_host(T.as_audio(x), SPS, W, SLACK)
    masks.setflags(write=False)
    return x, masks, np.flatnonzero(masks & 1).astype(np.int64)


def pocsag_candidates(hip, cap):
    """dd_pocsag_candidates with `cap` places and SPARE sentinels behind them -> (rc, count, the places, the sentinels still whole)"""
    x = hip.DevArray.from_host(T.as_audio(pocsag_case()[0]))
    lst = hip.DevArray.from_host(np.full(cap + SPARE, SENT))
    count = C.c_int64(-1)
    rc = hip.lib().dd_pocsag_candidates(x.ptr, x.n, SPS, W, SLACK, lst.ptr, cap, C.byref(count), None)
    hip.sync()
    got = lst.to_host()
    return rc, count.value, got[:cap], bool(np.all(got[cap:] == SENT))


def test_the_restatement_passes_in_the_workgroups_meant():
    _, masks, want = pocsag_case()
    nb = -(-len(masks) // TILE)
    assert len(masks) == pocsag.n_starts(N, SPS, W) and nb > 257
    assert set(WANTED) <= set(want.tolist())
    assert {0, 255, 256, nb - 1} <= set((want // TILE).tolist())


@pytest.mark.gpu
def test_one_bit_mask_beyond_256_workgroups(hip):
    x, masks, want = pocsag_case()
    rc, count, got, whole = pocsag_candidates(hip, len(want) + 3)
    assert rc == 0 and count == len(want) and whole
    assert np.array_equal(got[:count], want) and np.all(got[count:] == SENT)
    dev = pocsag.masks_device(hip.DevArray.from_host(T.as_audio(x)), SPS, W, SLACK)
    assert len(dev) == N and np.array_equal(dev[:len(masks)], masks) and not dev[len(masks):].any()
    assert np.array_equal(np.flatnonzero(dev & 1), want)


@pytest.mark.gpu
def test_one_bit_mask_with_a_list_one_place_short(hip):
    want = pocsag_case()[2]
    cap = len(want) - 1
    rc, count, got, whole = pocsag_candidates(hip, cap)
    assert rc == hip.DD_ERR_INVALID and count == len(want) and whole
    assert np.array_equal(got, want[:cap])


# ---------------------------------------------------------------------------------------------------------------- four phases per byte
RATE, Q = 2000000, 4
SQUITTERS = (8, 255 * TILE + 20, 256 * TILE + 64, 257 * TILE + 108)          # the samples at which a squitter starts


@functools.lru_cache(maxsize=None)
def adsb_case():
    """(recording, its candidates): a squitter near the start and one in each of the workgroups 255, 256 and 257, 240 samples each"""
    frames = [A.F_CALLSIGN] * len(SQUITTERS)
    raw = adsb.encode(frames, RATE, [float(s) for s in SQUITTERS], n=SQUITTERS[-1] + adsb.reach(RATE) + 300)
    raw.setflags(write=False)
    return raw, adsb.candidates_host(adsb.power(raw), RATE, Q)


def test_the_restatement_passes_at_the_squitters():
    raw, want = adsb_case()
    assert -(-adsb.n_candidates(len(raw), RATE, Q) // Q) > 257 * TILE
    assert {s * Q for s in SQUITTERS} <= set(want.tolist())
    assert {0, 255, 256, 257} <= set((want // Q // TILE).tolist())


@pytest.mark.gpu
def test_multi_phase_mask_beyond_256_workgroups(hip):
    raw, want = adsb_case()
    iq = adsb.to_device(raw)
    cap = len(want) + 3
    lst = hip.DevArray.from_host(np.full(cap + SPARE, SENT))
    count = C.c_int64(-1)
    rc = hip.lib().dd_adsb_candidates(iq.ptr, iq.n, RATE, Q, lst.ptr, cap, C.byref(count), None)
    hip.sync()
    got = lst.to_host()
    assert rc == 0 and count.value == len(want)
    assert np.array_equal(got[:len(want)], want) and np.all(got[len(want):] == SENT)
