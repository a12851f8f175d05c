"""
CPU-side check of k_chain_decim_b's LDS image (dd_debug_decimb_lds_check: the kernel's own address functions, evaluated on the host).

A lane's block sums read its block in steps of eight samples -- the last step up to seven samples past the kept one, under zero taps.
The products run on the matrix pipe, where 0 x NaN is NaN: every cell such a step reads must hold a value the current row wrote (its
staged samples, the halo of the row before, the zeros behind its last staged sample), or zeros the launch wrote and no row overwrites.
A cell nothing wrote holds whatever the CU's LDS held before; a cell an earlier row wrote holds one of that row's samples.  Either one
carries a non-finite value into outputs that do not depend on it.
"""
import ctypes as C

import pytest

from directdemod_amd import _hip

W = 2048


def _check(K, M, phi):
    out = (C.c_int64 * 12)()
    _hip.check(_hip.lib().dd_debug_decimb_lds_check(K, M, phi, out), "dd_debug_decimb_lds_check")
    keys = ("unwritten", "stale", "rmin", "rmax", "img", "wmax", "pmax", "rows", "ng", "amin", "amax", "pad")
    return dict(zip(keys, list(out)))


def _taps_per_NI(M):
    """one tap count per number of block sums NI = ceil(K / M) in 1 .. 8 that the kernel takes (K <= 256): K = NI M for even NI, (NI - 1) M + 1
    for odd NI > 1 -- both accumulator sets (NI > 4), and for NI = 5 the second set's first non-zero tap inside the block (j1lo > 0)"""
    ks = []
    for NI in range(1, 9):
        K = min(NI * M if NI % 2 == 0 else max((NI - 1) * M + 1, M - 1), 256)
        if K >= 2 and -(-K // M) == NI:
            ks.append(K)
    return ks


def _orbit(M, phi):
    """the row phases a stream with first kept sample phi meets: every row starts W mod M later in the decimation grid"""
    seen, r = [], phi
    while r not in seen:
        seen.append(r)
        r = (r - W) % M
    return seen


@pytest.mark.parametrize("M", range(8, 66, 2))
def test_every_cell_a_block_sum_reads_was_written_by_its_own_row(M):
    """Every even M in 8..64, a tap count for every NI = ceil(K / M) in 1..8, every stream phase: no read of a cell nothing wrote (a), none of a
    sample an earlier row left behind (b), every read inside the image and every requested read inside the wave's LDS allocation."""
    ks = _taps_per_NI(M)
    assert [-(-K // M) for K in ks] == list(range(1, min(8, -(-256 // M)) + 1))
    for K in ks:
        NI = -(-K // M)
        for phi in range(M):
            c = _check(K, M, phi)
            case = (K, M, phi, c)
            assert c["pad"] == (1 if M % 4 == 0 else 0) and c["ng"] == (2 if NI > 4 else 1), case
            assert c["rows"] == 2 * (len(_orbit(M, phi)) + 2), case
            assert c["unwritten"] == 0 and c["amin"] == -1, case
            assert c["stale"] == 0, case
            assert 0 <= c["rmin"] and c["rmax"] < c["img"], case
            assert c["wmax"] < c["img"] and c["pmax"] < c["img"] + 32, case        # (32: the NCO group phasors behind the image)
            # the check reads what it should: the first block (it starts inside the halo) and the cells past the row's last kept sample
            assert c["rmin"] <= M + 4 and c["rmax"] >= W + M - 1, case


@pytest.mark.parametrize("phi", [26, 28, 30])
def test_padded_image_reads_past_the_last_staged_sample_only_cells_it_cleared(phi):
    """M = 32, K = 151 at the stream phases where the last block's final step runs past the row's last staged sample.  Before the zeros
    behind every staged row (dw_b_tail_zero) these reads hit cells nothing wrote: 12, 24, 36 reads of cells 2210 .. 2211, 2213, 2215 for
    phi = 26, 28, 30 (and likewise three phases each for M = 8, 16, 64, 15 of 40 for M = 40, 9 of 12 for M = 12, 15 of 20 for M = 20)."""
    c = _check(151, 32, phi)
    assert c["pad"] == 1 and c["ng"] == 2
    assert c["rmax"] >= 2211 + (phi - 26)              # the reads of those cells are still there ...
    assert c["unwritten"] == 0 and c["stale"] == 0     # ... of cells the row cleared
    assert c["rmax"] < c["img"]


def test_layout_check_refuses_what_the_block_sum_kernel_does_not_take():
    out = (C.c_int64 * 12)()
    lib = _hip.lib()
    for K, M, phi in ((151, 33, 0), (151, 6, 0), (257, 34, 0), (255, 8, 0), (100, 10, 0)):     # (K > 8 M: the window kernel)
        assert lib.dd_debug_decimb_lds_check(K, M, phi, out) == _hip.DD_ERR_UNSUPPORTED, (K, M)
    with pytest.raises(ValueError):
        _hip.check(lib.dd_debug_decimb_lds_check(151, 32, 32, out), "phase out of range")
