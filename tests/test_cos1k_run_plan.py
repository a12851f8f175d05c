"""
k_chain_cos1k's run map as host arithmetic (no GPU): how long the launch path makes a run and what dd_debug_cos1k_shape overrides
(dd_cosfir.hip: cos1k_run_rows, cos1k_shape).

DESIGN.md 4.2d, "Runs": runs of 8 rows dealt to the waves in turn (run j to wave j mod waves) once every wave gets at least two of
them (rows >= 16 waves), one run per wave below that.
"""
import ctypes as C

import numpy as np
import pytest

from directdemod_amd import _hip

RUN_ROWS = 8
RUNS_FROM = 16        # rows per wave from which runs are dealt


def _runs(nrows, nwaves):
    out = (C.c_int * 3)()
    _hip.check(_hip.lib().dd_debug_cos1k_runs(nrows, nwaves, out), "dd_debug_cos1k_runs")
    return tuple(out)


@pytest.fixture
def shape():
    def force(nwaves, run_rows):
        return _hip.lib().dd_debug_cos1k_shape(nwaves, run_rows)
    yield force
    assert force(0, 0) == 0


@pytest.mark.parametrize("log2n,s,align,ncu", [(26, 1, 0, 256), (26, 0, 7, 256), (25, 1, 0, 256), (24, 1, 0, 256), (20, 0, 15, 256), (25, 0, 0, 64), (12, 1, 0, 256)])
def test_the_plans_own_choice(log2n, s, align, ncu):
    """with no override: the headline's taps take the running-sum kernel, the plan's waves are kept, and the run length follows the
    rule DESIGN.md states (the 2^26-sample headline on 256 CUs walks runs; a 2^24-sample chunk does not)"""
    t = np.ascontiguousarray(np.hamming(255), dtype=np.float64)
    fam = C.c_int(-1)
    _hip.check(_hip.lib().dd_debug_chain_select(t.ctypes.data_as(C.POINTER(C.c_double)), 255, 1, _hip.DD_CHAIN_NCO | _hip.DD_CHAIN_FM, 0, None,
                                                C.byref(fam)), "dd_debug_chain_select")
    assert fam.value == _hip.DD_FAMILY_COS1K
    plan = (C.c_int * 4)()
    _hip.check(_hip.lib().dd_debug_cos1k_plan(1 << log2n, s, align, ncu, plan), "dd_debug_cos1k_plan")
    base, nrows, grid, nwaves = list(plan)
    want = RUN_ROWS if nrows >= RUNS_FROM * nwaves else 0
    assert _runs(nrows, nwaves) == (grid, nwaves, want)
    if (log2n, ncu) == (26, 256):
        assert want == RUN_ROWS
    if (log2n, ncu) == (24, 256):
        assert want == 0


def test_the_rule_at_its_threshold():
    for nwaves in (4, 40, 2048):
        assert _runs(RUNS_FROM * nwaves - 1, nwaves)[2] == 0
        assert _runs(RUNS_FROM * nwaves, nwaves)[2] == RUN_ROWS


def test_the_override_replaces_waves_and_run_length_and_goes_away(shape):
    assert shape(12, 3) == 0
    assert _runs(40, 40) == (3, 12, 3)
    assert _runs(1 << 16, 2048) == (3, 12, 3)
    assert shape(0, 2) == 0                                  # the plan's waves, runs of 2
    assert _runs(40, 40) == (10, 40, 2)
    assert shape(36, 0) == 0                                 # 36 waves, the rule's own run length for them
    assert _runs(40, 40) == (9, 36, 0)
    assert _runs(36 * RUNS_FROM, 40) == (9, 36, RUN_ROWS)
    assert shape(0, 0) == 0
    assert _runs(40, 40) == (10, 40, 0)
    for bad in ((5, 0), (-4, 0), (4, -1)):                   # whole workgroups of 4 waves only
        assert shape(*bad) != 0
    assert _runs(40, 40) == (10, 40, 0)                      # a refused call changes nothing
