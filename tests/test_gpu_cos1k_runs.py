"""
k_chain_cos1k's run map and output stores (dd_cosfir.hip), on chunks of a few dozen rows.

Runs of R rows dealt to the waves in turn need a 2^25-sample chunk before the launch path chooses them; dd_debug_cos1k_shape forces
the wave count and the run length, so that a 40-row chunk walks them on 4 .. 36 waves: a ragged last run, waves without a run,
workgroup counts that are no multiple of 8.  Which rows start a run depends on R alone, so at equal R the outputs must be the same
bytes whatever the wave count.  The stores of a row go through one helper per cache policy (a pointer, or a buffer resource over
the row with a 32-bit lane offset; the angles' write-through stores are of the second kind): every output must be written, and
nothing beside the outputs.

Reference: the float64 oracle over one stream of 40 * 1024 + 300 samples, built once per module as tests/test_gpu_cos1k_edges.py
builds its own.  Tolerances: those of tests/test_gpu_parity.py for this kernel, copied, not loosened.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import dd_oracle as O

pytestmark = pytest.mark.gpu

# tests/test_gpu_parity.py's constants for this kernel
FIR_TOL = 2e-6
FM_MAX = 1e-4        # |z| >= 1e-3 median
FM_WELL = 2e-5       # |z| >= 0.1 median
FM_MED = 2e-6
SEAM_FM = 2e-5       # chunked == one shot, wrapped angle

FS = 2400000
F_OFF = 25000.0
ROWS = 40
REST = 300
N_STREAM = ROWS * 1024 + REST
GUARD = 64
PATTERN = 0x7FC0DEAD                      # a quiet NaN with a payload: no output is ever this word


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


@pytest.fixture(scope="module")
def stream(hip):
    """one stream and its float64 reference, shared by every case and left unchanged"""
    raw = O.synth_iq_fm(N_STREAM, FS, 4100, f_carrier=F_OFF, f_mod=700.0, dev=4.0)
    x = O.grid_c64(raw)
    taps = np.ascontiguousarray(O.win_hamming(255))
    y = O.FilterState(taps).applyOn(O.nco(x, F_OFF, FS, 0))
    z = y[1:] * np.conj(y[:-1])
    s = dict(raw=raw, x=x, taps=taps, y=y, ang=np.angle(z), mag=np.abs(z), peak=float(np.max(np.abs(y))),
             d_c64=hip.DevArray.from_host(x), d_u8=hip.DevArray.from_host(np.ascontiguousarray(raw.reshape(-1))))
    for v in (raw, x, taps, y, s["ang"], s["mag"]):
        v.setflags(write=False)
    return s


@pytest.fixture
def shape(hip):
    """dd_debug_cos1k_shape for the rest of the test; the plan's own choice comes back afterwards"""
    def force(nwaves, run_rows):
        hip.check(hip.lib().dd_debug_cos1k_shape(nwaves, run_rows), "dd_debug_cos1k_shape")
    yield force
    force(0, 0)


class Chain:
    """a dd_chain handle: NCO + hamming(255), angles (fm) or the FIR output itself, complex64 or raw u8 input"""

    def __init__(self, hip, taps, fm, u8):
        self.hip, self.lib, self.fm, self.u8 = hip, hip.lib(), fm, u8
        self.h = C.c_void_p()
        flags = hip.DD_CHAIN_NCO | (hip.DD_CHAIN_FM if fm else 0) | (hip.DD_CHAIN_U8_INPUT if u8 else 0)
        hip.check(self.lib.dd_chain_create(C.byref(self.h), taps.ctypes.data_as(C.POINTER(C.c_double)), 255,
                                           hip.cycles_q64(F_OFF, FS), 1, flags))

    def process(self, src, pos, n, out, opos):
        """samples [pos, pos + n) of the device stream `src` -> out[opos ...]; returns the output count"""
        got = C.c_int64(-1)
        self.hip.check(self.lib.dd_chain_process(self.h, src.ptr + (2 if self.u8 else 8) * pos, out.ptr + (4 if self.fm else 8) * opos,
                                                 n, C.byref(got), None))
        assert self.lib.dd_chain_last_kernel(self.h) == self.hip.DD_KERNEL_COS_RS          # the running-sum kernel
        return got.value

    def close(self):
        self.lib.dd_chain_destroy(self.h)


def fm_errors(got, ref_angle):
    return np.abs(np.angle(np.exp(1j * (np.asarray(got, dtype=np.float64) - ref_angle))))


def fm_check(got, ref_angle, mag):
    assert np.shape(got) == ref_angle.shape, (np.shape(got), ref_angle.shape)
    d = fm_errors(got, ref_angle)
    print("FM: max %.3g (|z| >= 1e-3 median), max %.3g (well-conditioned), median %.3g" %
          (np.max(d[mag >= 1e-3 * np.median(mag)]), np.max(d[mag >= 0.1 * np.median(mag)]), np.median(d)))
    assert np.max(d[mag >= 1e-3 * np.median(mag)]) <= FM_MAX
    assert np.max(d[mag >= 0.1 * np.median(mag)]) <= FM_WELL
    assert np.median(d) <= FM_MED


def fir_check(got, ref, peak):
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    e = float(np.max(np.abs(got - ref)) / peak)
    print("FIR: max error %.3g of the peak" % e)
    assert e < FIR_TOL


def check_against_oracle(stream, fm, first_sample, got):
    """`got`: the outputs of the samples from `first_sample` on (angles: index k pairs samples k + 1 and k; a stream start has none for
    sample 0, so its first angle is index 0 too)"""
    n = len(got)
    if fm:
        k0 = max(first_sample - 1, 0)
        fm_check(got, stream["ang"][k0:k0 + n], stream["mag"][k0:k0 + n])
    else:
        fir_check(got, stream["y"][first_sample:first_sample + n], stream["peak"])


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("forced", [(0, 0), (8, 2)], ids=["plan", "8waves_runs_of_2"])
@pytest.mark.parametrize("off", [0, 1, 7, 15])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fm", [True, False])
def test_every_output_is_stored_and_nothing_beside_them(hip, stream, select_kernel, shape, fm, u8, off, forced):
    """Chunks of 5, 9 and 33 rows at the stream's start and behind 300 samples, `out` 0, 1, 7 and 15 elements behind a line in a
    buffer filled with a NaN pattern, 64 guard elements on each side: every output within tolerance of the oracle (so it was
    written: the pattern is a NaN), every guard element untouched.  A row base or lane offset of the store form that is off by a
    row or a line shows as a pattern among the outputs or a value among the guards.  Run once in the plan's own shape (one run per
    wave) and once in runs of 2 rows on 8 waves (c1_prime_light, the angles of a run's last row flushed behind it)."""
    select_kernel(None)
    shape(*forced)
    src = stream["d_u8"] if u8 else stream["d_c64"]
    dt = np.float32 if fm else np.complex64
    plan = (C.c_int * 4)()
    for rows in (5, 9, 33):
        L = rows * 1024 - 16
        for lead in (0, REST):
            hip.check(hip.lib().dd_debug_cos1k_plan(L, 1 if fm and not lead else 0, off, 256, plan), "dd_debug_cos1k_plan")
            assert plan[1] == rows
            fill = np.full((L + 2 * GUARD + 16) * (1 if fm else 2), PATTERN, dtype=np.uint32).view(dt)
            out = hip.DevArray.from_host(fill)
            assert out.ptr % 128 == 0
            ch = Chain(hip, stream["taps"], fm, u8)
            if lead:
                scratch = hip.DevArray(lead, dt)
                assert ch.process(src, 0, lead, scratch, 0) == (lead - 1 if fm else lead)
            n = ch.process(src, lead, L, out, GUARD + off)
            ch.close()
            assert n == (L - 1 if fm and not lead else L)
            res = out.to_host()
            check_against_oracle(stream, fm, lead, res[GUARD + off:GUARD + off + n])
            assert np.all(words(res[:GUARD + off]) == PATTERN), "a store in front of the outputs"
            assert np.all(words(res[GUARD + off + n:]) == PATTERN), "a store behind the outputs"


@pytest.mark.parametrize("run_rows", [2, 3, 8])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fm", [True, False])
def test_runs_are_dealt_one_to_one_whatever_the_wave_count(hip, stream, select_kernel, shape, fm, u8, run_rows):
    """The 40-row chunk in runs of 2, 3 and 8 rows on 4, 8, 12, 20 and 36 waves (1, 2, 3, 5 and 9 workgroups; 40 rows in runs of 3 or
    8 end in a ragged run; 36 waves leave waves without a run for R = 3 and 8), then the stream's remaining samples as a second chunk:
    the state it starts from (tail_out, lasty_out) was written by the wave that owns the first chunk's last run.  Equal R: the same
    bytes for every wave count, both chunks; and both within tolerance of the oracle."""
    select_kernel(None)
    src = stream["d_u8"] if u8 else stream["d_c64"]
    dt = np.float32 if fm else np.complex64
    L1 = ROWS * 1024 - 16
    plan = (C.c_int * 4)()
    hip.check(hip.lib().dd_debug_cos1k_plan(L1, 1 if fm else 0, 0, 256, plan), "dd_debug_cos1k_plan")
    assert plan[1] == ROWS
    first = None
    for nwaves in (4, 8, 12, 20, 36):
        shape(nwaves, run_rows)
        out = hip.DevArray.from_host(np.full((N_STREAM + 16) * (1 if fm else 2), PATTERN, dtype=np.uint32).view(dt))
        ch = Chain(hip, stream["taps"], fm, u8)
        n1 = ch.process(src, 0, L1, out, 0)
        n2 = ch.process(src, L1, N_STREAM - L1, out, n1)
        ch.close()
        assert n1 == (L1 - 1 if fm else L1) and n1 + n2 == (N_STREAM - 1 if fm else N_STREAM)
        res = out.to_host()[:n1 + n2]
        if first is None:
            first = res
            check_against_oracle(stream, fm, 0, res)
        else:
            assert np.array_equal(words(res), words(first)), "nwaves = %d differs from nwaves = 4 at run_rows = %d" % (nwaves, run_rows)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fm", [True, False])
def test_runs_of_8_rows_against_one_run_per_wave(hip, stream, select_kernel, shape, fm, u8):
    """the same 40-row chunk with run_rows = 8 (five runs, each started by c1_prime_light) and in the plan's own shape (run_rows = 0:
    every wave one row, started the same way): a run's first rows differ in their last bits only -- the suite's chunked == one-shot
    bound for angles, 2e-6 of the peak for the FIR output"""
    select_kernel(None)
    src = stream["d_u8"] if u8 else stream["d_c64"]
    dt = np.float32 if fm else np.complex64
    L = ROWS * 1024 - 16
    res = []
    for forced in ((0, 8), (0, 0)):
        shape(*forced)
        out = hip.DevArray(L + 16, dt)
        ch = Chain(hip, stream["taps"], fm, u8)
        n = ch.process(src, 0, L, out, 0)
        ch.close()
        res.append(out.to_host()[:n])
    if fm:
        d = fm_errors(res[0], res[1].astype(np.float64))
        print("run_rows 8 against 0: max wrapped difference %.3g rad" % np.max(d))
        assert np.max(d) < SEAM_FM
    else:
        e = float(np.max(np.abs(res[0] - res[1])) / stream["peak"])
        print("run_rows 8 against 0: max difference %.3g of the peak" % e)
        assert e < FIR_TOL
    check_against_oracle(stream, fm, 0, res[0])
