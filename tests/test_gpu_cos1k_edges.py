"""
k_chain_cos1k's edge rows and state hand-out (dd_cosfir.hip: c1_edge_samples), shape by shape.

An edge row is a row of 1024 samples that holds samples before the first output, the carried state (254 samples of history after
the NCO, the last FIR output) or the chunk's end; it loads every position's sample, history entry and phasor-table entry on clamped
indices in one batch and selects by position afterwards, and the wave that owns the chunk's last run writes the next chunk's
history before its runs.  The cases below put every boundary of those selections -- n < 0, n + 254 >= 0, n < L -- at every kind of
place in a row: chunk lengths around 1, 16, 255 and 1024, `out` 0, 1, 7 and 15 elements behind a 64-byte line (which moves the row
grid: DDCos1kArgs::base), stream start (no angle for sample 0, no carried state) and mid-stream chunks (history and last output
carried), complex64 and raw u8 input, angles and complex64 output, NCO on.

Reference: the float64 oracle (oracle/dd_oracle.py), computed once per module over one 8192-sample stream; a FIR is causal, so a
chunk's outputs are a slice of the stream's.  Tolerances: those of tests/test_gpu_parity.py for this kernel (FIR 2e-6 of the peak;
FM 2e-5 rad on well-conditioned outputs, 1e-4 where the product is not vanishing, median 2e-6), copied, not loosened.
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
SEAM_FM = 2e-5       # chunked == one shot, wrapped angle (test_capi_chain_handle_and_prime)

FS = 2400000
F_OFF = 25000.0
N_STREAM = 8192
LENGTHS = [1, 2, 15, 16, 17, 254, 255, 256, 1023, 1024, 1025, 2051]
OFFSETS = [0, 1, 7, 15]
LEAD = 300           # mid-stream cases: samples processed before the chunk under test (more than the 254 of history)


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
    s = dict(raw=raw, x=x, taps=taps, y=y, ang=np.angle(z), mag=np.abs(z),
             d_c64=hip.DevArray.from_host(x), d_u8=hip.DevArray.from_host(np.ascontiguousarray(raw.reshape(-1))))
    for v in (raw, x, taps, y, s["ang"], s["mag"]):
        v.setflags(write=False)
    return s


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


def fm_check(got, ref_angle, mag):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref_angle.shape, (got.shape, ref_angle.shape)
    d = np.abs(np.angle(np.exp(1j * (got - ref_angle))))
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


def _run_lengths(hip, stream, fm, u8, off, lead):
    """every length of LENGTHS as a chunk of its own whose `out` sits `off` elements behind a 64-byte (angles) / 128-byte (complex64)
    line, at the stream's start (lead = 0) or behind `lead` samples processed first; results and references of all lengths joined"""
    src = stream["d_u8"] if u8 else stream["d_c64"]
    out = hip.DevArray(4096, np.float32 if fm else np.complex64)
    scratch = hip.DevArray(4096, np.float32 if fm else np.complex64)
    assert out.ptr % 128 == 0
    gots, refs, mags = [], [], []
    for L in LENGTHS:
        ch = Chain(hip, stream["taps"], fm, u8)
        first = 0
        if lead:
            first = ch.process(src, 0, lead, scratch, 0)
            assert first == (lead - 1 if fm else lead)
        n = ch.process(src, lead, L, out, off)
        ch.close()
        res = out.to_host()[off:off + n]
        if fm:
            assert n == (L if lead else L - 1)
            k0 = lead - 1 if lead else 0
            refs.append(stream["ang"][k0:k0 + n])
            mags.append(stream["mag"][k0:k0 + n])
        else:
            assert n == L
            refs.append(stream["y"][lead:lead + L])
        gots.append(res)
    got, ref = np.concatenate(gots), np.concatenate(refs)
    if fm:
        fm_check(got, ref, np.concatenate(mags))
    else:
        fir_check(got, ref, np.max(np.abs(stream["y"])))


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fm", [True, False])
def test_stream_start_chunks_of_every_edge_length(hip, stream, select_kernel, fm, u8, off):
    """s = 1 (FM): row -1 holds the zero history and sample 0, which has no angle; L = 1 gives no angle at all, L <= 16 ends inside the
    first lane, 254 / 255 / 256 straddle the history's length, 1023 / 1024 / 1025 the row's, 2051 has one interior row between two
    edge rows when `out` is aligned (row 0 is an edge row: it holds sample 0) -- every chunk ends in an edge row that hands out the
    next history and the last FIR output"""
    select_kernel(None)
    _run_lengths(hip, stream, fm, u8, off, 0)


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fm", [True, False])
def test_mid_stream_chunks_of_every_edge_length(hip, stream, select_kernel, fm, u8, off):
    """s = 0: the chunk's first rows read the carried history (n < 0) and, for angles, the carried FIR output (n = -1); for L < 254 the
    new history is part old history, part new samples"""
    select_kernel(None)
    _run_lengths(hip, stream, fm, u8, off, LEAD)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fm", [True, False])
def test_cut_stream_equals_one_chunk(hip, stream, select_kernel, fm, u8):
    """6000 samples cut as [1, 253, 1024, 777, 2048, rest], outputs back to back (so `out` sits at a different place of its line for
    every chunk), against the same samples as ONE chunk: the state handed from chunk to chunk -- written BEFORE the owning wave's
    rows -- is what the one-chunk run has in its own rows.  Angles: 2e-5 rad wrapped (the suite's chunked == one-shot bound);
    complex64: 2e-6 of the peak (both runs are within that of the float64 filter; the stricter bound is used)."""
    select_kernel(None)
    N = 6000
    cuts = [1, 253, 1024, 777, 2048]
    cuts.append(N - sum(cuts))
    src = stream["d_u8"] if u8 else stream["d_c64"]
    dt = np.float32 if fm else np.complex64
    one, cut = hip.DevArray(N + 16, dt), hip.DevArray(N + 16, dt)
    ch = Chain(hip, stream["taps"], fm, u8)
    n_one = ch.process(src, 0, N, one, 0)
    ch.close()
    ch = Chain(hip, stream["taps"], fm, u8)
    pos = opos = 0
    for n in cuts:
        opos += ch.process(src, pos, n, cut, opos)
        pos += n
    ch.close()
    assert n_one == opos == (N - 1 if fm else N)
    a, b = one.to_host()[:opos], cut.to_host()[:opos]
    if fm:
        d = np.abs(np.angle(np.exp(1j * (a.astype(np.float64) - b.astype(np.float64)))))
        print("cut stream against one chunk: max wrapped difference %.3g rad" % np.max(d))
        assert np.max(d) < SEAM_FM
        fm_check(b, stream["ang"][:opos], stream["mag"][:opos])
    else:
        e = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
        print("cut stream against one chunk: max difference %.3g of the peak" % e)
        assert e < FIR_TOL
        fir_check(b, stream["y"][:N], np.max(np.abs(stream["y"][:N])))


@pytest.mark.parametrize("fm", [True, False])
def test_last_wave_walks_interior_rows_then_the_edge_row(hip, stream, select_kernel, fm):
    """The smallest chunk in which the LAST wave's range holds interior rows and the chunk's final edge row: nrows >= 2 nwaves, which
    with every wave of the device in use (nwaves = 8 per CU) is a little over 16 rows per CU.  Path reached: run_rows = 0 (one
    run per wave, rows [nrows w / nwaves, nrows (w + 1) / nwaves) -- run_rows = 8 needs nrows >= 16 nwaves, a 2^25-sample chunk on
    256 CUs), the last wave: history hand-out first, then c1_prime_light, interior rows, the edge row with the chunk's end.
    The stream is the module's 8192 samples repeated; the float64 reference is taken over windows (the FIR forgets after 254
    samples): the chunk's start, a wave boundary in the middle, and its end."""
    import torch
    select_kernel(None)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    L = 2 * 8 * ncu * 1024 + 1500
    plan = (C.c_int * 4)()
    hip.check(hip.lib().dd_debug_cos1k_plan(L, 1 if fm else 0, 0, ncu, plan), "dd_debug_cos1k_plan")
    base, nrows, grid, nwaves = list(plan)
    assert nwaves == 8 * ncu and 2 * nwaves <= nrows < 16 * nwaves                  # run_rows = 0, at least two rows for every wave
    reps = -(-L // N_STREAM)
    x = np.tile(stream["x"], reps)[:L]
    src = hip.DevArray.from_host(x)
    out = hip.DevArray(L, np.float32 if fm else np.complex64)
    ch = Chain(hip, stream["taps"], fm, False)
    n = ch.process(src, 0, L, out, 0)
    ch.close()
    assert n == (L - 1 if fm else L)
    res = out.to_host()
    W = 4096
    mid = base + 1024 * ((nrows * (nwaves // 2)) // nwaves) - W // 2                # around the first row of wave nwaves / 2
    peak = np.max(np.abs(stream["y"]))
    for w0 in (0, mid, L - W):
        lo = max(w0 - 254, 0)
        y = O.FilterState(stream["taps"]).applyOn(O.nco(x[lo:w0 + W], F_OFF, FS, lo))[w0 - lo:]        # y[w0 .. w0 + W)
        if fm:
            z = y[1:] * np.conj(y[:-1])                                             # angle index k: samples k + 1 and k
            fm_check(res[w0:w0 + W - 1], np.angle(z), np.abs(z))
        else:
            fir_check(res[w0:w0 + W], y, peak)
