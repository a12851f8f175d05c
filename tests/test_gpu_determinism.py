"""
Launch-to-launch determinism of the hot-path kernels (run with -m gpu on an MI355X).

None of the kernels uses an atomic on the data path, so the same call over the same device-resident input must give the
same BITS every time -- whatever ran on the GPU in between.  The hardware does not clear LDS between workgroups: a
kernel that reads an LDS word it never wrote is still "correct within tolerance" when the stale word only steers a
wave-uniform choice between two valid code paths (that was the case for k_chain_mfma_ab's small-angle test in round 2:
outputs one ulp apart from launch to launch), and wrong when it is data.  Both show up here: every configuration runs
after dd_debug_fill_lds() has left NaN bit patterns, zeros and huge finite values in every CU's LDS, and the outputs are
compared as integers.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import dd_oracle as O

pytestmark = pytest.mark.gpu

FS = 2400000
PATTERNS = (0xFFFFFFFF, 0x00000000, 0x7F7F7F7F, 0xFFFFFFFF)     # NaN (f32 and f16), zeros, 3.4e38 / f16 NaN, NaN again


@pytest.fixture(scope="module")
def g():
    torch = pytest.importorskip("torch")
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from directdemod_amd import _hip
    _hip.require_gpu()
    import bench

    class G:
        pass
    r = G()
    r.torch, r.hip, r.lib, r.bench = torch, _hip, _hip.lib(), bench
    r.dev = torch.device("cuda", 0)
    r.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return r


def _chain_runs(g, taps, M, flags, x, n, out_floats, f_off=25000.0):
    """One dd_chain handle, reset and re-run over the same input after each LDS fill; returns the outputs."""
    t, lib, hip = g.torch, g.lib, g.hip
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    h = C.c_void_p()
    hip.check(lib.dd_chain_create(C.byref(h), taps.ctypes.data_as(C.POINTER(C.c_double)), len(taps),
                                  hip.cycles_q64(f_off, FS), M, flags), "dd_chain_create")
    outs, kernels = [], []
    try:
        for pat in PATTERNS:
            hip.check(lib.dd_debug_fill_lds(pat, g.stream), "dd_debug_fill_lds")
            lib.dd_chain_reset(h, g.stream)
            out = t.full((out_floats,), float("nan"), dtype=t.float32, device=g.dev)
            got = C.c_int64(0)
            hip.check(lib.dd_chain_process(h, x.data_ptr(), out.data_ptr(), n, C.byref(got), g.stream), "dd_chain_process")
            t.cuda.synchronize()
            kernels.append(lib.dd_chain_last_kernel(h))
            outs.append((out, got.value))
    finally:
        lib.dd_chain_destroy(h)
    return outs, kernels


def _assert_identical(g, outs, per_out):
    t = g.torch
    ref, got0 = outs[0]
    assert got0 > 0
    valid = ref[:got0 * per_out]
    assert bool(t.isfinite(valid).all())
    for out, got in outs[1:]:
        assert got == got0
        diff = int((out[:got * per_out].view(t.int32) != valid.view(t.int32)).sum())
        assert diff == 0, "%d of %d output words differ between two launches over the same input" % (diff, got * per_out)


def _hamming(K):
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(K) / (K - 1))


@pytest.mark.parametrize("ntaps", [255, 151, 127, 63])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("kernel", ["auto", "ab", "fft1k", "cos1k"])
def test_fm_chain_undecimated_is_bit_reproducible(g, ntaps, u8, kernel, select_kernel):
    """NCO + FIR + FM at M = 1: k_chain_fft1k (the 162..256-tap class by default, every class when forced: no atomics, one
    wave per block, LDS image rewritten completely before it is read) and k_chain_mfma_ab (every tap class) with the edge
    tiles riding along."""
    select_kernel(None if kernel == "auto" else kernel)
    if ntaps == 255 and kernel in ("auto", "cos1k"):
        want = g.hip.DD_KERNEL_COS_RS                            # Hamming 255: the running-sum kernel (round 5)
    elif kernel == "fft1k" or (kernel in ("auto", "cos1k") and ntaps > 161):
        want = g.hip.DD_KERNEL_FFT_OS
    else:
        want = g.hip.DD_KERNEL_MFMA_AB
    t = g.torch
    n = (1 << 23) + 12345
    x = g.bench.make_input(t, n, 0, g.dev, 5 + ntaps)
    flags = g.hip.DD_CHAIN_NCO | g.hip.DD_CHAIN_FM
    if u8:
        x = (x + 127.5).round().clamp(0, 255).to(t.uint8).contiguous()
        flags |= g.hip.DD_CHAIN_U8_INPUT
    outs, kernels = _chain_runs(g, _hamming(ntaps), 1, flags, x, n, n)
    assert set(kernels) == {want}
    _assert_identical(g, outs, 1)


@pytest.mark.parametrize("kernel", ["auto", "fft1k", "ab"])
def test_complex_output_chain_is_bit_reproducible(g, kernel, select_kernel):
    """NCO + FIR, complex64 out: k_chain_cos1k's complex-output flavour (the default for Hamming 255 since round 5), k_chain_fft1k's
    and k_chain_mfma_ab's (forced)."""
    select_kernel(None if kernel == "auto" else kernel)
    t = g.torch
    n = (1 << 23) + 777
    x = g.bench.make_input(t, n, 0, g.dev, 99)
    outs, kernels = _chain_runs(g, _hamming(255), 1, g.hip.DD_CHAIN_NCO, x, n, 2 * n)
    assert set(kernels) == {{"auto": g.hip.DD_KERNEL_COS_RS, "fft1k": g.hip.DD_KERNEL_FFT_OS, "ab": g.hip.DD_KERNEL_MFMA_AB}[kernel]}
    _assert_identical(g, outs, 2)


@pytest.mark.parametrize("M,ntaps,fm", [(34, 151, True), (50, 127, False), (8, 255, True), (2, 63, False)])
@pytest.mark.parametrize("u8", [False, True])
def test_decimating_chain_is_bit_reproducible(g, M, ntaps, fm, u8):
    """k_chain_decim_p (persistent, edge tiles in the same launch), complex64 and FM outputs."""
    t = g.torch
    n = (1 << 23) + 4321
    x = g.bench.make_input(t, n, 0, g.dev, 1000 + M)
    flags = g.hip.DD_CHAIN_NCO | (g.hip.DD_CHAIN_FM if fm else 0)
    if u8:
        x = (x + 127.5).round().clamp(0, 255).to(t.uint8).contiguous()
        flags |= g.hip.DD_CHAIN_U8_INPUT
    per = 1 if fm else 2
    outs, kernels = _chain_runs(g, _hamming(ntaps), M, flags, x, n, per * (n // M + 2))
    assert len(set(kernels)) == 1 and kernels[0] != g.hip.DD_KERNEL_NONE
    _assert_identical(g, outs, per)


@pytest.mark.parametrize("shape", ["C3", "C4", "ragged", "tiny_chunks"])
@pytest.mark.parametrize("fm", [True, False])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("kernel", ["auto", "decimp"])
def test_chunk_list_in_one_launch_equals_the_chunk_loop_bit_for_bit(g, shape, fm, u8, kernel, select_kernel):
    """dd_chain_process_chunks: every chunk of a decimating chunk loop in ONE launch.  k_chain_decim_w (even M in 8..64, round 5) lays
    its rows on the absolute decimation grid and rotates every sample by a pure function of its absolute index: the list is one long
    chunk, no hand-over inside the launch.  k_chain_decim_multi (other M; every M when "decimp" is selected): the carried state crosses
    the chunk seams through device memory inside the launch.  Outputs, per-chunk counts and the state left behind (checked by one more
    chunk afterwards) must equal those of the dd_chain_process loop as integers; also after LDS fills, and with the seam flags' buffer
    reused from call to call."""
    select_kernel(None if kernel == "auto" else kernel)
    t, lib, hip = g.torch, g.lib, g.hip
    if shape == "C3":
        M, taps, n, cuts = 50, _hamming(127), 1 << 23, [i << 21 for i in range(5)]
    elif shape == "C4":
        M, taps, n, cuts = 34, _hamming(151), (1 << 23) + 999, [0, 3000000, 6000000, (1 << 23) + 999]
    elif shape == "ragged":
        M, taps, n, cuts = 8, _hamming(255), (1 << 22) + 77, [0, 1000001, 1000001 + 70003, 3000000, (1 << 22) + 77]
    else:
        M, taps, n, cuts = 5, _hamming(63), 200000, list(range(0, 200001, 20000))      # chunks without an interior run
    tail = 50000                                                                      # one more chunk through the plain entry afterwards
    x = g.bench.make_input(t, n + tail, 0, g.dev, 4242 + M)
    flags = hip.DD_CHAIN_NCO | (hip.DD_CHAIN_FM if fm else 0)
    isz = 8
    if u8:
        x = (x + 127.5).round().clamp(0, 255).to(t.uint8).contiguous()
        flags |= hip.DD_CHAIN_U8_INPUT
        isz = 2
    per = 1 if fm else 2
    taps = np.ascontiguousarray(taps, dtype=np.float64)

    def make():
        h = C.c_void_p()
        hip.check(lib.dd_chain_create(C.byref(h), taps.ctypes.data_as(C.POINTER(C.c_double)), len(taps), hip.cycles_q64(25000.0, FS), M, flags), "create")
        return h
    nfl = per * ((n + tail) // M + 8)
    # the loop
    h = make()
    ref = t.full((nfl,), float("nan"), dtype=t.float32, device=g.dev)
    counts, pos = [], 0
    got = C.c_int64(0)
    for a, b in zip(cuts[:-1] + [n], cuts[1:] + [n + tail]):
        hip.check(lib.dd_chain_process(h, x.data_ptr() + isz * a, ref.data_ptr() + 4 * per * pos, b - a, C.byref(got), g.stream), "process")
        counts.append(got.value)
        pos += got.value
    assert lib.dd_chain_last_kernel(h) != hip.DD_KERNEL_NONE
    lib.dd_chain_destroy(h)
    t.cuda.synchronize()
    # one launch (twice on the same handle after a reset, once after an LDS fill)
    h = make()
    bounds = (C.c_int64 * len(cuts))(*cuts)
    nout = (C.c_int64 * (len(cuts) - 1))()
    for rep, pat in enumerate((None, 0xFFFFFFFF, 0x00000000)):
        if pat is not None:
            hip.check(lib.dd_debug_fill_lds(pat, g.stream), "fill")
        lib.dd_chain_reset(h, g.stream)
        out = t.full((nfl,), float("nan"), dtype=t.float32, device=g.dev)
        hip.check(lib.dd_chain_process_chunks(h, x.data_ptr(), out.data_ptr(), bounds, len(cuts) - 1, nout, g.stream), "chunks")
        assert lib.dd_chain_last_kernel(h) == (hip.decim_wave_kernel(len(taps), M) if kernel == "auto" and shape != "tiny_chunks" else hip.DD_KERNEL_DECIM_MULTI)
        assert list(nout) == counts[:-1]
        p2 = sum(nout)
        hip.check(lib.dd_chain_process(h, x.data_ptr() + isz * n, out.data_ptr() + 4 * per * p2, tail, C.byref(got), g.stream), "process")
        assert got.value == counts[-1]
        t.cuda.synchronize()
        tot = per * (p2 + got.value)
        assert bool(t.isfinite(ref[:tot]).all())
        diff = int((out[:tot].view(t.int32) != ref[:tot].view(t.int32)).sum())
        assert diff == 0, "%d of %d output words differ from the chunk loop (rep %d)" % (diff, tot, rep)
    lib.dd_chain_destroy(h)


def test_withheld_hand_over_is_reported_not_silently_wrong(g, select_kernel):
    """k_chain_decim_multi (the chunk-list kernel for the decimations k_chain_decim_w does not take; selected here with "decimp"):
    dd_chain_process_chunks hands the carried FIR / FM state from chunk to chunk INSIDE one launch (agent-scope flags).  A
    consumer whose flag never arrives gives up after a bounded spin and reads whatever the state buffers hold; that used to end
    with DD_OK and wrong samples.  dd_debug_seam withholds one chunk's flag (and shortens the spin bound): the call itself still
    returns (the kernel completes), the error surfaces as DD_ERR_TIMEOUT at dd_stream_sync -- or at the next chunk-list call on
    the filter, whichever comes first -- and a run without the fault afterwards is bit-identical to the chunk loop again."""
    select_kernel("decimp")
    t, lib, hip = g.torch, g.lib, g.hip
    M, taps, n = 34, np.ascontiguousarray(_hamming(151), dtype=np.float64), 1 << 22
    cuts = [0, 1000000, 2000001, 3000000, n]
    x = g.bench.make_input(t, n, 0, g.dev, 99)
    h = C.c_void_p()
    hip.check(lib.dd_chain_create(C.byref(h), taps.ctypes.data_as(C.POINTER(C.c_double)), len(taps), hip.cycles_q64(30000.0, FS), M,
                                  hip.DD_CHAIN_NCO | hip.DD_CHAIN_FM), "create")
    bounds = (C.c_int64 * len(cuts))(*cuts)
    nout = (C.c_int64 * (len(cuts) - 1))()
    nfl = n // M + 8

    def one_launch():
        lib.dd_chain_reset(h, g.stream)
        out = t.full((nfl,), float("nan"), dtype=t.float32, device=g.dev)
        rc = lib.dd_chain_process_chunks(h, x.data_ptr(), out.data_ptr(), bounds, len(cuts) - 1, nout, g.stream)
        return rc, out
    rc, good = one_launch()
    assert rc == 0 and lib.dd_chain_last_kernel(h) == hip.DD_KERNEL_DECIM_MULTI
    assert lib.dd_stream_sync(g.stream) == 0
    # fault 1: reported by dd_stream_sync
    hip.check(lib.dd_debug_seam(1, 12), "dd_debug_seam")              # chunk 1's flag withheld, waits bounded by 2^12 polls
    rc, bad = one_launch()
    assert rc == 0                                                   # (the launch is asynchronous: nothing is known yet)
    rc = lib.dd_stream_sync(g.stream)
    assert rc == hip.DD_ERR_TIMEOUT, rc
    assert b"hand-over" in lib.dd_last_error()
    assert lib.dd_stream_sync(g.stream) == 0                         # reported once
    # fault 2: reported by the next chunk-list call through the same filter (once the faulty launch has finished)
    hip.check(lib.dd_debug_seam(2, 12), "dd_debug_seam")
    rc, bad = one_launch()
    assert rc == 0
    t.cuda.synchronize()                                             # (torch's own sync: the library has not looked yet)
    rc, _ = one_launch()
    assert rc == hip.DD_ERR_TIMEOUT, rc
    with pytest.raises(hip.HipError):
        hip.check(rc, "dd_chain_process_chunks")
    #  the report zeroes the error word -- a further chunk-list call WITHOUT a reset must still refuse to go on from the state
    # the faulty launch committed
    out2 = t.full((nfl,), float("nan"), dtype=t.float32, device=g.dev)
    assert lib.dd_chain_process_chunks(h, x.data_ptr(), out2.data_ptr(), bounds, len(cuts) - 1, nout, g.stream) == hip.DD_ERR_TIMEOUT
    assert b"reset" in lib.dd_last_error()
    # and without the fault everything is as before
    hip.check(lib.dd_debug_seam(-1, 0), "dd_debug_seam")
    rc, again = one_launch()
    assert rc == 0 and lib.dd_stream_sync(g.stream) == 0
    tot = sum(nout)
    assert int((again[:tot].view(t.int32) != good[:tot].view(t.int32)).sum()) == 0
    lib.dd_chain_destroy(h)


@pytest.mark.parametrize("n", [300, 5000, 70000])
def test_short_chunks_are_bit_reproducible(g, n):
    """chunks too short for the persistent kernels (dense / tiled kernels only)."""
    t = g.torch
    x = g.bench.make_input(t, n, 0, g.dev, n)
    for M in (1, 5):
        outs, _ = _chain_runs(g, _hamming(255), M, g.hip.DD_CHAIN_NCO | g.hip.DD_CHAIN_FM, x, n, n)
        _assert_identical(g, outs, 1)


def test_class_level_filters_are_bit_reproducible(g):
    """the stand-alone stages behind the drop-in classes: FIR (float64 taps), IIR block scan, polyphase resampler."""
    t, hip = g.torch, g.hip
    import directdemod_amd.comm as comm
    import directdemod_amd.filters as filters
    import directdemod_amd.resample as resample
    L = 1 << 20
    x = O.grid_c64(O.synth_iq_fm(L, FS, 31, f_carrier=25e3))
    a = np.abs(x).astype(np.float32)

    def once():
        sig = comm.commSignal(FS, x).offsetFreq(25000.0).filter(filters.blackmanHarris(151)).signal
        env = comm.commSignal(FS, a).filter(filters.butter(FS, 4160.0)).signal
        iq = comm.commSignal(FS, x).filter(filters.butter(FS, 40000.0)).signal        # complex IIR: the wave-wide block scan
        aud = comm.commSignal(FS, a).resamplePoly(resample.polyResampler(FS, 20800)).signal
        return [np.asarray(v).copy() for v in (sig, env, iq, aud)]
    runs = []
    for pat in PATTERNS[:3]:
        hip.check(g.lib.dd_debug_fill_lds(pat, g.stream), "dd_debug_fill_lds")
        t.cuda.synchronize()
        runs.append(once())
    for r in runs[1:]:
        for got, ref in zip(r, runs[0]):
            assert got.dtype == ref.dtype and got.shape == ref.shape
            assert np.array_equal(got.view(np.uint8), ref.view(np.uint8))


def test_audio_side_stages_are_bit_reproducible(g):
    """config 4 end to end (crude + accurate sync: fused front end, Hilbert envelope, zero-phase filters, normalised
    correlation, peak pick, the batched sync windows), the FFT resampler, filtfilt and the AFSK correlators."""
    t, hip = g.torch, g.hip
    import directdemod_amd.comm as comm
    import directdemod_amd.demod_am as demod_am
    import directdemod_amd.noaa_sync as noaa
    import directdemod_amd.source as source
    import directdemod_amd._ops as ops
    from directdemod_amd import afsk
    raw = O.synth_apt_iq(3.0, 2048000, seed=4)
    rng = np.random.default_rng(12)
    real = rng.standard_normal(50001)
    cplx = (rng.standard_normal(4000) + 1j * rng.standard_normal(4000)).astype(np.complex128)
    aud = rng.standard_normal(30000) * 0.3 + np.sin(2 * np.pi * 1700 * np.arange(30000) / 22050)

    def once():
        ns = noaa.noaa_sync(source.IQarray(raw, 2048000), 30000.0)
        sa, sb = ns.getCrudeSync()
        (ia, pa, ta), (ib, pb, tb) = ns.getAccurateSync()
        outs = [np.asarray(v, dtype=np.float64) for v in (sa, sb, ia, pa, ta, ib, pb, tb)]
        outs.append(np.asarray(demod_am.demod_am().demod_blocks(real, 3000)))
        outs.append(np.asarray(comm.commSignal(60235, real).bwLim(40960, True).signal))
        outs.append(ops.filtfilt(O.win_blackmanharris(151), hip.DevArray.from_host(cplx)).to_host())
        bf = afsk.binary_filter(aud, 22050)
        outs.append(np.asarray(bf))
        outs.append(np.asarray(afsk.bit_edges(bf, 18)))
        return outs
    runs = []
    for pat in PATTERNS[:3]:
        hip.check(g.lib.dd_debug_fill_lds(pat, g.stream), "dd_debug_fill_lds")
        t.cuda.synchronize()
        runs.append(once())
    for r in runs[1:]:
        for k, (got, ref) in enumerate(zip(r, runs[0])):
            assert got.dtype == ref.dtype and got.shape == ref.shape, k
            assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), "stage output %d differs between runs" % k


# k_chain_decim_b through the padded LDS image (M = 0 mod 4), at stream phases where a row's last block reads past the row's last staged
# sample (phi = (first kept absolute index) mod M; dd_debug_decimb_lds_check, tests/test_decimb_layout.py) and at phi = 0
PADDED_B = [(32, 151, (26, 30)), (40, 151, (2, 38)), (16, 33, (10, 14)), (64, 255, (58, 62)), (12, 65, (1, 11)), (20, 100, (3, 18)), (8, 33, (2, 6))]
PADDED_PATTERNS = PATTERNS + (0x7F800000,)                      # + Inf (0 x Inf = NaN as well)
START = 7 * 2048 + 333                                          # absolute index of the chunk's first sample: rows do not start with the chunk


def _fused_handles(g, taps, fm):
    lib, hip = g.lib, g.hip
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    fir = C.c_void_p()
    hip.check(lib.dd_fir_create(C.byref(fir), taps.ctypes.data_as(C.POINTER(C.c_double)), len(taps)), "dd_fir_create")
    hip.check(lib.dd_fir_reset(fir, hip.DD_HIST_ZEROS, None, g.stream), "dd_fir_reset")
    fmh = None
    if fm:
        fmh = C.c_void_p()
        hip.check(lib.dd_fm_create(C.byref(fmh)), "dd_fm_create")
    return fir, fmh


def _fused_once(g, taps, M, fm, x, isz, n, start, off, flags, fill=None):
    """one dd_fused_process call (NCO on, stream at absolute sample `start`, first kept sample at chunk index `off`) on fresh state"""
    t, lib, hip = g.torch, g.lib, g.hip
    fir, fmh = _fused_handles(g, taps, fm)
    try:
        if fill is not None:
            hip.check(lib.dd_debug_fill_lds(fill, g.stream), "dd_debug_fill_lds")
        per = 1 if fm else 2
        out = t.full((per * (n // M + 2),), float("nan"), dtype=t.float32, device=g.dev)
        got = C.c_int64(0)
        hip.check(lib.dd_fused_process(fir, fmh, x.data_ptr(), out.data_ptr(), n, 1, hip.cycles_q64(25000.0, FS), start, M, off, flags, 1,
                                       C.byref(got), g.stream), "dd_fused_process")
        t.cuda.synchronize()
        return out, got.value, lib.dd_fir_last_kernel(fir)
    finally:
        lib.dd_fir_destroy(fir)
        if fmh is not None:
            lib.dd_fm_destroy(fmh)


@pytest.mark.parametrize("fm,u8", [(True, False), (False, False), (True, True), (False, True)])
@pytest.mark.parametrize("M,ntaps,phis", PADDED_B)
def test_padded_block_sums_are_bit_reproducible_after_lds_fills(g, M, ntaps, phis, fm, u8):
    """k_chain_decim_b's padded image: a row's last block reads up to seven samples past its kept sample (under zero taps, on the matrix pipe,
    where 0 x NaN is NaN); past the row's last staged sample those are cells the row clears.  Six rows per call (runs of two rows and the
    row before each), NaN / zero / huge / Inf LDS fills: every output finite and the same bits after every fill."""
    t, hip = g.torch, g.hip
    n = 6 * 2048 + 1111
    x = g.bench.make_input(t, n, START, g.dev, 77 + M)
    flags, isz = 0, 8
    if u8:
        x = (x + 127.5).round().clamp(0, 255).to(t.uint8).contiguous()
        flags, isz = hip.DD_CHAIN_U8_INPUT, 2
    per = 1 if fm else 2
    for phi in (0,) + tuple(phis):
        off = (phi - START) % M
        outs = []
        for pat in PADDED_PATTERNS:
            out, got, kern = _fused_once(g, _hamming(ntaps), M, fm, x, isz, n, START, off, flags, fill=pat)
            assert kern == hip.DD_KERNEL_DECIM_BLOCKS, (phi, kern)
            outs.append((out, got))
        assert outs[0][1] == len(range(off, n, M)) - (1 if fm else 0)
        _assert_identical(g, outs, per)


@pytest.mark.parametrize("M,ntaps,phi", [(32, 151, 26), (40, 151, 38), (12, 65, 11)])
@pytest.mark.parametrize("fm", [True, False])
def test_padded_chunk_list_in_one_launch_equals_the_chunk_loop_after_lds_fills(g, M, ntaps, phi, fm):
    """dd_fused_process_chunks (one k_chain_decim_b launch for the whole list) at a stream phase where rows read past their last staged
    sample, after LDS fills: the outputs and per-chunk counts of the dd_fused_process loop, bit for bit."""
    t, lib, hip = g.torch, g.lib, g.hip
    n = 40000
    cuts = [0, 1, 2047, 2048 + 5, 9001, 20011, 20012, n]
    x = g.bench.make_input(t, n, START, g.dev, 5 + M)
    off0 = (phi - START) % M
    taps = _hamming(ntaps)
    per = 1 if fm else 2
    nfl = per * (n // M + 8)
    cyc = hip.cycles_q64(25000.0, FS)
    # the loop (after a NaN fill): every chunk carries the filter history, the FM sample and the decimation phase on
    fir, fmh = _fused_handles(g, taps, fm)
    hip.check(lib.dd_debug_fill_lds(0xFFFFFFFF, g.stream), "fill")
    ref = t.full((nfl,), float("nan"), dtype=t.float32, device=g.dev)
    counts, pos, off = [], 0, off0
    got = C.c_int64(0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        hip.check(lib.dd_fused_process(fir, fmh, x.data_ptr() + 8 * a, ref.data_ptr() + 4 * per * pos, b - a, 1, cyc, START + a, M, off, 0, 1,
                                       C.byref(got), g.stream), "dd_fused_process")
        counts.append(got.value)
        pos += got.value
        off = (off - (b - a)) % M
    t.cuda.synchronize()
    lib.dd_fir_destroy(fir)
    if fmh is not None:
        lib.dd_fm_destroy(fmh)
    tot = per * pos
    assert bool(t.isfinite(ref[:tot]).all())
    bounds = (C.c_int64 * len(cuts))(*cuts)
    nout = (C.c_int64 * (len(cuts) - 1))()
    for pat in PADDED_PATTERNS:
        fir, fmh = _fused_handles(g, taps, fm)
        hip.check(lib.dd_debug_fill_lds(pat, g.stream), "fill")
        out = t.full((nfl,), float("nan"), dtype=t.float32, device=g.dev)
        hip.check(lib.dd_fused_process_chunks(fir, fmh, x.data_ptr(), out.data_ptr(), bounds, len(cuts) - 1, 1, cyc, START, M, off0, 0, nout,
                                              g.stream), "dd_fused_process_chunks")
        t.cuda.synchronize()
        assert lib.dd_fir_last_kernel(fir) == hip.DD_KERNEL_DECIM_BLOCKS
        lib.dd_fir_destroy(fir)
        if fmh is not None:
            lib.dd_fm_destroy(fmh)
        assert list(nout) == counts
        diff = int((out[:tot].view(t.int32) != ref[:tot].view(t.int32)).sum())
        assert diff == 0, "%d of %d output words differ from the chunk loop (fill %#x)" % (diff, tot, pat)


# ---- who owns device memory: handles created, used once and destroyed over and over; grow-only buffers before and after growing
def _bits_equal(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), "%s: bits differ" % (what,)


def test_handles_survive_create_use_destroy_rounds(g):
    """Twenty rounds; each creates, uses once and drops one handle of every family: the M = 1 chain with the running-sum state
    (hamming(255)), the transform state (hamming(200)) and the MFMA fragments (hamming(63)), the block-sum decimator with its
    tap cache and dd_fm (blackmanHarris(151), / 34, FM), dd_iir on its one-lane path (3000 samples) and its block-parallel
    path (5000 samples; matrices and scratch), dd_rpoly, dd_fmad, and a raw dd_fir + dd_fm pair through the C ABI.
    filters.pool_clear() ends every round: without it the pool keeps the dd_fir handles and dd_fir_destroy never runs.
    Every round's outputs are the first round's, bit for bit."""
    hip = g.hip
    import directdemod_amd.comm as comm
    import directdemod_amd.demod_fm as demod_fm
    import directdemod_amd.filters as filters
    import directdemod_amd.resample as resample
    fs2 = 2048000
    x = O.grid_c64(O.synth_iq_fm(70000, FS, 41, f_carrier=25e3))
    x2 = O.grid_c64(O.synth_iq_fm(70000, fs2, 42, f_carrier=30e3))
    a = np.abs(x).astype(np.float32)
    xd = g.bench.make_input(g.torch, 70000, 0, g.dev, 44)

    def one_round(first):
        outs = []
        f255, f200, f63, bh = filters.hamming(255), filters.hamming(200), filters.hamming(63), filters.blackmanHarris(151)
        fm, fm2 = demod_fm.demod_fm(), demod_fm.demod_fm()
        outs.append(comm.commSignal(FS, x).offsetFreq(25000.0).filter(f255).funcApply(fm.demod).signal)
        outs.append(comm.commSignal(FS, x[:20000]).offsetFreq(25000.0).filter(f200).signal)
        outs.append(comm.commSignal(FS, x[:20001]).filter(f63).signal)
        outs.append(comm.commSignal(fs2, x2).offsetFreq(30000.0).filter(bh).bwLim(60000, uniq="First").funcApply(fm2.demod).signal)
        if first:
            assert f255._last_kernel() == hip.DD_KERNEL_COS_RS
            assert f200._last_kernel() == hip.DD_KERNEL_FFT_OS
            assert f63._last_kernel() in (hip.DD_KERNEL_MFMA_AB, hip.DD_KERNEL_MFMA_TILES)
            assert bh._last_kernel() == hip.DD_KERNEL_DECIM_BLOCKS
        outs.append(comm.commSignal(FS, a[:3000]).filter(filters.butter(FS, 4160.0)).signal)
        outs.append(comm.commSignal(FS, a[:5000]).filter(filters.butter(FS, 4160.0)).signal)
        outs.append(comm.commSignal(FS, a[:30000]).resamplePoly(resample.polyResampler(FS, 20800)).signal)
        outs.append(demod_fm.demod_fmAD().demod(x[:4096]))
        out, got, kern = _fused_once(g, O.win_blackmanharris(151), 34, True, xd, 8, 70000, 0, 0, 0)
        assert kern == hip.DD_KERNEL_DECIM_BLOCKS and got > 0
        outs.append(out[:got].cpu().numpy())
        outs = [np.asarray(v).copy() for v in outs]
        del f255, f200, f63, bh, fm, fm2
        filters.pool_clear()
        return outs

    ref = one_round(True)
    for k, v in enumerate(ref):
        assert v.size > 0 and np.all(np.isfinite(v)), k
    for rnd in range(1, 20):
        for k, (got, want) in enumerate(zip(one_round(False), ref)):
            _bits_equal(got, want, "round %d, output %d" % (rnd, k))


def test_grow_only_buffers_give_the_same_bits_after_growing(g):
    """The grow-only buffers on the handles, before and after they grow: dd_iir's scratch (one butter handle at 5000, 70 000 and
    5000 samples again, storeState=False, block-parallel path each time) and dd_fir's chunk-list image (one handle: a list of 2
    chunks, of 16, of 2 again through k_chain_decim_multi).  Each result is what a fresh handle gives for that input, bit for bit."""
    t, lib, hip = g.torch, g.lib, g.hip
    import directdemod_amd.filters as filters
    x = O.grid_c64(O.synth_iq_fm(70000, FS, 43, f_carrier=25e3))
    flt = filters.butter(FS, 40000.0, storeState=False)
    for n in (5000, 70000, 5000):
        got = np.asarray(flt.applyOn(x[:n]))
        want = np.asarray(filters.butter(FS, 40000.0, storeState=False).applyOn(x[:n]))
        assert got.shape == (n,) and np.all(np.isfinite(got.view(np.float64)))
        _bits_equal(got, want, "butter, %d samples" % n)

    n, M, taps = 64000, 5, _hamming(63)
    xd = g.bench.make_input(t, n, 0, g.dev, 99)
    cyc = hip.cycles_q64(25000.0, FS)
    lists = ([0, 30001, n], list(range(0, n + 1, 4000)), [0, 30001, n])
    assert [len(c) - 1 for c in lists] == [2, 16, 2]

    def run(fir, fmh, cuts):
        bounds = (C.c_int64 * len(cuts))(*cuts)
        nout = (C.c_int64 * (len(cuts) - 1))()
        out = t.full((n // M + 8,), float("nan"), dtype=t.float32, device=g.dev)
        hip.check(lib.dd_fused_process_chunks(fir, fmh, xd.data_ptr(), out.data_ptr(), bounds, len(cuts) - 1, 1, cyc, 0, M, 0, 0, nout,
                                              g.stream), "dd_fused_process_chunks")
        t.cuda.synchronize()
        assert lib.dd_fir_last_kernel(fir) == hip.DD_KERNEL_DECIM_MULTI
        tot = sum(nout)
        assert tot > 0 and bool(t.isfinite(out[:tot]).all())
        return out[:tot].cpu().numpy(), list(nout)

    fir, fmh = _fused_handles(g, taps, True)
    try:
        for cuts in lists:
            hip.check(lib.dd_fir_reset(fir, hip.DD_HIST_ZEROS, None, g.stream), "dd_fir_reset")
            hip.check(lib.dd_fm_reset(fmh), "dd_fm_reset")
            got, cnt = run(fir, fmh, cuts)
            f2, m2 = _fused_handles(g, taps, True)
            try:
                want, cnt2 = run(f2, m2, cuts)
            finally:
                lib.dd_fir_destroy(f2)
                lib.dd_fm_destroy(m2)
            assert cnt == cnt2
            _bits_equal(got, want, "chunk list of %d" % (len(cuts) - 1))
    finally:
        lib.dd_fir_destroy(fir)
        lib.dd_fm_destroy(fmh)
