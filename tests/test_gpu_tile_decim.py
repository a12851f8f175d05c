"""
The tile family of the fused chain -- k_chain_decim (edge tiles, short or unaligned chunks), k_chain_decim_p<false|true> (persistent
workgroups over a chunk's interior tiles) and k_chain_decim_multi<false|true> (the same for a whole chunk list) -- against the float64
oracle at the shapes the dispatcher sends it since the row kernels took even M in [8, 64] with 2..256 taps: odd M, M < 8, M > 64 (the
reference's own /68, /92 and /108), and more than 256 taps.

Every run goes through the raw C-ABI (dd_chain_create / dd_chain_process / dd_chain_process_chunks) under the default selector, with
the NCO on (30 kHz at 2.048 MS/s), and the kernel id of every chunk is held against what dd_debug_decim_tile_plan predicts, so that a
change of the dispatcher or of the plan cannot quietly take these tests off the kernels they are about.

Tolerances: up to 256 taps the project's own (FIR_TOL, fm_check of test_gpu_parity.py).  Beyond 256 taps the project states none, and
none is invented: the test forms, from the reference alone, a float32 model of the same direct form (the oracle's samples after the NCO
rounded to complex64, float32 taps, one float32 multiply and add per tap in tap order), measures its relative error e_model against
the float64 oracle, and bounds the kernel at max(FIR_TOL, 4 e_model) -- the factor 4 covers fused-versus-separate rounding and the NCO
table -- with the three FM tiers scaled by the same ratio.  Measured on an MI355X (kernel error / e_model, complex output, the worse of
the aligned and the odd-start run): (34, 257) 1.0e-6 / 9.8e-7, (50, 300) 9.7e-7 / 9.0e-7, (8, 513) 1.1e-6 / 1.1e-6, (8, 515) 1.2e-6 /
1.2e-6, (16, 600) 1.3e-6 / 1.2e-6, (2, 6200) 4.4e-6 / 4.4e-6; the FM angles of those shapes are within 5.2e-6 rad of the oracle's.
"""
import ctypes as C
import functools
import os
from collections import namedtuple

import numpy as np
import pytest

from oracle import dd_oracle as O
from test_gpu_parity import FIR_TOL, FM_MAX, FM_MED, FM_WELL, rel_err

pytestmark = pytest.mark.gpu

FS, FC = 2048000, 30000.0
SPAN_MAX, THREADS = 6144, 256

# >= 64 interior tiles in the long chunk: M > 64 (the reference's decimations first), odd M, M < 8, more than 256 taps with an even M the
# row kernels would otherwise take, taps past the 512 carried samples an edge tile fetches in its first two rounds, one tap, and every
# K mod 8 remainder of the odd-M (9, 7..9) and even-M (6, 15..17) tap loops
LONG = [(108, 151), (68, 127), (92, 151), (66, 64), (3, 151), (7, 255), (33, 64), (65, 127), (2, 64), (4, 33), (6, 100), (200, 33), (34, 257),
        (50, 300), (8, 513), (8, 515), (16, 600), (3, 1), (5, 2), (9, 7), (9, 8), (9, 9), (6, 15), (6, 16), (6, 17)]
# spans beyond DD_DECIM_SPAN_MAX (T = 2; S = 6232, 8150, 12401, 6203): the trailing staging loop, the last three beyond 64 KB of LDS
LARGE = [(3100, 33), (4000, 151), (6200, 2), (2, 6200)]


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from directdemod_amd import _hip
    _hip.require_gpu()
    return _hip


def _taps(M, K):
    if K == 1:
        return np.array([1.0])
    if K == 2:
        return np.array([0.5, 0.5])
    return np.ascontiguousarray(O.firwin_lowpass(K, 0.45 / M))


def _tile_T(M, K):
    return min(THREADS, max(2, int((SPAN_MAX - K - (M - 1)) / M) + 1))


def _next_off(pos, M):
    return (M - pos % M) % M


Stream = namedtuple("Stream", "bounds i_empty i_long raw")


@functools.lru_cache(maxsize=None)
def _stream(M, K):
    """the chunk bounds and the raw u8 samples of shape (M, K).  Long shapes: ragged cuts, a chunk that keeps no sample (behind a
    one-sample chunk where the decimation phase would otherwise be 0: only a chunk shorter than its phase keeps nothing), one chunk of
    72 T M + 2 K samples, [1, 20000 + M].  Large-span shapes: the ragged cuts and one chunk to about 40 M samples (13000 for K = 6200)."""
    if (M, K) in LARGE:
        total = 13000 if K == 6200 else 40 * M
        cuts = [1, 2, K - 1, 3, M - 1, M, M + 1]
        cuts.append(total - sum(cuts))
        i_empty = i_long = -1
    else:
        cuts = [1, 2, K - 1, 3, M - 1, M, M + 1, 2047, 4096 + 5, 7]
        if _next_off(sum(cuts), M) == 0:
            cuts.append(1)
        i_empty = len(cuts)
        cuts.append(min(_next_off(sum(cuts), M), 5))
        i_long = len(cuts)
        cuts += [72 * _tile_T(M, K) * M + 2 * K, 1, 20000 + M]
    bounds = np.cumsum([0] + cuts).astype(np.int64)
    raw = O.synth_iq_fm(int(bounds[-1]), FS, 500 + M + K, f_carrier=FC, f_mod=900.0, dev=3.0)
    raw.setflags(write=False)
    bounds.setflags(write=False)
    return Stream(bounds, i_empty, i_long, raw)


@functools.lru_cache(maxsize=None)
def _reference(M, K):
    """(the float64 oracle's kept FIR outputs, e_model) -- e_model: the relative error of the float32 direct-form model, K > 256 only"""
    st = _stream(M, K)
    taps = _taps(M, K)
    xr = O.nco(O.grid_c64(st.raw), FC, FS)
    y = O.FilterState(taps).applyOn(xr)[::M]
    e_model = None
    if K > 256:
        xx = np.concatenate([np.ones(K - 1, dtype=np.complex64), xr.astype(np.complex64)])         # (the carried history of a stream start: ones)
        g = taps[::-1].astype(np.float32)
        at = np.arange(0, len(xr), M)
        acc = np.zeros(len(at), dtype=np.complex64)
        for j in range(K):
            acc += g[j] * xx[at + j]
        assert acc.dtype == np.complex64
        e_model = rel_err(acc, y)
    y.setflags(write=False)
    return y, e_model


def _plan(hip, L, K, M, off, fm, has_last, u8, align):
    out = (C.c_int64 * 9)()
    hip.check(hip.lib().dd_debug_decim_tile_plan(int(L), K, M, off, int(fm), int(has_last), int(u8), int(align), out), "dd_debug_decim_tile_plan")
    return dict(zip(("T", "nblocks", "S", "S2", "persistent", "lo", "hi", "lds", "lds_p"), list(out)))


class Chain:
    """a dd_chain over device input at `ptr` (stream sample i at ptr + isz i) that mirrors the chunker variables the plan door needs"""

    def __init__(self, hip, M, K, fm_on, u8, ptr):
        self.hip, self.lib, self.M, self.K, self.fm_on, self.u8, self.ptr = hip, hip.lib(), M, K, fm_on, u8, ptr
        self.isz = 2 if u8 else 8
        self.odt = np.dtype(np.float32 if fm_on else np.complex64)
        taps = _taps(M, K)
        self.h = C.c_void_p()
        flags = hip.DD_CHAIN_NCO | (hip.DD_CHAIN_FM if fm_on else 0) | (hip.DD_CHAIN_U8_INPUT if u8 else 0)
        hip.check(self.lib.dd_chain_create(C.byref(self.h), taps.ctypes.data_as(C.POINTER(C.c_double)), K, hip.cycles_q64(FC, FS), M, flags))
        self.has_last = 0

    def close(self):
        self.lib.dd_chain_destroy(self.h)

    def predict(self, a, b):
        """(kernel id, plan) of the chunk [a, b), and the chunker variables moved on behind it"""
        hip, M = self.hip, self.M
        n, off = int(b - a), _next_off(int(a), M)
        if len(range(off, n, M)) == 0:
            return hip.DD_KERNEL_NONE, None
        p = _plan(hip, n, self.K, M, off, self.fm_on, self.has_last, self.u8, (self.ptr + self.isz * int(a)) % 16)
        if self.fm_on:
            self.has_last = 1
        return (hip.DD_KERNEL_DECIM_PERSISTENT if p["persistent"] else hip.DD_KERNEL_DECIM_TILES), p

    def loop(self, bounds, fill=None):
        """the chunks one by one; (outputs, [(kernel id, plan)] per chunk), self.counts the outputs per chunk.  fill: an LDS pattern put
        down before every launch"""
        hip, lib = self.hip, self.lib
        self.counts = []
        o = hip.DevArray(int(bounds[-1] - bounds[0]) // self.M + 2, self.odt)
        opos, seen = 0, []
        for a, b in zip(bounds[:-1], bounds[1:]):
            n = int(b - a)
            no = lib.dd_chain_out_count(self.h, n)
            want, p = self.predict(a, b)
            if fill is not None:
                hip.check(lib.dd_debug_fill_lds(fill, None))
            got = C.c_int64(-1)
            hip.check(lib.dd_chain_process(self.h, self.ptr + self.isz * int(a), o.ptr + self.odt.itemsize * opos, n, C.byref(got), None))
            assert got.value == no, (a, b, got.value, no)
            assert lib.dd_chain_last_kernel(self.h) == want, (int(a), int(b), lib.dd_chain_last_kernel(self.h), want, p)
            seen.append((want, p))
            self.counts.append(no)
            opos += no
        return o.to_host()[:opos], seen

    def chunk_list(self, bounds):
        """the same chunks through dd_chain_process_chunks; (outputs, outputs per chunk, kernel id)"""
        hip, lib = self.hip, self.lib
        o = hip.DevArray(int(bounds[-1] - bounds[0]) // self.M + 2, self.odt)
        bd = np.ascontiguousarray(bounds, dtype=np.int64)
        nout = np.full(len(bd) - 1, -1, dtype=np.int64)
        hip.check(lib.dd_chain_process_chunks(self.h, self.ptr, o.ptr, bd.ctypes.data_as(C.POINTER(C.c_int64)), len(bd) - 1,
                                              nout.ctypes.data_as(C.POINTER(C.c_int64)), None))
        return o.to_host()[:int(nout.sum())], nout, lib.dd_chain_last_kernel(self.h)


def _device_input(hip, raw, u8, shift=0):
    """(owner, pointer of stream sample 0) of the raw u8 samples, or of the complex64 samples they widen to.  shift = 1 (u8): the stream
    sits one sample into its buffer, every pointer 2 bytes on"""
    if not u8:
        d = hip.DevArray.from_host(raw if np.iscomplexobj(raw) else O.grid_c64(raw), dtype=np.complex64)
        return d, d.ptr
    d = hip.DevArray.from_host(np.concatenate([np.zeros(2 * shift, dtype=np.uint8), raw.reshape(-1)]))
    return d, d.ptr + 2 * shift


def _fm_check(got, y, scale, M, K):
    """fm_check of test_gpu_parity.py on the oracle's kept FIR outputs y, its three tiers times `scale` (1 up to 256 taps)"""
    ref, _ = O.fm_demod(y, None)
    mag = np.abs(y[1:] * np.conj(y[:-1]))
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    mask = mag >= 1e-3 * np.median(mag)
    # what fm_check leaves out must be a small share, or the comparison says little.  The outputs whose windows still hold the carried
    # history of a stream start (ones, against samples of amplitude 60) are small by construction; where they alone are more than
    # that share -- 6200 taps over 13000 samples -- the share is taken behind them (the complex-output case checks them all)
    lead = min(len(mask), -(-(K - 1) // M))
    left_out = np.mean(~mask) if lead <= 0.01 * len(mask) else np.mean(~mask[lead:])
    assert left_out <= 0.01, "fm_check leaves out %.3g of the outputs" % left_out
    d = np.abs(np.angle(np.exp(1j * (got - ref))))
    well = mag >= 0.1 * np.median(mag)
    fig = (float(np.max(d[mask])), float(np.max(d[well])), float(np.median(d)))
    print("  fm: max %.3g (bound %.3g), well-conditioned max %.3g (%.3g), median %.3g (%.3g), left out %.3g" %
          (fig[0], FM_MAX * scale, fig[1], FM_WELL * scale, fig[2], FM_MED * scale, np.mean(~mask)))
    assert fig[0] <= FM_MAX * scale, "max wrapped FM error %g" % fig[0]
    assert fig[1] <= FM_WELL * scale, "max wrapped FM error on well-conditioned outputs %g" % fig[1]
    assert fig[2] <= FM_MED * scale, "median FM error %g" % fig[2]


def _check_against_oracle(got, M, K, fm_on, what):
    y, e_model = _reference(M, K)
    bound = FIR_TOL if e_model is None else max(FIR_TOL, 4 * e_model)
    print("%s M %d K %d fm %d: e_model %s, bound %.3g" % (what, M, K, fm_on, "-" if e_model is None else "%.3g" % e_model, bound))
    if fm_on:
        _fm_check(got, y, bound / FIR_TOL, M, K)
    else:
        e = rel_err(got, y)
        print("  fir: rel err %.3g" % e)
        assert e < bound


def _names(hip, seen):
    name = {hip.DD_KERNEL_NONE: "none", hip.DD_KERNEL_DECIM_TILES: "tiles", hip.DD_KERNEL_DECIM_PERSISTENT: "persistent"}
    return " ".join(name[k] for k, _ in seen)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fm_on", [False, True])
@pytest.mark.parametrize("M,K", LONG + LARGE)
def test_tile_kernels_shapes_cuts_and_u8(hip, M, K, fm_on, u8):
    """Ragged cuts (one sample, shorter than the taps, around M), a chunk that keeps no sample, one chunk with an interior run for the
    persistent kernel, and a tail, chunk by chunk with carried state: output counts, the kernel id of every chunk as the plan door
    predicts it, and the whole output against the float64 oracle.  Raw u8 input once more with every pointer 2 bytes on, which puts the
    long chunk on an odd sample: its 16-byte loads would sit on 2 mod 4, so all of it must go through k_chain_decim's edge path."""
    st = _stream(M, K)
    large = (M, K) in LARGE
    TILES, PERS, NONE = hip.DD_KERNEL_DECIM_TILES, hip.DD_KERNEL_DECIM_PERSISTENT, hip.DD_KERNEL_NONE
    # (u8: the buffer that puts the long chunk on a 4-byte boundary first)
    shift = int(st.bounds[st.i_long]) & 1 if (u8 and not large) else 0
    d, ptr = _device_input(hip, st.raw, u8, shift)
    ch = Chain(hip, M, K, fm_on, u8, ptr)
    got, seen = ch.loop(st.bounds)
    ch.close()
    print("kernels M %d K %d fm %d u8 %d: %s" % (M, K, fm_on, u8, _names(hip, seen)))
    kinds = [k for k, _ in seen]
    if large:
        assert set(kinds) <= {TILES, NONE} and TILES in kinds
        assert all(p["T"] == 2 and p["S"] > SPAN_MAX for _, p in seen if p)
        if (M, K) != (3100, 33):
            assert max(p["lds"] for _, p in seen if p) > 64 * 1024
    else:
        assert kinds[st.i_empty] == NONE and kinds[st.i_long] == PERS and TILES in kinds
        assert seen[st.i_long][1]["hi"] - seen[st.i_long][1]["lo"] >= 64
    _check_against_oracle(got, M, K, fm_on, "aligned")
    if u8 and not large:
        d, ptr = _device_input(hip, st.raw, u8, 1 - shift)
        ch = Chain(hip, M, K, fm_on, u8, ptr)
        got, seen = ch.loop(st.bounds)
        ch.close()
        assert seen[st.i_long][0] == TILES and seen[st.i_long][1]["nblocks"] >= 64
        _check_against_oracle(got, M, K, fm_on, "odd start")


def _without_empty_chunks(bounds, M):
    """the bounds of a stream that starts at sample 0 without the start of any chunk that keeps no sample"""
    return np.array([b for i, b in enumerate(bounds)
                     if i in (0, len(bounds) - 1) or len(range(_next_off(int(b), M), int(bounds[i + 1] - b), M))], dtype=np.int64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fm_on", [False, True])
@pytest.mark.parametrize("M,K", [(108, 151), (3, 151), (7, 255), (65, 127), (50, 300)])
def test_tile_chunk_lists_equal_the_chunk_loop(hip, M, K, fm_on, u8):
    """dd_chain_process_chunks over the same bounds without the chunk that keeps no sample -- chunks with and without an interior run,
    chunks shorter than K - 1 -- is ONE k_chain_decim_multi launch and gives the chunk loop's bits; with that chunk in the list it falls
    back to the loop, and still gives the same bits."""
    st = _stream(M, K)
    shift = int(st.bounds[st.i_long]) & 1 if u8 else 0
    d, ptr = _device_input(hip, st.raw, u8, shift)
    full = st.bounds
    # (every chunk that keeps no sample -- the one put there for it, and the ragged cuts that fall between two multiples of M -- gives
    #  its few samples to the chunk before it)
    kept = _without_empty_chunks(full, M)
    assert st.bounds[st.i_empty] not in kept and st.bounds[st.i_long] in kept and len(kept) >= 8
    for bounds, multi in ((kept, True), (full, False)):
        one = Chain(hip, M, K, fm_on, u8, ptr)
        want, seen = one.loop(bounds)
        one.close()
        ch = Chain(hip, M, K, fm_on, u8, ptr)
        got, nout, kern = ch.chunk_list(bounds)
        ch.close()
        assert (kern == hip.DD_KERNEL_DECIM_MULTI) == multi, (kern, multi)
        assert list(nout) == one.counts
        if multi:
            assert any(p and p["persistent"] for _, p in seen) and any(p and not p["persistent"] for _, p in seen)
            assert any(b - a < K - 1 for a, b in zip(bounds[:-1], bounds[1:]))
        assert got.dtype == want.dtype and len(got) == len(want) and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fm_on", [False, True])
def test_tile_chunk_list_of_a_one_tap_filter_falls_back_to_the_loop(hip, fm_on, u8):
    """K = 1 carries no history for the in-launch hand-over: the list is run chunk by chunk, same bits"""
    M, K = 3, 1
    st = _stream(M, K)
    d, ptr = _device_input(hip, st.raw, u8, int(st.bounds[st.i_long]) & 1 if u8 else 0)
    bounds = _without_empty_chunks(st.bounds, M)            # (so that nothing but the single tap sends the list to the loop)
    ch = Chain(hip, M, K, fm_on, u8, ptr)
    want, _ = ch.loop(bounds)
    ch.close()
    ch = Chain(hip, M, K, fm_on, u8, ptr)
    got, nout, kern = ch.chunk_list(bounds)
    ch.close()
    assert kern in (hip.DD_KERNEL_DECIM_TILES, hip.DD_KERNEL_DECIM_PERSISTENT)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fm_on", [False, True])
@pytest.mark.parametrize("M,K", [(108, 151), (3, 151), (7, 255)])
def test_a_sample_reaches_the_outputs_of_its_own_windows_only(hip, M, K, fm_on, u8):
    """One marked sample per run -- a chunk's first and last sample, the first and the last sample an interior tile stages, the first
    sample past that tile's span (inside the rounding of its 16-byte loads), the last sample of the stream -- reaches exactly the outputs
    p with p M - (K - 1) <= at <= p M (FM: the pairs that hold such a p) and nothing else: no tile reads a neighbour's sample, no load
    past a span is used.  complex64: the mark is a NaN, which no tap can round away, and the non-finite outputs are exactly that set.
    Raw u8 cannot hold a NaN: the sample has both bytes flipped by 128 instead, and the outputs whose bits differ from the unmarked run
    lie in that set -- and are not none where the set holds a whole window, whose middle taps a change of 128 cannot round away."""
    n0, n2 = K + M + 701, 5000 + M
    nlong = 72 * _tile_T(M, K) * M + 2 * K
    bounds = np.cumsum([0, n0, nlong, n2]).astype(np.int64)
    L = int(bounds[-1])
    raw = O.synth_iq_fm(L, FS, 900 + M + K, f_carrier=FC, f_mod=900.0, dev=3.0)
    shift = int(bounds[1]) & 1 if u8 else 0

    def run(data):
        d, ptr = _device_input(hip, data, u8, shift)
        ch = Chain(hip, M, K, fm_on, u8, ptr)
        got, seen = ch.loop(bounds)
        ch.close()
        assert [k for k, _ in seen] == [hip.DD_KERNEL_DECIM_TILES, hip.DD_KERNEL_DECIM_PERSISTENT, hip.DD_KERNEL_DECIM_TILES]
        return got, seen[1][1]

    x = O.grid_c64(raw)
    base, p = run(raw if u8 else x)
    assert np.all(np.isfinite(base))
    b = (p["lo"] + p["hi"]) // 2
    off = _next_off(int(bounds[1]), M)
    pfirst = -1 + b * (p["T"] - 1) if fm_on else b * p["T"]               # (an FM sample precedes the long chunk: s = 0)
    ns = int(bounds[1]) + off + pfirst * M - (K - 1)
    kept = np.arange(0, L, M)
    for at in (int(bounds[1]), int(bounds[2]) - 1, ns, ns + p["S"] - 1, ns + p["S"], L - 1):
        assert bounds[1] <= at < L
        hit = (kept - (K - 1) <= at) & (at <= kept)
        if fm_on:
            hit = hit[1:] | hit[:-1]
        if u8:
            data = raw.copy()
            data[at] ^= 0x80
            got, _ = run(data)
            diff = (_bits(got) != _bits(base)).reshape(len(got), -1).any(axis=1)
            assert not np.any(diff & ~hit), (at, np.nonzero(diff)[0], np.nonzero(hit)[0])
            assert np.any(diff) or hit.sum() < -(-K // M), at
        else:
            data = x.copy()
            data[at] = np.nan + 0j
            got, _ = run(data)
            bad = ~np.isfinite(got)
            assert np.array_equal(bad, hit), (at, np.nonzero(bad)[0], np.nonzero(hit)[0])


@pytest.mark.parametrize("fm_on", [False, True])
@pytest.mark.parametrize("M,K", [(108, 151), (3, 151), (8, 513), (3100, 33)])
def test_tile_kernels_do_not_read_lds_they_have_not_written(hip, M, K, fm_on):
    """LDS is not cleared between workgroups: the same stream after dd_debug_fill_lds(all ones: NaNs) and after dd_debug_fill_lds(0) before
    every launch gives the same bits (a tap loop or a discriminator that reads past what its tile staged would see the fill)."""
    st = _stream(M, K)
    d, ptr = _device_input(hip, st.raw, False)
    outs = []
    for fill in (0xFFFFFFFF, 0):
        ch = Chain(hip, M, K, fm_on, False, ptr)
        got, _ = ch.loop(st.bounds, fill=fill)
        ch.close()
        outs.append(got)
    assert np.all(np.isfinite(outs[0]))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
