// Fused hot path:  offsetFreq (NCO) -> FIR (state carried) -> bwLim (integer decimation, only kept outputs are
// computed) -> demod_fm.  Reference call sites: decode_noaa.py:623, decode_fm.py:64-68, decode_afsk1200.py:79-94,
// tutorial/3_chunking.py:24-38; operators comm.py:63-130, filters.py:53-75, demod_fm.py:29-51.
//
// This file is the host layer every product call goes through:
//   handles       dd_fir (taps + carried history), dd_fm (last sample), dd_chain (both + the chunker variables)
//   dispatcher    chain_select: which kernel family takes a launch -- the ONLY place that rule lives
//   launch plans  dense / tile kernels (launch_dense, decim_plan, persistent_grid); the other families plan in their own units
//   entry points  dd_fused_process*, dd_chain_process*, dd_fir_c64, dd_fm_discrim_c64, dd_debug_*
// The f32 direct-form kernels this unit compiles are in dd_chain_tile_kernels.h; the other families are units of their
// own: dd_decimw.hip (row kernels), dd_cosfir.hip (k_chain_cos1k), dd_fftfir.hip (k_chain_fft1k), dd_mfma.hip (MFMA).
#include "dd_chain_tile_kernels.h"
#include "dd_cosfir.h"
#include "dd_fftfir.h"
#include <stdlib.h>
#include <atomic>
#include <mutex>

// ---------------------------------------------------------------- dispatcher
// The process-wide selector word: which kernel runs is decided by tap class, unless a tool or test has forced one through
// dd_debug_select_kernel (a debug entry like dd_debug_fill_lds); the environment variable DD_MFMA_KERNEL only seeds the
// word, read ONCE when the first chain is launched (no getenv in the launch path).
enum { DD_KSEL_UNREAD = -1, DD_KSEL_AUTO = 0, DD_KSEL_AB = 1, DD_KSEL_FFT1K = 2, DD_KSEL_COS1K = 3, DD_KSEL_DECIMP = 4 };
static std::atomic<int> g_kernel_sel{DD_KSEL_UNREAD};
static int kernel_sel_parse(const char* name) {
    if (!name || !*name || strcmp(name, "auto") == 0) return DD_KSEL_AUTO;
    if (strcmp(name, "ab") == 0) return DD_KSEL_AB;
    if (strcmp(name, "fft1k") == 0) return DD_KSEL_FFT1K;
    if (strcmp(name, "cos1k") == 0) return DD_KSEL_COS1K;
    if (strcmp(name, "decimp") == 0) return DD_KSEL_DECIMP;
    return -2;
}
static int kernel_sel() {
    int c = g_kernel_sel.load(std::memory_order_relaxed);
    if (c == DD_KSEL_UNREAD) {
        c = kernel_sel_parse(getenv("DD_MFMA_KERNEL"));
        if (c < 0) c = DD_KSEL_AUTO;
        g_kernel_sel.store(c, std::memory_order_relaxed);
    }
    return c;
}
extern "C" int dd_debug_select_kernel(const char* name) {
    const int c = kernel_sel_parse(name);
    if (c < 0) {
        dd_set_error("dd_debug_select_kernel: unknown kernel '%s' (auto, ab, fft1k, cos1k, decimp)", name);
        return DD_ERR_INVALID;
    }
    g_kernel_sel.store(c, std::memory_order_relaxed);
    return DD_OK;
}

// Which kernel family takes a launch: a pure function of the taps (K of them), the decimation M, the DD_CHAIN_* flags, the
// low bits of the input pointer and the selector word `sel`.  `skip` is a set of (1 << family) bits the caller has found
// unusable (their state could not be created): such a family falls through to the next one.  The finer kernel id inside a
// family (tiles / persistent, MFMA tiles / ab, wave / blocks) is the business of the family's own launcher and plan.
//   M > 1   rows    k_chain_decim_b / _w (dd_decimw.hip): even M in [8, 64], 2..256 taps, complex64 input on an 8-byte or raw
//                   u8 input on a 2-byte boundary: one wave per row of kept outputs on the absolute decimation grid.
//                   Selector "decimp" keeps them off: the tile kernels instead.  (DD_CHAIN_FORCE_DIRECT does not: it
//                   names the M = 1 matrix / transform kernels.)
//           tiles   k_chain_decim / _p / _multi: everything else.
//   M == 1  in this order, each only where the one before does not apply:
//           dense   k_chain_dense, f32 direct form: DD_CHAIN_FORCE_DIRECT, or more than 257 taps (beyond the MFMA tap classes;
//                   the running-sum and transform kernels are reachable only below that bound);
//           cos1k   k_chain_cos1k: 255 taps a0 + a1 cos(2 pi k / 254) (filters.hamming; dd_cos1k_supported declines a near-pure
//                   cosine) under selector "auto" or "cos1k", a third of the overlap-save form's arithmetic.  "ab", "fft1k" and
//                   "decimp" keep it off, and so does DD_CHAIN_TIGHT (the caller asks for the transform kernel's stop-band bound);
//           fft1k   k_chain_fft1k, up to 256 taps: under selector "fft1k" wherever it applies, else in the 162..257-tap class for
//                   every selector but "ab".  Its time does not depend on the tap count (0.221 ms per 2^26 samples, 0.207 from
//                   raw u8); the MFMA kernel's does: 0.227 ms in that class, 0.20 below.  Any input alignment.  So "decimp" with
//                   filters.hamming(255) lands here;
//           mfma    k_chain_mfma_ab / _edge: the rest ("ab" forces them in the 162..257-tap class too);
//           dense   when nothing above could be created.
static int chain_select(const double* taps, int K, int M, int flags, unsigned in_align, int sel, int skip) {
    if (M > 1) {
        const void* in = reinterpret_cast<const void*>((uintptr_t)in_align);
        return (sel != DD_KSEL_DECIMP && dd_decimw_supported(K, M, flags, in)) ? DD_FAMILY_ROWS : DD_FAMILY_TILES;
    }
    const int ksteps = dd_mfma_supported(K, M);
    if ((flags & DD_CHAIN_FORCE_DIRECT) || !ksteps) return DD_FAMILY_DENSE;
    auto open = [skip](int family) { return !(skip & (1 << family)); };
    if (open(DD_FAMILY_COS1K) && (sel == DD_KSEL_AUTO || sel == DD_KSEL_COS1K) && K == 255 && !(flags & DD_CHAIN_TIGHT) &&
        dd_cos1k_supported(taps, K, M, flags))
        return DD_FAMILY_COS1K;
    if (open(DD_FAMILY_FFT1K) && (sel == DD_KSEL_FFT1K || (ksteps == 18 && sel != DD_KSEL_AB)) && dd_fft1k_supported(K, M, flags))
        return DD_FAMILY_FFT1K;
    return open(DD_FAMILY_MFMA) ? DD_FAMILY_MFMA : DD_FAMILY_DENSE;
}

extern "C" int dd_debug_chain_select(const double* taps_host, int ntaps, int decim, int flags, int in_align_bytes, const char* selector_name,
                                     int* family) {
    DD_REQUIRE(taps_host && family && ntaps >= 1 && decim >= 1 && in_align_bytes >= 0, "arguments");
    const int sel = kernel_sel_parse(selector_name);
    DD_REQUIRE(sel >= 0, "selector_name (auto, ab, fft1k, cos1k, decimp)");
    *family = chain_select(taps_host, ntaps, decim, flags, (unsigned)in_align_bytes, sel, 0);
    return DD_OK;
}

// the lazily created state of an M = 1 family; nullptr when it has none or when its create failed (tried once)
static void* family_state(dd_fir* f, int family) {
    void** st = family == DD_FAMILY_COS1K ? &f->cos : family == DD_FAMILY_FFT1K ? &f->fft : family == DD_FAMILY_MFMA ? &f->mfma : nullptr;
    int* tried = family == DD_FAMILY_COS1K ? &f->cos_tried : family == DD_FAMILY_FFT1K ? &f->fft_tried : &f->mfma_tried;
    if (!st) return nullptr;
    if (!*st && !*tried) {
        *tried = 1;
        const int rc = family == DD_FAMILY_COS1K ? dd_cos1k_create(st, f->taps.data(), f->K)
                     : family == DD_FAMILY_FFT1K ? dd_fft_create(st, f->taps.data(), f->K) : dd_mfma_create(st, f->taps.data(), f->K);
        if (rc != DD_OK) *st = nullptr;
    }
    return *st;
}
// the family this filter's next launch takes (flags: DD_CHAIN_*; in: the input pointer, its low bits matter)
static int fir_select(const dd_fir* f, int M, int flags, const void* in) {
    const int skip = ((f->cos_tried && !f->cos) ? 1 << DD_FAMILY_COS1K : 0) | ((f->fft_tried && !f->fft) ? 1 << DD_FAMILY_FFT1K : 0) |
                     ((f->mfma_tried && !f->mfma) ? 1 << DD_FAMILY_MFMA : 0);
    return chain_select(f->taps.data(), f->K, M, flags, (unsigned)(reinterpret_cast<uintptr_t>(in) & 15), kernel_sel(), skip);
}

// ---------------------------------------------------------------- dd_fir (taps + history)
// ---- chunk-list launches: hand-overs that timed out (dd_seam_wait) become DD_ERR_TIMEOUT --------------------------------
static std::mutex g_seam_mu;
static std::vector<dd_fir*> g_seam_pending;          // filters that have made a chunk-list launch (their error word is looked at until they are destroyed)
static int g_seam_withhold = -1, g_seam_spin_log2 = 0;

extern "C" int dd_debug_seam(int withhold_chunk, int spin_log2) {
    std::lock_guard<std::mutex> lk(g_seam_mu);
    g_seam_withhold = withhold_chunk;
    g_seam_spin_log2 = spin_log2;
    return DD_OK;
}
// look at one filter's error word (dd_fir::seam_err_host); caller holds g_seam_mu.  A look while the launch still runs may be
// early; the word is final once its stream has been synchronised, and every later fused launch and dd_stream_sync looks again.
static int seam_look(dd_fir* f) {
    if (!f->seam_pending || !f->seam_err_host) return DD_OK;
    const unsigned n = *reinterpret_cast<volatile unsigned int*>(f->seam_err_host.get());
    if (n == 0) return DD_OK;
    f->state_invalid = 1;          // (the faulty launch also committed its carried state: nothing may continue from it)
    *reinterpret_cast<volatile unsigned int*>(f->seam_err_host.get()) = 0;
    dd_set_error("chunk-list launch: %u in-launch hand-over wait(s) of the carried FIR / FM state timed out; the outputs of that "
                 "dd_*_process_chunks call are invalid (run the chunks one by one, or raise the bound with dd_debug_seam)", n);
    return DD_ERR_TIMEOUT;
}
int dd_seam_poll_all(void) {
    std::lock_guard<std::mutex> lk(g_seam_mu);
    int rc = DD_OK;
    const std::vector<dd_fir*> firs = g_seam_pending;
    for (dd_fir* f : firs) {
        const int r = seam_look(f);
        if (r != DD_OK) rc = r;
    }
    return rc;
}
static void seam_forget(dd_fir* f) {
    std::lock_guard<std::mutex> lk(g_seam_mu);
    for (size_t i = 0; i < g_seam_pending.size(); ++i)
        if (g_seam_pending[i] == f) { g_seam_pending.erase(g_seam_pending.begin() + i); break; }
    if (f->seam_err_host) { (void)hipDeviceSynchronize(); f->seam_err_host.reset(); }      // (no launch may still count into it)
    f->seam_err = nullptr; f->seam_pending = 0;
}
// May a launch go on from this filter's carried state?  A chunk-list launch whose in-launch hand-over timed out is reported
// here (by every fused launch, not only by dd_stream_sync), and the state that launch committed is refused until the filter
// is reset -- also by a SECOND call, after the look has zeroed the word.  Only THIS filter's word decides: a timeout on
// another filter marks that filter, whose next call, or dd_stream_sync, reports it.  Caller holds g_seam_mu.
static int fir_usable(dd_fir* f) {
    const int rc = seam_look(f);
    if (rc != DD_OK) return rc;
    if (f->state_invalid) {
        dd_set_error("this filter's carried state comes from a chunk-list launch that timed out (DD_ERR_TIMEOUT was reported): reset it "
                     "(dd_fir_reset / dd_chain_reset / dd_chain_seek) before processing more samples");
        return DD_ERR_TIMEOUT;
    }
    return DD_OK;
}

extern "C" int dd_fir_create(dd_fir** h, const double* taps, int ntaps) {
    DD_REQUIRE(h && taps, "null argument");
    DD_REQUIRE(ntaps >= 1 && ntaps <= 8192, "ntaps must be in [1, 8192]");
    if (!dd_nco_table()) {
        dd_set_error("no usable GPU: the HIP path is mandatory (there is no CPU fallback)");
        return DD_ERR_NODEVICE;
    }
    dd_fir* f = new dd_fir();
    f->K = ntaps;
    f->taps.assign(taps, taps + ntaps);
    const int R = DD_DENSE_R;
    const int K = ntaps;
    // G[i] = g[i-(R-1)], g[j] = h[K-1-j]; zero padded so every R-block read is in range
    const int niter = (K + R - 1 + R - 1) / R;
    const int len = niter * R + 6 * R;                    // (k_chain_decim_w reads whole trips of 32 taps: zeros behind the last one)
    std::vector<float> g(len, 0.f);
    for (int j = 0; j < K; ++j) g[j + R - 1] = (float)taps[K - 1 - j];
    const int nc = K > 1 ? K - 1 : 1;
    hipError_t e = f->taps_rev.alloc(len);
    if (e == hipSuccess) e = hipMemcpy(f->taps_rev, g.data(), len * sizeof(float), hipMemcpyHostToDevice);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = (i < 2 ? f->tail[i] : f->tail_const[i - 2]).alloc(nc);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_fill_c64, dim3((nc + 255) / 256), dim3(256), 0, 0, f->tail_const[0].get(), nc, 0.f, 0.f);
        hipLaunchKernelGGL(k_fill_c64, dim3((nc + 255) / 256), dim3(256), 0, 0, f->tail_const[1].get(), nc, 1.f, 0.f);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        dd_fir_destroy(f);
        dd_set_error("dd_fir_create: %s", hipGetErrorString(e));
        return DD_ERR_HIP;
    }
    int rc = dd_fir_reset(f, DD_HIST_ONES, nullptr, nullptr);
    if (rc != DD_OK) {
        dd_fir_destroy(f);
        return rc;
    }
    DD_HIP_CHECK(hipDeviceSynchronize());
    *h = f;
    return DD_OK;
}

extern "C" int dd_fir_destroy(dd_fir* f) {
    if (!f) return DD_OK;
    if (f->mfma) dd_mfma_destroy(f->mfma);
    if (f->fft) dd_fft_destroy(f->fft);
    if (f->cos) dd_cos1k_destroy(f->cos);
    seam_forget(f);
    delete f;
    return DD_OK;
}

int dd_fir_reset_f64(dd_fir* f, int mode, const float* hist_host, hipStream_t s);   // dd_fir.hip

extern "C" int dd_fir_reset(dd_fir* f, int mode, const float* hist_host, void* stream) {
    DD_REQUIRE(f, "h");
    DD_REQUIRE(mode == DD_HIST_ZEROS || mode == DD_HIST_ONES || mode == DD_HIST_GIVEN, "mode");
    hipStream_t s = dd_stream(stream);
    const int n = f->K - 1;
    if (n > 0) {
        if (mode == DD_HIST_GIVEN) {
            DD_REQUIRE(hist_host, "hist_host");
            DD_HIP_CHECK(hipMemcpyAsync(f->tail[f->parity], hist_host, sizeof(float2) * n, hipMemcpyHostToDevice, s));
            DD_HIP_CHECK(hipStreamSynchronize(s));
            f->tail_override = nullptr;
        } else {
            // DD_HIST_ONES: lfilter_zi(b,[1]) unscaled == history of 1.0+0j (filters.py:45, quirk Q1).
            // No launch: the next kernel simply reads the constant history buffer.
            f->tail_override = f->tail_const[mode == DD_HIST_ONES ? 1 : 0];
        }
    }
    f->hist_mode = mode;
    f->state_invalid = 0;
    f->launches = 0;
    return dd_fir_reset_f64(f, mode, hist_host, s);
}

// ---------------------------------------------------------------- dd_fm
extern "C" int dd_fm_create(dd_fm** h) {
    DD_REQUIRE(h, "h");
    dd_fm* f = new dd_fm();
    hipError_t e = f->last.alloc(2);
    if (e == hipSuccess) e = hipMemset(f->last, 0, 2 * sizeof(float2));
    if (e != hipSuccess) {
        delete f;
        dd_set_error("dd_fm_create: %s", hipGetErrorString(e));
        return (e == hipErrorNoDevice) ? DD_ERR_NODEVICE : DD_ERR_HIP;
    }
    *h = f;
    return DD_OK;
}
extern "C" int dd_fm_destroy(dd_fm* h) {
    delete h;
    return DD_OK;
}
extern "C" int dd_fm_reset(dd_fm* h) {
    DD_REQUIRE(h, "h");
    h->has_last = 0;
    return DD_OK;
}

// ---------------------------------------------------------------- fused launch
static inline int64_t kept_count(int64_t L, int off, int M) {
    return (L > off) ? (L - off + M - 1) / M : 0;
}
// the decimation phase the chunk after a chunk of n samples with phase off starts with: kept global indices are the
// multiples of M (nextOff of comm.py:123-127, quirk Q4)
static inline int next_off(int64_t n, int off, int M) {
    return (int)((M - (n - off) % M) % M);
}
static inline size_t in_elem_size(int flags) { return (flags & DD_CHAIN_U8_INPUT) ? 2 : sizeof(float2); }
static inline size_t out_elem_size(const dd_fm* fm) { return fm ? sizeof(float) : sizeof(float2); }

int64_t dd_fused_out_count(const dd_fm* fm, int64_t n, int M, int off) {
    const int64_t Ld = kept_count(n, off, M);
    if (!fm) return Ld;
    const int64_t no = Ld - (fm->has_last ? 0 : 1);
    return no > 0 ? no : 0;
}

// one chunk's arguments, from what the entry points are given (flags: DD_CHAIN_U8_INPUT | DD_CHAIN_FORCE_DIRECT | DD_CHAIN_TIGHT)
static DDFusedArgs fused_args(const void* in, void* out, int64_t n, int nco, uint64_t cyc, int64_t start_index, int M, int off, int flags, int commit) {
    DDFusedArgs a;
    a.in = in;
    a.out = out;
    a.n = n;
    a.cyc = cyc;
    a.start_index = start_index;
    a.M = M;
    a.off = off;
    a.flags = (nco ? DD_CHAIN_NCO : 0) | (flags & (DD_CHAIN_U8_INPUT | DD_CHAIN_FORCE_DIRECT | DD_CHAIN_TIGHT));
    a.commit = commit;
    return a;
}

// the kernels' parameter block for one chunk that reads and writes the handles' own state; has_last: whether an FM sample
// precedes the chunk (fm->has_last, or 1 behind an earlier chunk of the same chunk list).  T / nblocks: by the family's plan.
static DDChainParams chain_params(const dd_fir* fir, const dd_fm* fm, const DDFusedArgs& a, int has_last) {
    DDChainParams P;
    memset(&P, 0, sizeof(P));
    P.in = a.in;
    P.out = a.out;
    P.tail_in = fir->tail_override ? fir->tail_override : fir->tail[fir->parity];
    P.tail_out = a.commit ? fir->tail[fir->parity ^ 1] : nullptr;
    P.taps_rev = fir->taps_rev;
    P.nco_tbl = dd_nco_table();
    P.cyc = a.cyc;
    P.abs0 = a.start_index;
    P.L = a.n;
    P.K = fir->K;
    P.M = a.M;
    P.off = a.off;
    P.Ld = kept_count(a.n, a.off, a.M);
    P.flags = (a.flags & (DD_CHAIN_NCO | DD_CHAIN_U8_INPUT | DD_CHAIN_TIGHT)) | (fm ? DD_CHAIN_FM : 0);
    P.s = (fm && !has_last) ? 1 : 0;
    if (fm) {
        P.lasty_in = fm->last + fm->parity;
        P.lasty_out = fm->last + (fm->parity ^ 1);
    }
    return P;
}

// tiles of T FIR outputs over a chunk's kept samples (an FM tile recomputes the output before its first one)
static int tile_count(int64_t Ld, int s, bool isfm, int T) {
    const int nblocks = isfm ? (int)((Ld - s + (T - 2)) / (T - 1)) : (int)((Ld + T - 1) / T);
    return nblocks < 1 ? 1 : nblocks;
}
static void tile_grid(DDChainParams& P, int T) {
    P.T = T;
    P.nblocks = tile_count(P.Ld, P.s, (P.flags & DD_CHAIN_FM) != 0, T);
}

static int launch_dense(DDChainParams& P, hipStream_t s, int* kernel_id) {
    tile_grid(P, DD_DENSE_T);
    const int R = DD_DENSE_R;
    const int niter = (P.K + R - 1 + R - 1) / R;
    const int S = P.T + niter * R;
    const int SP = S + (S >> 3) + 8;
    const size_t lds = (size_t)SP * 2 * sizeof(float) + sizeof(float2) * ((S + 63) / 64 + 1) +
                       sizeof(float2) * DD_DENSE_THREADS;
    DD_REQUIRE(lds <= 160 * 1024, "filter too long for the dense kernel's LDS tile");
    if (lds > 64 * 1024)
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_chain_dense, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_chain_dense, dim3(P.nblocks), dim3(DD_DENSE_THREADS), lds, s, P);
    DD_LAUNCH_CHECK();
    *kernel_id = DD_KERNEL_DENSE_F32;
    return DD_OK;
}

// the dynamic-LDS limit of the persistent and chunk-list tile kernels (once per device)
static int raise_decim_lds_limit() {
    static DDOncePerDevice attr;
    if (attr.need()) {
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_chain_decim_p<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_chain_decim_p<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_chain_decim_multi<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_chain_decim_multi<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr.mark();
    }
    return DD_OK;
}

// geometry of one chunk through the tile kernels (M > 1): tile size, tile count, spans, LDS, and -- when the chunk has an
// interior run worth a persistent grid -- that run [lo, hi).  Host arithmetic only (dd_debug_decim_tile_plan hands it out):
//   T          FIR outputs per tile (an FM tile recomputes the output before its first one); S the samples a tile stages,
//              S2 that span rounded up to whole load granules (sample pairs for complex64, octets for raw u8)
//   [lo, hi)   the interior tiles: span S2 inside the chunk, all T outputs valid, not the chunk's last tile (that one
//              writes the carried state), input on a load granule -- the tiles whose loads are unconditional
//   lds, lds_p dynamic LDS of the edge kernel / of a launch with persistent workgroups
struct DDDecimGeom {
    int T, nblocks, S, S2, lo, hi;
    bool persistent;
    size_t lds, lds_p;
};
static int decim_geometry(int64_t L, int K, int M, int off, bool isfm, int s, bool u8in, unsigned in_align, DDDecimGeom& g) {
    int T = (DD_DECIM_SPAN_MAX - K - (M - 1)) / M + 1;
    if (T > DD_DECIM_THREADS) T = DD_DECIM_THREADS;
    if (T < 2) T = 2;
    const int64_t Ld = kept_count(L, off, M);
    g.T = T;
    g.nblocks = tile_count(Ld, s, isfm, T);
    const int64_t S64 = (int64_t)(T - 1) * M + K + (M - 1);
    const int64_t SP = S64 + 4;
    const int64_t lds64 = (int64_t)sizeof(float2) * (SP + (S64 + 63) / 64 + 1 + DD_DECIM_THREADS) + (int64_t)sizeof(float) * ((K + 7) & ~7) + 16;
    DD_REQUIRE(lds64 <= 160 * 1024, "filter/decimation too large for the decimating kernel's LDS tile");
    const int S = (int)S64;
    const size_t lds = (size_t)lds64;
    g.S = S;
    g.S2 = u8in ? ((S + 7) & ~7) : ((S + 1) & ~1);
    g.lds = lds;
    g.lds_p = lds;
    g.persistent = false;
    g.lo = g.hi = g.nblocks;
    const int S2 = g.S2;
    if (S2 <= DD_DECIM_SPAN_MAX && (in_align & (u8in ? 3 : 7)) == 0) {
        const int64_t adv = isfm ? (T - 1) : T;                      // outputs a tile advances by
        const int64_t pf0 = isfm ? (int64_t)s - 1 : 0;               // pfirst of tile 0
        // ns(b) = off + (pf0 + b adv) M - (K-1) >= 0 ;  ns(b) + S2 <= L ;  pf0 + b adv >= 0 ;  pf0 + b adv + T <= Ld
        int64_t lo = 0;
        while (lo < g.nblocks && ((int64_t)off + (pf0 + lo * adv) * M - (K - 1) < 0 || pf0 + lo * adv < 0)) ++lo;
        int64_t hi = g.nblocks - 1;                                  // exclusive bound candidates, walk down
        while (hi > lo && ((int64_t)off + (pf0 + (hi - 1) * adv) * M - (K - 1) + S2 > L || pf0 + (hi - 1) * adv + T > Ld)) --hi;
        if (hi - lo >= 64) {
            g.lo = (int)lo;
            g.hi = (int)hi;
            g.persistent = true;
            const size_t lds_p0 = sizeof(float2) * ((size_t)S2 + 4 + S2 / 64 + 2 + DD_DECIM_THREADS) + sizeof(float) * ((K + 7) & ~7) + 16;
            g.lds_p = lds_p0 > lds ? lds_p0 : lds;                   // the edge workgroups of the same launch need `lds`
        }
    }
    return DD_OK;
}

extern "C" int dd_debug_decim_tile_plan(int64_t L, int K, int M, int off, int fm, int has_last, int u8, int in_align_bytes, int64_t* out) {
    DD_REQUIRE(out && L >= 0 && K >= 1 && M >= 2 && off >= 0 && off < M && in_align_bytes >= 0, "arguments");
    DDDecimGeom g;
    const int rc = decim_geometry(L, K, M, off, fm != 0, (fm && !has_last) ? 1 : 0, u8 != 0, (unsigned)in_align_bytes, g);
    if (rc != DD_OK) return rc;
    out[0] = g.T; out[1] = g.nblocks; out[2] = g.S; out[3] = g.S2; out[4] = g.persistent ? 1 : 0; out[5] = g.lo; out[6] = g.hi;
    out[7] = (int64_t)g.lds; out[8] = (int64_t)g.lds_p;
    return DD_OK;
}

// one chunk's plan: its geometry into the parameter block (P.T, P.nblocks, P.skip_lo / skip_hi), and what the device has to
// be told and asked for it -- the dynamic-LDS limits, and how many persistent workgroups a CU holds
struct DDDecimPlan {
    size_t lds, lds_p;
    bool persistent;
    int lo, hi, per_cu;
};
static int decim_plan(DDChainParams& P, DDDecimPlan& pl) {
    const bool u8in = (P.flags & DD_CHAIN_U8_INPUT) != 0;
    DDDecimGeom g;
    const int rc0 = decim_geometry(P.L, P.K, P.M, P.off, (P.flags & DD_CHAIN_FM) != 0, P.s, u8in,
                                   (unsigned)(reinterpret_cast<uintptr_t>(P.in) & 15), g);
    if (rc0 != DD_OK) return rc0;
    P.T = g.T;
    P.nblocks = g.nblocks;
    P.skip_lo = g.lo;
    P.skip_hi = g.hi;
    pl.lds = g.lds;
    pl.lds_p = g.lds_p;
    pl.persistent = g.persistent;
    pl.lo = g.lo;
    pl.hi = g.hi;
    pl.per_cu = 1;
    if (g.lds > 64 * 1024)
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_chain_decim, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
    if (g.persistent) {
        const int rc = raise_decim_lds_limit();
        if (rc != DD_OK) return rc;
        // every workgroup must be resident from the start (a persistent grid with queued workgroups
        // runs in rounds): ask the runtime how many fit (LDS and registers)
        static std::mutex occ_mu;
        static size_t occ_lds[2] = {0, 0};          // the answer depends on (flavour, LDS size) only: asked once per change
        static int occ_val[2] = {0, 0};
        std::lock_guard<std::mutex> lk(occ_mu);
        int per_cu = occ_val[u8in];
        if (occ_lds[u8in] != pl.lds_p || per_cu < 1) {
            if ((u8in ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_chain_decim_p<true>, DD_DECIM_THREADS, pl.lds_p)
                      : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_chain_decim_p<false>, DD_DECIM_THREADS, pl.lds_p)) != hipSuccess || per_cu < 1) per_cu = 1;
            occ_lds[u8in] = pl.lds_p;
            occ_val[u8in] = per_cu;
        }
        pl.per_cu = per_cu;
    }
    return DD_OK;
}

// persistent workgroups for n_interior tiles beside n_edge trailing workgroups (one edge tile each), all resident at once:
// the persistent grid leaves the edge tiles their slots
static int persistent_grid(int n_interior, int n_edge, int per_cu) {
    const int slots = dd_cu_count() * per_cu;
    int grid = n_edge < slots / 2 ? slots - n_edge : slots / 2;
    if (grid > n_interior) grid = n_interior;
    if (grid >= 8) grid &= ~7;
    return grid < 0 ? 0 : grid;
}

static int launch_tiles(DDChainParams& P, hipStream_t s, int* kernel_id) {
    DDDecimPlan pl;
    int rc = decim_plan(P, pl);
    if (rc != DD_OK) return rc;
    if (pl.persistent) {
        // the tiles around the interior run ride along as trailing workgroups of the same launch
        const int n_rest = P.nblocks - (pl.hi - pl.lo);
        const int grid = persistent_grid(pl.hi - pl.lo, n_rest, pl.per_cu);
        if (P.flags & DD_CHAIN_U8_INPUT) hipLaunchKernelGGL(k_chain_decim_p<true>, dim3(grid + n_rest), dim3(DD_DECIM_THREADS), pl.lds_p, s, P, pl.lo, pl.hi, grid);
        else hipLaunchKernelGGL(k_chain_decim_p<false>, dim3(grid + n_rest), dim3(DD_DECIM_THREADS), pl.lds_p, s, P, pl.lo, pl.hi, grid);
        DD_LAUNCH_CHECK();
        *kernel_id = DD_KERNEL_DECIM_PERSISTENT;
    } else {
        // no interior run (short chunk, unaligned input): every tile through the stand-alone edge kernel
        hipLaunchKernelGGL(k_chain_decim, dim3(P.nblocks), dim3(DD_DECIM_THREADS), pl.lds, s, P);
        DD_LAUNCH_CHECK();
        *kernel_id = DD_KERNEL_DECIM_TILES;
    }
    return DD_OK;
}

int dd_fused_launch(dd_fir* fir, dd_fm* fm, const DDFusedArgs& a, int64_t* n_out, hipStream_t s) {
    DD_REQUIRE(fir && a.n >= 0 && a.M >= 1 && a.off >= 0 && a.off < a.M, "fused arguments");
    int rc;
    {
        std::lock_guard<std::mutex> lk(g_seam_mu);
        rc = fir_usable(fir);
    }
    if (rc != DD_OK) return rc;
    DDChainParams P = chain_params(fir, fm, a, fm ? fm->has_last : 0);
    const int64_t no = dd_fused_out_count(fm, a.n, a.M, a.off);
    if (n_out) *n_out = no;
    fir->last_kernel = DD_KERNEL_NONE;
    if (a.n == 0) return DD_OK;
    DD_REQUIRE(a.in, "in");
    DD_REQUIRE(a.out || no == 0, "out");

    const float* taps_g0 = fir->taps_rev + (DD_DENSE_R - 1);
    if (P.Ld == 0) {
        // no kept sample in this chunk: only the FIR history moves on
        if (a.commit && fir->K > 1) {
            if (fir_select(fir, a.M, a.flags, a.in) == DD_FAMILY_ROWS) {
                // (the row kernels' history is THEIR value of a sample after the NCO: the same arithmetic for a chunk without a kept sample)
                rc = dd_decimw_launch(P, taps_g0, fir->taps.data(), &fir->dw_taps, s);
                if (rc != DD_OK) return rc;
            } else {
                hipLaunchKernelGGL(k_tail_update, dim3(1), dim3(256), 0, s, P);
            }
            DD_LAUNCH_CHECK();
            fir->parity ^= 1;
            fir->tail_override = nullptr;
        }
        return DD_OK;
    }

    // a family whose state cannot be created falls through to the next one (family_state marks it, fir_select skips it)
    int family = fir_select(fir, a.M, a.flags, a.in);
    void* st = family_state(fir, family);
    while (!st && (family == DD_FAMILY_COS1K || family == DD_FAMILY_FFT1K || family == DD_FAMILY_MFMA)) {
        family = fir_select(fir, a.M, a.flags, a.in);
        st = family_state(fir, family);
    }
    int kid = DD_KERNEL_NONE;
    switch (family) {
        case DD_FAMILY_COS1K: rc = dd_cos1k_launch(st, P, s); kid = DD_KERNEL_COS_RS; break;
        case DD_FAMILY_FFT1K: rc = dd_fft1k_launch(st, P, s); kid = DD_KERNEL_FFT_OS; break;
        case DD_FAMILY_MFMA: rc = dd_mfma_launch(st, P, s, &kid); break;
        case DD_FAMILY_ROWS: kid = DD_KERNEL_DECIM_WAVE; rc = dd_decimw_launch(P, taps_g0, fir->taps.data(), &fir->dw_taps, s, &kid); break;
        case DD_FAMILY_TILES: rc = launch_tiles(P, s, &kid); break;
        default: rc = launch_dense(P, s, &kid); break;
    }
    if (rc != DD_OK) return rc;
    fir->last_kernel = kid;
    ++fir->launches;
    if (a.commit) {
        fir->parity ^= 1;
        fir->tail_override = nullptr;
    }
    if (fm) {
        fm->parity ^= 1;
        fm->has_last = 1;
    }
    return DD_OK;
}

extern "C" int dd_fused_process(dd_fir* fir, dd_fm* fm, const void* in, void* out, int64_t n,
                                int nco, uint64_t cycles_q64, int64_t start_index, int decim, int offset,
                                int flags, int carry, int64_t* n_out, void* stream) {
    DD_REQUIRE(fir, "fir");
    return dd_fused_launch(fir, fm, fused_args(in, out, n, nco, cycles_q64, start_index, decim, offset, flags, carry), n_out, dd_stream(stream));
}

// ---------------------------------------------------------------- stand-alone rows
extern "C" int dd_fir_c64(dd_fir* f, const float* in_c64, float* out_c64, int64_t n, int carry, void* stream) {
    DD_REQUIRE(f && n >= 0, "h/n");
    return dd_fused_launch(f, nullptr, fused_args(in_c64, out_c64, n, 0, 0, 0, 1, 0, 0, carry), nullptr, dd_stream(stream));
}

extern "C" int dd_fm_discrim_c64(dd_fm* h, const float* in_c64, float* out, int64_t n, int carry,
                                 int64_t* n_out, void* stream) {
    DD_REQUIRE(h && n >= 0, "h/n");
    // demod_fm.py:44/48 index sig[-1]: an empty chunk is an IndexError in the reference
    DD_REQUIRE(!(carry && n == 0), "empty chunk with storeState (IndexError in the reference)");
    const int s = (carry && h->has_last) ? 0 : 1;
    const int64_t no = n - s > 0 ? n - s : 0;
    if (n_out) *n_out = no;
    if (n == 0) return DD_OK;
    DD_REQUIRE(in_c64 && (out || no == 0), "null buffer");
    int64_t g = (no + 255) / 256;
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(k_fm, dim3((unsigned)g), dim3(256), 0, dd_stream(stream), (const float2*)in_c64, out, no, s,
                       h->last + h->parity, carry ? h->last + (h->parity ^ 1) : (float2*)nullptr, n);
    DD_LAUNCH_CHECK();
    if (carry) {
        h->parity ^= 1;
        h->has_last = 1;
    }
    return DD_OK;
}

// ---------------------------------------------------------------- chunk lists
// The chunks [bounds[i], bounds[i+1]) of `in` through (fir, fm) exactly as the per-chunk loop would take them -- chunk i
// starts at absolute index start_index + (bounds[i] - bounds[0]) with the decimation phase the previous chunk left
// (comm.py:123-125) -- in ONE launch when the chain decimates (M > 1) and every chunk keeps at least one sample.
// Returns 1 when it has done so (state committed), 0 when the caller must loop, < 0 on error.
static int fused_chunks_one_launch(dd_fir* fir, dd_fm* fm, const void* in, void* out, const int64_t* bounds_host, int nchunks,
                                   int nco, uint64_t cyc, int64_t start_index, int M, int off0, int flags, int64_t* n_out_host, hipStream_t s) {
    const bool isfm = fm != nullptr;
    const bool u8 = (flags & DD_CHAIN_U8_INPUT) != 0;
    if (!(M > 1 && nchunks >= 2 && !(flags & DD_CHAIN_FORCE_DIRECT) && fir->K >= 2)) return 0;
    flags &= DD_CHAIN_U8_INPUT;
    if (fir_select(fir, M, flags, in) == DD_FAMILY_ROWS) {
        // the row kernels lay their rows on the ABSOLUTE decimation grid, which a chunk list continues from chunk to chunk (comm.py:123-125),
        // and a sample after the NCO is a pure function of its absolute index: the list is ONE chunk -- same outputs as the loop, bit for
        // bit, no hand-over inside the launch
        int has_last = isfm ? fm->has_last : 0, off = off0;
        for (int i = 0; i < nchunks; ++i) {
            const int64_t ni = bounds_host[i + 1] - bounds_host[i];
            const int64_t Ld = kept_count(ni, off, M);
            if (ni == 0 || Ld == 0) return 0;
            if (n_out_host) n_out_host[i] = isfm ? Ld - (has_last ? 0 : 1) : Ld;
            off = next_off(ni, off, M);
            if (isfm) has_last = 1;
        }
        const DDFusedArgs a = fused_args(in, out, bounds_host[nchunks] - bounds_host[0], nco, cyc, start_index, M, off0, flags, 1);
        const int rc = dd_fused_launch(fir, fm, a, nullptr, s);
        return rc == DD_OK ? 1 : rc;
    }
    int withhold = -1, spin_log2 = 0;
    {
        // an earlier chunk-list launch through this filter whose hand-over timed out: say so now, before anything is enqueued
        std::lock_guard<std::mutex> lk(g_seam_mu);
        const int rc0 = fir_usable(fir);
        if (rc0 != DD_OK) return rc0;
        withhold = g_seam_withhold;
        g_seam_withhold = -1;                  // (one launch)
        spin_log2 = g_seam_spin_log2;
    }
    if (!fir->seam_err) {
        DDPinnedBuf<unsigned int> words;
        unsigned int* dev = nullptr;
        DD_HIP_CHECK(words.alloc(2, hipHostMallocMapped));
        words[0] = words[1] = 0;
        DD_HIP_CHECK(hipHostGetDevicePointer((void**)&dev, words, 0));
        fir->seam_err_host = std::move(words);
        fir->seam_err = dev;
    }
    {
        // (a chunk list whose chunks have no interior run never passes through decim_plan's persistent branch)
        const int rc0 = raise_decim_lds_limit();
        if (rc0 != DD_OK) return rc0;
    }
    std::vector<DDChainParams> Pv;
    std::vector<DDDecimPlan> plv;
    std::vector<int64_t> nout(nchunks, 0);
    int64_t abs_index = start_index, opos = 0;
    int has_last = isfm ? fm->has_last : 0, off = off0;
    for (int i = 0; i < nchunks; ++i) {
        const int64_t n = bounds_host[i + 1] - bounds_host[i];
        const DDFusedArgs a = fused_args(reinterpret_cast<const char*>(in) + in_elem_size(flags) * (size_t)(bounds_host[i] - bounds_host[0]),
                                         reinterpret_cast<char*>(out) + out_elem_size(fm) * (size_t)opos, n, nco, cyc, abs_index, M, off, flags, 1);
        DDChainParams P = chain_params(fir, fm, a, has_last);      // (tail / last-sample pointers: set below, once the seam buffers exist)
        if (n == 0 || P.Ld == 0) return 0;
        DDDecimPlan pl;
        int rc = decim_plan(P, pl);
        if (rc != DD_OK) return rc;
        nout[i] = isfm ? P.Ld - P.s : P.Ld;
        if (nout[i] < 0) nout[i] = 0;
        Pv.push_back(P);
        plv.push_back(pl);
        opos += nout[i];
        abs_index += n;
        off = next_off(n, off, M);
        if (isfm) has_last = 1;
    }
    // device image: [flags, 16-byte padded][parameter blocks][segments][interior prefix][edge prefix][seam tails][seam last samples]
    const int K1 = fir->K - 1;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_par = al(sizeof(unsigned int) * nchunks), o_seg = o_par + al(sizeof(DDChainParams) * nchunks);
    const size_t o_ipre = o_seg + al(sizeof(DDSeg) * nchunks), o_epre = o_ipre + al(sizeof(int) * (nchunks + 1));
    const size_t o_tail = o_epre + al(sizeof(int) * (nchunks + 1)), o_last = o_tail + al(sizeof(float2) * (size_t)K1 * nchunks);
    const size_t total = o_last + al(sizeof(float2) * nchunks);
    if (total > fir->multi.bytes()) {
        DD_HIP_CHECK(hipStreamSynchronize(s));
        DD_HIP_CHECK(fir->multi.alloc(total));
    }
    char* const multi = fir->multi;
    unsigned int* seam_flags = reinterpret_cast<unsigned int*>(multi);
    float2* seam_tail = reinterpret_cast<float2*>(multi + o_tail);
    float2* seam_last = reinterpret_cast<float2*>(multi + o_last);
    std::vector<char> img(o_tail, 0);                         // (from the seam flags, which start as zeros, to the edge prefix: ONE copy)
    DDChainParams* hP = reinterpret_cast<DDChainParams*>(img.data() + o_par);
    DDSeg* hS = reinterpret_cast<DDSeg*>(img.data() + o_seg);
    int* hI = reinterpret_cast<int*>(img.data() + o_ipre);
    int* hE = reinterpret_cast<int*>(img.data() + o_epre);
    hI[0] = hE[0] = 0;
    size_t lds_p = 0;
    int per_cu = 0;
    for (int i = 0; i < nchunks; ++i) {
        DDChainParams& P = Pv[i];
        if (i > 0) P.tail_in = seam_tail + (size_t)K1 * (i - 1);
        if (i < nchunks - 1) P.tail_out = seam_tail + (size_t)K1 * i;
        if (isfm) {
            if (i > 0) P.lasty_in = seam_last + (i - 1);
            if (i < nchunks - 1) P.lasty_out = seam_last + i;
        }
        P.seam_wait = i > 0 ? seam_flags + (i - 1) : nullptr;
        P.seam_post = i < nchunks - 1 ? seam_flags + i : nullptr;
        if (P.seam_post && i == withhold) P.seam_post = fir->seam_err + 1;       // (dd_debug_seam: this chunk's flag is never set)
        P.seam_err = fir->seam_err;
        P.seam_spin_log2 = spin_log2;
        hP[i] = P;
        hS[i].in = P.in; hS[i].out = P.out; hS[i].abs0 = P.abs0; hS[i].off = P.off; hS[i].s = P.s; hS[i].lo = plv[i].lo; hS[i].pad = 0;
        hI[i + 1] = hI[i] + (plv[i].hi - plv[i].lo);
        hE[i + 1] = hE[i] + (P.nblocks - (plv[i].hi - plv[i].lo));
        if (plv[i].lds_p > lds_p) lds_p = plv[i].lds_p;
        if (plv[i].persistent && (per_cu == 0 || plv[i].per_cu < per_cu)) per_cu = plv[i].per_cu;
    }
    const int n_int = hI[nchunks], n_edge = hE[nchunks];
    if (per_cu < 1) per_cu = 1;
    DD_HIP_CHECK(hipMemcpyAsync(multi, img.data(), img.size(), hipMemcpyHostToDevice, s));      // (pageable source: staged before the call returns)
    const int grid = persistent_grid(n_int, n_edge, per_cu);
    const DDChainParams* dP = reinterpret_cast<const DDChainParams*>(multi + o_par);
    const DDSeg* dS = reinterpret_cast<const DDSeg*>(multi + o_seg);
    const int* dI = reinterpret_cast<const int*>(multi + o_ipre);
    const int* dE = reinterpret_cast<const int*>(multi + o_epre);
    if (u8) hipLaunchKernelGGL(k_chain_decim_multi<true>, dim3(grid + n_edge), dim3(DD_DECIM_THREADS), lds_p, s, dP, dS, dI, dE, nchunks, grid);
    else hipLaunchKernelGGL(k_chain_decim_multi<false>, dim3(grid + n_edge), dim3(DD_DECIM_THREADS), lds_p, s, dP, dS, dI, dE, nchunks, grid);
    DD_LAUNCH_CHECK();
    {
        // the kernel counts waits that gave up into fir->seam_err_host; every later fused launch and dd_stream_sync looks at it
        std::lock_guard<std::mutex> lk(g_seam_mu);
        if (!fir->seam_pending) g_seam_pending.push_back(fir);
        fir->seam_pending = 1;
    }
    fir->last_kernel = DD_KERNEL_DECIM_MULTI;
    ++fir->launches;
    fir->parity ^= 1;
    fir->tail_override = nullptr;
    if (isfm) {
        fm->parity ^= 1;
        fm->has_last = 1;
    }
    if (n_out_host) for (int i = 0; i < nchunks; ++i) n_out_host[i] = nout[i];
    return 1;
}

// A chunk list through (fir, fm): `in` points at the first chunk's first sample, start_index / off are the chunker variables
// of the FIRST chunk, the later chunks' follow by the reference's own carry rules (comm.py:75-76, 123-125).  One launch where
// fused_chunks_one_launch takes the list, else the chunk loop.  *consumed: the samples of the chunks that went through.
static int fused_chunks(dd_fir* fir, dd_fm* fm, const void* in, void* out, const int64_t* bounds_host, int nchunks, int nco, uint64_t cyc,
                        int64_t start_index, int M, int off, int flags, int64_t* n_out_host, int64_t* consumed, hipStream_t s) {
    *consumed = 0;
    for (int i = 0; i < nchunks; ++i) DD_REQUIRE(bounds_host[i + 1] >= bounds_host[i], "bounds must ascend");
    if (nchunks == 0) return DD_OK;
    int rc = fused_chunks_one_launch(fir, fm, in, out, bounds_host, nchunks, nco, cyc, start_index, M, off, flags, n_out_host, s);
    if (rc != 0) {
        if (rc == 1) *consumed = bounds_host[nchunks] - bounds_host[0];
        return rc < 0 ? rc : DD_OK;
    }
    int64_t opos = 0;
    for (int i = 0; i < nchunks; ++i) {
        const int64_t n = bounds_host[i + 1] - bounds_host[i];
        int64_t got = 0;
        const DDFusedArgs a = fused_args(reinterpret_cast<const char*>(in) + in_elem_size(flags) * (size_t)(bounds_host[i] - bounds_host[0]),
                                         reinterpret_cast<char*>(out) + out_elem_size(fm) * (size_t)opos, n, nco, cyc, start_index + *consumed, M, off, flags, 1);
        rc = dd_fused_launch(fir, fm, a, &got, s);
        if (rc != DD_OK) return rc;
        if (n_out_host) n_out_host[i] = got;
        opos += got;
        *consumed += n;
        off = next_off(n, off, M);
    }
    return DD_OK;
}

// The object-model form (dd_fused_process): carry is 1 (storeState).
extern "C" int dd_fused_process_chunks(dd_fir* fir, dd_fm* fm, const void* in, void* out, const int64_t* bounds_host, int nchunks,
                                       int nco, uint64_t cycles_q64, int64_t start_index, int decim, int offset, int flags,
                                       int64_t* n_out_host, void* stream) {
    DD_REQUIRE(fir && bounds_host && nchunks >= 0 && decim >= 1 && offset >= 0 && offset < decim, "arguments");
    int64_t consumed = 0;
    return fused_chunks(fir, fm, in, out, bounds_host, nchunks, nco, cycles_q64, start_index, decim, offset, flags, n_out_host, &consumed, dd_stream(stream));
}

// ---------------------------------------------------------------- dd_chain convenience handle
// Bundles a filter, an FM demodulator and the chunker variables of one stream
// (NCO sample index "freqoffset", decimation phase "bwlim", constants.py:38-39).
struct dd_chain {
    dd_fir* fir = nullptr;
    dd_fm* fm = nullptr;
    uint64_t cyc = 0;
    int M = 1, flags = 0;
    int64_t abs_index = 0;
    DDDevBuf<char> scratch;     // discarded outputs of dd_chain_prime (grow-only)
};

extern "C" int dd_chain_create(dd_chain** h, const double* taps, int ntaps, uint64_t cycles_q64,
                               int decim, int flags) {
    DD_REQUIRE(h && taps, "null argument");
    DD_REQUIRE(decim >= 1, "decim must be >= 1");
    dd_chain* c = new dd_chain();
    c->cyc = cycles_q64;
    c->M = decim;
    c->flags = flags;
    int rc = dd_fir_create(&c->fir, taps, ntaps);
    if (rc == DD_OK && (flags & DD_CHAIN_FM)) rc = dd_fm_create(&c->fm);
    if (rc != DD_OK) {
        dd_chain_destroy(c);
        return rc;
    }
    *h = c;
    return DD_OK;
}

extern "C" int dd_chain_destroy(dd_chain* c) {
    if (!c) return DD_OK;
    dd_fir_destroy(c->fir);
    dd_fm_destroy(c->fm);
    delete c;
    return DD_OK;
}

extern "C" int dd_chain_reset(dd_chain* c, void* stream) {
    DD_REQUIRE(c, "h");
    c->abs_index = 0;
    if (c->fm) dd_fm_reset(c->fm);
    return dd_fir_reset(c->fir, DD_HIST_ONES, nullptr, stream);
}

// the decimation phase at the handle's position: what next_off has carried from index 0
static inline int chain_off(const dd_chain* c) {
    return next_off(c->abs_index, 0, c->M);
}

extern "C" int64_t dd_chain_out_count(const dd_chain* c, int64_t n) {
    if (!c || n < 0) return -1;
    return dd_fused_out_count(c->fm, n, c->M, chain_off(c));
}

// 1: the chain's next launch takes one of the M = 1 matrix / transform / running-sum kernels, 0: a direct-form kernel
extern "C" int dd_chain_path(const dd_chain* c) {
    if (!c) return DD_ERR_INVALID;
    const int family = fir_select(c->fir, c->M, c->flags, nullptr);
    return (family == DD_FAMILY_COS1K || family == DD_FAMILY_FFT1K || family == DD_FAMILY_MFMA) ? 1 : 0;
}

extern "C" int dd_fir_last_kernel(const dd_fir* f) {
    if (!f) return DD_ERR_INVALID;
    return f->last_kernel;
}

extern "C" long long dd_fir_launch_count(const dd_fir* f) {
    return f ? f->launches : -1;
}

extern "C" int dd_chain_last_kernel(const dd_chain* c) {
    if (!c) return DD_ERR_INVALID;
    return c->fir->last_kernel;
}

extern "C" int dd_chain_process(dd_chain* c, const void* in, void* out, int64_t n, int64_t* n_out, void* stream) {
    DD_REQUIRE(c && n >= 0, "h/n");
    const DDFusedArgs a = fused_args(in, out, n, c->flags & DD_CHAIN_NCO, c->cyc, c->abs_index, c->M, chain_off(c), c->flags, 1);
    int rc = dd_fused_launch(c->fir, c->fm, a, n_out, dd_stream(stream));
    if (rc == DD_OK) c->abs_index += n;
    return rc;
}

// The chunks [bounds[i], bounds[i+1]) of `in` (sample offsets, ascending, nchunks + 1 of them) as dd_chain_process would
// take them one after the other -- same outputs, bit for bit, concatenated at `out`, same state afterwards.
extern "C" int dd_chain_process_chunks(dd_chain* c, const void* in, void* out, const int64_t* bounds_host, int nchunks,
                                       int64_t* n_out_host, void* stream) {
    DD_REQUIRE(c && bounds_host && nchunks >= 0, "arguments");
    const char* in0 = reinterpret_cast<const char*>(in) + (nchunks > 0 ? in_elem_size(c->flags) * (size_t)bounds_host[0] : 0);
    int64_t consumed = 0;
    const int rc = fused_chunks(c->fir, c->fm, in0, out, bounds_host, nchunks, c->flags & DD_CHAIN_NCO, c->cyc, c->abs_index, c->M, chain_off(c),
                                c->flags, n_out_host, &consumed, dd_stream(stream));
    c->abs_index += consumed;
    return rc;
}

extern "C" int dd_chain_seek(dd_chain* c, int64_t abs_index, void* stream) {
    DD_REQUIRE(c && abs_index >= 0, "arguments");
    c->abs_index = abs_index;
    if (c->fm) dd_fm_reset(c->fm);
    return dd_fir_reset(c->fir, abs_index == 0 ? DD_HIST_ONES : DD_HIST_ZEROS, nullptr, stream);   // launch-free
}

extern "C" int dd_chain_prime(dd_chain* c, const void* halo_in, int64_t n_halo, int64_t abs_index, void* stream) {
    DD_REQUIRE(c && n_halo >= 0 && abs_index >= 0, "arguments");
    DD_REQUIRE(n_halo <= abs_index, "halo longer than the samples that precede abs_index");
    hipStream_t s = dd_stream(stream);
    if (abs_index == 0) return dd_chain_reset(c, stream);
    DD_REQUIRE(halo_in, "halo_in");
    const bool at_start = (n_halo == abs_index);
    DD_REQUIRE(at_start || n_halo >= (int64_t)c->fir->K - 1 + c->M,
               "halo must hold at least ntaps-1+decim samples (or reach back to the stream start)");
    // Replay the halo as a chunk whose outputs are discarded.  If the halo reaches
    // the stream start the history is the reference's ones (Q1); otherwise it is
    // irrelevant: the last kept output and the last K-1 inputs of the halo have
    // their full windows inside the halo.
    c->abs_index = abs_index - n_halo;
    if (c->fm) dd_fm_reset(c->fm);
    int rc = dd_fir_reset(c->fir, at_start ? DD_HIST_ONES : DD_HIST_ZEROS, nullptr, stream);
    if (rc != DD_OK) return rc;
    const int64_t no = dd_chain_out_count(c, n_halo);
    const size_t ob = (size_t)(no > 0 ? no : 1) * out_elem_size(c->fm);
    if (ob > c->scratch.bytes()) {
        DD_HIP_CHECK(hipStreamSynchronize(s));
        DD_HIP_CHECK(c->scratch.alloc(ob));
    }
    return dd_chain_process(c, halo_in, c->scratch.get(), n_halo, nullptr, stream);
}

// dd_code_warmup (dd_runtime.hip): the runtime loads a translation unit's code object when one of its kernels is first named
int dd_code_touch_chain(void) {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void*)k_chain_dense) == hipSuccess ? DD_OK : DD_ERR_HIP;
}
