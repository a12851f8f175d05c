// Audio-rate rows of the NOAA tail (R2, A1, X1, X2, and 8f-2 / P: the accurate-sync windows and the crude tail), float64 on the
// device so that sync index picks stay bit-exact (H7).  Sizes here are 1e5 .. 1e7 samples.  This file holds what the families share -- the FFT
// library's plan cache (the stand-alone class routes only), the sync entry points' mutex and scratch buffers, the own float64 cyclic
// convolution of 2^17 / 2^18 points (dd_hconv_kernels.h) and its tables -- and includes the six parts (dd_audio_envelope.h,
// dd_audio_resample.h, dd_audio_xcorr.h, dd_audio_sync.h, dd_audio_crude.h, dd_audio_apt.h): one translation unit, split by entry-point
// family in round 6.  The parts are layers: each uses only this file and the parts included before it.
#include "dd_common.h"
#include <hipfft/hipfft.h>
#include <map>
#include <mutex>
#include <vector>
#include <algorithm>
#include <chrono>
#include <complex>

#define DD_FFT_CHECK(expr)                                                     \
    do {                                                                       \
        hipfftResult _r = (expr);                                              \
        if (_r != HIPFFT_SUCCESS) {                                            \
            dd_set_error("%s failed: hipfft error %d", #expr, (int)_r);        \
            return DD_ERR_HIP;                                                 \
        }                                                                      \
    } while (0)

// ---------------------------------------------------------------- plan cache
// (a plan is bound to the stream it is used on -- hipfftSetStream -- and owns a work area: one plan per stream, so two
// host threads on two streams never re-bind or share one)
struct PlanKey {
    int dev;
    int type;
    int64_t n;
    int batch;
    hipStream_t stream;
    bool operator<(const PlanKey& o) const {
        if (dev != o.dev) return dev < o.dev;
        if (type != o.type) return type < o.type;
        if (n != o.n) return n < o.n;
        if (batch != o.batch) return batch < o.batch;
        return stream < o.stream;
    }
};
static std::mutex g_plan_mu;
static std::map<PlanKey, hipfftHandle> g_plans;

static int get_plan(hipfftHandle* out, hipfftType type, int64_t n, int batch, hipStream_t s) {
    int dev = 0;
    DD_HIP_CHECK(hipGetDevice(&dev));
    DD_REQUIRE(n >= 1 && n < (1ll << 31), "FFT length");
    std::lock_guard<std::mutex> lk(g_plan_mu);
    PlanKey k{dev, (int)type, n, batch, s};
    auto it = g_plans.find(k);
    if (it == g_plans.end()) {
        hipfftHandle h;
        DD_FFT_CHECK(hipfftPlan1d(&h, (int)n, type, batch));
        DD_FFT_CHECK(hipfftSetStream(h, s));
        it = g_plans.emplace(k, h).first;
    }
    *out = it->second;
    return DD_OK;
}

static inline unsigned grid1(int64_t n) { return (unsigned)((n + 255) / 256); }

// An entry point that enqueues kernels on buffers another call may free or reuse (the Hilbert-kernel spectra of g_hilb, the pageable
// staging vectors of the uploads) and then returns EARLY on an error must not leave that work in flight: this guard synchronises the
// stream when the function is left without having done so itself.
struct DDSyncOnExit {
    hipStream_t s;
    bool armed;
    explicit DDSyncOnExit(hipStream_t st) : s(st), armed(true) {}
    void done() { armed = false; }
    ~DDSyncOnExit() { if (armed) (void)hipStreamSynchronize(s); }
};

// ---------------------------------------------------------------- the sync entry points' mutex and buffers
// One mutex serialises the entry points that use the buffers below or the Hilbert-kernel spectra cache (dd_audio_envelope.h).
static std::mutex g_sync_mu;
// grow-only scratch per device for the audio-rate entry points' intermediates (no allocation in the steady state:
// a hipMalloc/hipFree pair costs 50-100 us, a dozen of them were half of a correlate + peak-pick call)
// ... and pinned host staging per device for the entry points' one copy back (grow-only; callers hold g_sync_mu).
// One pair per device ordinal, on the heap and never deleted: nothing is freed at exit
struct DDSyncBufs {
    DDDevBuf<char> scratch;
    DDPinnedBuf<char> pinned;
};
static DDSyncBufs* const g_sync_bufs = new DDSyncBufs[64];

static int sync_bufs(DDSyncBufs** out) {
    int dev = 0;
    DD_HIP_CHECK(hipGetDevice(&dev));
    DD_REQUIRE(dev >= 0 && dev < 64, "device index");
    *out = &g_sync_bufs[dev];
    return DD_OK;
}
static int sync_scratch(size_t bytes, char** out) {
    DDSyncBufs* b = nullptr;
    const int rc = sync_bufs(&b);
    if (rc != DD_OK) return rc;
    DD_HIP_CHECK(b->scratch.grow(bytes));
    *out = b->scratch;
    return DD_OK;
}
static int sync_pinned(size_t bytes, char** out) {
    DDSyncBufs* b = nullptr;
    const int rc = sync_bufs(&b);
    if (rc != DD_OK) return rc;
    DD_HIP_CHECK(b->pinned.grow(bytes, hipHostMallocDefault));
    *out = b->pinned;
    return DD_OK;
}

// ---------------------------------------------------------------- own float64 cyclic convolution of length 2^17 / 2^18 (dd_hconv_kernels.h)
#include "dd_hconv_kernels.h"
static std::mutex g_hc_mu;
// device -> W_512^j (512) | W_{2^18}^j (512) | W_{2^17}^j (256).  On the heap, never deleted: nothing is freed at exit
static DDDevBuf<double2>* const g_hc_tab = new DDDevBuf<double2>[64];
static bool hc_length_ok(int64_t M) { return M == ((int64_t)1 << 17) || M == ((int64_t)1 << 18); }
static int hc_lg(int64_t M) { return M == ((int64_t)1 << 18) ? 9 : 8; }      // rows of 2^lg points: 9 (M = 2^18) or 8 (M = 2^17)
// the device's table; W_512^j is its head, the row pass's W_M^j follows at DD_HC_N (M = 2^18) or 2 DD_HC_N (M = 2^17)
static int hc_tables(const double2** tab) {
    int dev = 0;
    DD_HIP_CHECK(hipGetDevice(&dev));
    DD_REQUIRE(dev >= 0 && dev < 64, "device index");
    std::lock_guard<std::mutex> lk(g_hc_mu);
    if (!g_hc_tab[dev]) {
        std::vector<double2> h(2 * DD_HC_N + 256);
        const long double tp = 6.283185307179586476925286766559L;
        for (int j = 0; j < DD_HC_N; ++j) {
            h[j] = make_double2((double)cosl(tp * j / DD_HC_N), (double)-sinl(tp * j / DD_HC_N));
            h[DD_HC_N + j] = make_double2((double)cosl(tp * j / 262144.0L), (double)-sinl(tp * j / 262144.0L));
        }
        for (int j = 0; j < 256; ++j) h[2 * DD_HC_N + j] = make_double2((double)cosl(tp * j / 131072.0L), (double)-sinl(tp * j / 131072.0L));
        DDDevBuf<double2> d;                                     // (the slot takes it once it is filled)
        DD_HIP_CHECK(d.alloc(h.size()));
        hipError_t e = hipMemcpy(d, h.data(), sizeof(double2) * h.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) { dd_set_error("twiddle table upload: %s", hipGetErrorString(e)); return DD_ERR_HIP; }
        g_hc_tab[dev] = std::move(d);
    }
    *tab = g_hc_tab[dev];
    return DD_OK;
}
template <int LG, typename SRC, typename SPEC, typename DST>
static int hc_run_lg(const SRC& src, const SPEC& spec, const DST& dst, double2* T, int jobs, hipStream_t s) {
    const double2* tab = nullptr;
    const int rc = hc_tables(&tab);
    if (rc != DD_OK) return rc;
    static DDOncePerDevice once;                                 // the column passes take 64 KB of dynamic LDS: once per device and instantiation
    if (once.need()) {
        DD_HIP_CHECK((hc_set_lds_attr<LG, SRC, DST>()));
        once.mark();
    }
    hc_convolve<LG>(src, spec, dst, T, jobs, tab, tab + (LG == 9 ? 1 : 2) * DD_HC_N, s);
    return DD_OK;
}
// THE door to the transform: `jobs` cyclic convolutions of M points (hc_length_ok(M)), src -> times spec -> dst, through the image T [jobs][M]
template <typename SRC, typename SPEC, typename DST>
static int hc_run(int64_t M, const SRC& src, const SPEC& spec, const DST& dst, double2* T, int jobs, hipStream_t s) {
    return hc_lg(M) == 9 ? hc_run_lg<9>(src, spec, dst, T, jobs, s) : hc_run_lg<8>(src, spec, dst, T, jobs, s);
}
// a spectrum of M bins into the row pass's order, scaled
static void hc_perm(int64_t M, const double2* in, double2* out, int hermitian, double scale, hipStream_t s) {
    if (hc_lg(M) == 9) hipLaunchKernelGGL(k_hc_perm<9>, dim3((unsigned)(M / 256)), dim3(256), 0, s, in, out, hermitian, scale);
    else hipLaunchKernelGGL(k_hc_perm<8>, dim3((unsigned)(M / 256)), dim3(256), 0, s, in, out, hermitian, scale);
}
// envelope of `nwin` windows (two per image) through the three launches; HHp: the kernel spectrum in row-pass order
static int hc_envelope(int64_t M, const float2* X, int64_t L, int nwin, const double2* HHp, double2* W, double* ENV, hipStream_t s) {
    const HcEnvIO io = {X, L, L - 1, nwin, ENV};
    return hc_run(M, io, HcOneSpec{HHp}, io, W, (nwin + 1) / 2, s);
}

// ---------------------------------------------------------------- the entry-point families (round 6: one file each, one translation unit)
#include "dd_audio_envelope.h"      // A1   dd_am_envelope_f64; the Hilbert-kernel spectra and the block envelope every part uses
#include "dd_audio_resample.h"      // R2   dd_resample_fft_f64 / _chunks, dd_rpoly_*
#include "dd_audio_xcorr.h"         // X1, X2   dd_xcorr_norm_f64, dd_find_peaks_f64; the scan, the run-length correlation and the peak pick
#include "dd_audio_sync.h"          // 8f-2  dd_noaa_sync_windows(_multi), dd_noaa_prepare
#include "dd_audio_crude.h"         // P     dd_noaa_crude_tail
#include "dd_audio_apt.h"           // APT image: dd_median_segments_f64, dd_apt_lines_f64, dd_apt_map_u8, dd_apt_color_u8

// the stream is about to be destroyed (dd_stream_destroy, after it has been synchronised): its plans (with their work areas) and
// its chirp-z tables go with it -- a later stream that happens to get the same address must not inherit a plan bound to a dead
// stream, and dead entries must not fill the 64-entry chirp-z cache
void dd_audio_forget_stream(hipStream_t s) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        for (auto it = g_plans.begin(); it != g_plans.end();) {
            if (it->first.dev == dev && it->first.stream == s) {
                (void)hipfftDestroy(it->second);
                it = g_plans.erase(it);
            } else {
                ++it;
            }
        }
    }
    czt_forget_stream(dev, s);
}

// dd_code_warmup (dd_runtime.hip): the runtime loads a translation unit's code object when one of its kernels is first named
int dd_code_touch_audio(void) {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void*)k_cvt_f32_f64) == hipSuccess ? DD_OK : DD_ERR_HIP;
}
