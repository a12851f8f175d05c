// F1/F3 (stand-alone FIR, filters.py:53-75) and F2 (zero-phase filtfilt,
// filters.py:72-73) entry points; F4 (butter, the IIR) is the part dd_iir.h, included below.
//  - complex64 full-rate data goes through the fused-chain kernels of dd_chain.hip
//    with NCO/FM/decimation disabled (same LDS-tiled direct form / MFMA path);
//  - float64 audio-rate data (NOAA tail): LDS-tiled, register-blocked
//    kernels shared with the zero-phase path (dd_filtfilt_kernels.h); one lane per
//    output remains for filters longer than the tile.
#include "dd_chain_kernels.h"
#include "dd_filtfilt_kernels.h"

__global__ void k_fill_f64(double* p, int n, double v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

static int fir_f64_state(dd_fir* f, hipStream_t s) {
    if (f->taps_dev) return DD_OK;
    DDDevBuf<double> taps, h0, h1;                   // (the filter sees them once the taps are up and the history is filled)
    DD_HIP_CHECK(taps.alloc(f->K));
    DD_HIP_CHECK(hipMemcpy(taps, f->taps.data(), sizeof(double) * f->K, hipMemcpyHostToDevice));
    const int nh = f->K > 1 ? f->K - 1 : 1;
    DD_HIP_CHECK(h0.alloc(nh));
    DD_HIP_CHECK(h1.alloc(nh));
    hipLaunchKernelGGL(k_fill_f64, dim3((nh + 255) / 256), dim3(256), 0, s, h0.get(), nh,
                       f->hist_mode == DD_HIST_ONES ? 1.0 : 0.0);
    DD_LAUNCH_CHECK();
    f->taps_dev = std::move(taps);
    f->hist[0] = std::move(h0);
    f->hist[1] = std::move(h1);
    return DD_OK;
}

// float64 side of dd_fir_reset (called from dd_chain.hip)
int dd_fir_reset_f64(dd_fir* f, int mode, const float* hist_host, hipStream_t s) {
    if (!(f->taps_dev || mode == DD_HIST_GIVEN)) return DD_OK;
    int rc = fir_f64_state(f, s);
    if (rc != DD_OK) return rc;
    const int nh = f->K - 1;
    if (nh <= 0) return DD_OK;
    if (mode == DD_HIST_GIVEN) {
        // hist_host holds complex64 pairs; the real path takes the real parts
        std::vector<double> hr(nh);
        for (int i = 0; i < nh; ++i) hr[i] = (double)hist_host[2 * i];
        DD_HIP_CHECK(hipMemcpyAsync(f->hist[f->hpar], hr.data(), sizeof(double) * nh, hipMemcpyHostToDevice, s));
        DD_HIP_CHECK(hipStreamSynchronize(s));
    } else {
        hipLaunchKernelGGL(k_fill_f64, dim3((nh + 255) / 256), dim3(256), 0, s, f->hist[f->hpar].get(), nh,
                           mode == DD_HIST_ONES ? 1.0 : 0.0);
        DD_LAUNCH_CHECK();
    }
    return DD_OK;
}

// float64 history for the real path, given as doubles (lfiltic with initOut values that float32 cannot hold)
extern "C" int dd_fir_reset_hist_f64(dd_fir* f, const double* hist_host, void* stream) {
    DD_REQUIRE(f, "h");
    hipStream_t s = dd_stream(stream);
    const int nh = f->K - 1;
    if (nh <= 0) return DD_OK;
    DD_REQUIRE(hist_host, "hist_host");
    int rc = fir_f64_state(f, s);
    if (rc != DD_OK) return rc;
    DD_HIP_CHECK(hipMemcpyAsync(f->hist[f->hpar], hist_host, sizeof(double) * nh, hipMemcpyHostToDevice, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    return DD_OK;
}

// ---------------------------------------------------------------- float64 real FIR
__global__ void __launch_bounds__(256) k_fir_f64(const double* __restrict__ in, double* __restrict__ out, int64_t n,
                                                 const double* __restrict__ taps, int K,
                                                 const double* __restrict__ hist) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
        const int64_t j = i - k;
        const double v = (j >= 0) ? in[j] : hist[(K - 1) + j];
        acc = fma(taps[k], v, acc);
    }
    out[i] = acc;
}
__global__ void k_hist_update_f64(const double* __restrict__ in, int64_t n, int K, const double* __restrict__ hold,
                                  double* __restrict__ hnew) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K - 1) return;
    const int64_t j = n - (K - 1) + i;
    hnew[i] = (j >= 0) ? in[j] : hold[(K - 1) + j];
}

extern "C" int dd_fir_f64(dd_fir* f, const double* in, double* out, int64_t n, int carry, void* stream) {
    DD_REQUIRE(f && n >= 0, "h/n");
    if (n == 0) return DD_OK;
    DD_REQUIRE(in && out, "null buffer");
    hipStream_t s = dd_stream(stream);
    int rc = fir_f64_state(f, s);
    if (rc != DD_OK) return rc;
    const double* const taps = f->taps_dev;
    double* const hist = f->hist[f->hpar];
    if (dd_ff_tiled_ok(f->K, sizeof(double)) && in != out) {
        // LDS-tiled, register-blocked form (dd_filtfilt_kernels.h), same summation order as the plain kernel
        hipLaunchKernelGGL((k_filtfilt_tile<double, 2>), dim3((unsigned)((n + DD_FF_TILE - 1) / DD_FF_TILE), 1), dim3(DD_FF_THREADS),
                           dd_ff_lds_bytes(f->K), s, in, out, n, 0, taps, f->K, (int64_t)0, (int64_t)0,
                           (const double*)hist);
    } else {
        hipLaunchKernelGGL(k_fir_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n, taps, f->K, hist);
    }
    DD_LAUNCH_CHECK();
    if (carry && f->K > 1) {
        hipLaunchKernelGGL(k_hist_update_f64, dim3((f->K + 254) / 256), dim3(256), 0, s, in, n, f->K, hist,
                           f->hist[f->hpar ^ 1].get());
        DD_LAUNCH_CHECK();
        f->hpar ^= 1;
    }
    return DD_OK;
}

// ---------------------------------------------------------------- filtfilt
// scipy.signal.filtfilt(b,[1],x): ext = odd_ext(x, 3K); forward lfilter with the
// history = ext[0] (zi * x0), reverse, filter again with history = first sample,
// reverse, crop.  Each pass is a direct FIR whose out-of-range taps read the
// pass's first input sample.
template <typename T>
static int filtfilt_impl(const double* taps_host, int K, const T* in, T* out, int64_t n, hipStream_t s) {
    const int edge = 3 * K;
    if (n <= edge) {
        dd_set_error("The length of the input vector x must be greater than padlen, which is %d.", edge);
        return DD_ERR_INVALID;
    }
    const int64_t N = n + 2 * (int64_t)edge;
    const size_t tb = (sizeof(double) * (size_t)K + 255) & ~(size_t)255;
    DDScratchLock scr;                      // held until this entry point has enqueued everything
    int rcs = scr.get(tb + sizeof(T) * (size_t)N, s);
    char* base = scr.ptr;
    if (rcs != DD_OK) return rcs;
    double* taps = reinterpret_cast<double*>(base);
    T* y1 = reinterpret_cast<T*>(base + tb);
    DD_HIP_CHECK(hipMemcpyAsync(taps, taps_host, sizeof(double) * K, hipMemcpyHostToDevice, s));
    if constexpr (sizeof(T) == 8) {
        if (dd_ff_tiled_ok(K, sizeof(T))) {
            dd_filtfilt_launch<T>(in, n, y1, out, n, n, K, taps, 1, s);
        } else {
            hipLaunchKernelGGL(k_filtfilt_fwd<T>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, in, y1, n, edge, taps, K);
            hipLaunchKernelGGL(k_filtfilt_bwd<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y1, out, n, edge, taps, K);
        }
    } else {
        hipLaunchKernelGGL(k_filtfilt_fwd<T>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, in, y1, n, edge, taps, K);
        hipLaunchKernelGGL(k_filtfilt_bwd<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y1, out, n, edge, taps, K);
    }
    hipError_t le = hipGetLastError();
    hipError_t se = hipStreamSynchronize(s);               // the taps are the caller's host memory
    DD_HIP_CHECK(le);
    DD_HIP_CHECK(se);
    return DD_OK;
}

extern "C" int dd_filtfilt_f64(const double* taps_host, int ntaps, const double* in, double* out,
                               int64_t n, int is_complex, void* stream) {
    DD_REQUIRE(taps_host && ntaps >= 1 && in && out && n >= 0, "arguments");
    if (is_complex) return filtfilt_impl<double2>(taps_host, ntaps, (const double2*)in, (double2*)out, n, dd_stream(stream));
    return filtfilt_impl<double>(taps_host, ntaps, in, out, n, dd_stream(stream));
}

extern "C" int dd_filtfilt_c64(const double* taps_host, int ntaps, const float* in_c64, float* out_c64,
                               int64_t n, void* stream) {
    DD_REQUIRE(taps_host && ntaps >= 1 && in_c64 && out_c64 && n >= 0, "arguments");
    return filtfilt_impl<float2>(taps_host, ntaps, (const float2*)in_c64, (float2*)out_c64, n, dd_stream(stream));
}

#include "dd_iir.h"               // F4   dd_iir_create / _destroy, dd_iir_f64, dd_iir_c64, dd_iir_filtfilt_f64 (butter)

// dd_code_warmup (dd_runtime.hip): the runtime loads a translation unit's code object when one of its kernels is first named
int dd_code_touch_fir(void) {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void*)k_fill_f64) == hipSuccess ? DD_OK : DD_ERR_HIP;
}
