// The signal classes no decoder of the reference uses but its package exports:
//   filters.medianFilter        scipy.signal.medfilt(x, n)                       filters.py:322-326   k_medfilt
//   demod_fm.demod_fmAD         np.diff(np.unwrap(np.angle(x))), angle carried   demod_fm.py:57-96    k_fm_angle_diff
//   filters.blackmanHarrisConv  scipy.signal.convolve(x, w, mode='same')         filters.py:145-174   k_conv_same
// The inputs a workgroup needs are staged once in LDS; no state but demod_fmAD's one angle.
#include "dd_common.h"
#include "dd_atan.h"

#define DD_SIG_THREADS 256
#define DD_SIG_PER_LANE (DD_MEDFILT_TILE / DD_SIG_THREADS)
#define DD_CONV_SEG 512              // taps per pass of k_conv_same over the staged samples

static_assert(DD_MEDFILT_TILE % DD_SIG_THREADS == 0, "a lane owns a whole number of outputs");

// ---------------------------------------------------------------- sliding median
// Tile of DD_MEDFILT_TILE outputs per workgroup, its K - 1 halo samples beside it in LDS, positions outside [0, n) staged as 0
// (medfilt's zero padding).  An element "sorts before" another when it is smaller, or equal and earlier: a total order, so in every
// window exactly one element has K / 2 others before it -- the median (NaN aside, see filters.medianFilter).
// A lane owns an ELEMENT, not an output: it counts the elements before its own in the first window that holds it (K compares), then
// slides that window along -- one element leaves, one enters, two compares per step -- through the up to K windows that hold it, and
// wherever the count is K / 2 its element is that window's output.  3 K compares per element instead of K^2 / 2 per output; no two
// lanes write the same output; lanes read consecutive LDS words throughout.  Selection only: an output is one of the inputs, bit for bit.
template <typename T>
__global__ void __launch_bounds__(DD_SIG_THREADS) k_medfilt(const T* __restrict__ x, int64_t n, int K, T* __restrict__ out) {
    __shared__ T win[DD_MEDFILT_TILE + DD_MEDFILT_MAX - 1];
    __shared__ T res[DD_MEDFILT_TILE];
    const int half = K / 2;
    const int W = DD_MEDFILT_TILE + K - 1;
    const int64_t t0 = (int64_t)blockIdx.x * DD_MEDFILT_TILE;
    for (int p = threadIdx.x; p < W; p += DD_SIG_THREADS) {
        const int64_t g = t0 - half + p;
        win[p] = (g >= 0 && g < n) ? x[g] : (T)0;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < DD_MEDFILT_TILE; o += DD_SIG_THREADS)
        res[o] = win[o + half];                         // what a window without a median (NaNs) keeps: its centre
    __syncthreads();
    for (int p = threadIdx.x; p < W; p += DD_SIG_THREADS) {
        const T c = win[p];
        int o = max(0, p - (K - 1));                     // the first window (by its first staged position) that holds p ...
        const int o_end = min(DD_MEDFILT_TILE - 1, p);   // ... and the last
        int before = 0;
        for (int j = 0; j < K; ++j) {
            const T v = win[o + j];
            before += (v < c || (v == c && o + j < p)) ? 1 : 0;
        }
        for (;;) {
            if (before == half) res[o] = c;
            if (o == o_end) break;
            const T gone = win[o], come = win[o + K];
            before -= (gone < c || (gone == c && o < p)) ? 1 : 0;
            before += (come < c || (come == c && o + K < p)) ? 1 : 0;
            ++o;
        }
    }
    __syncthreads();
    for (int o = threadIdx.x; o < DD_MEDFILT_TILE; o += DD_SIG_THREADS)
        if (t0 + o < n) out[t0 + o] = res[o];
}

template <typename T>
static int medfilt_impl(const T* in, T* out, int64_t n, int ksize, hipStream_t s, const char* who) {
    if (n < 0 || ksize < 1 || !(ksize & 1)) {
        dd_set_error("%s: Each element of kernel_size should be odd.", who);
        return DD_ERR_INVALID;
    }
    if (ksize > DD_MEDFILT_MAX) {
        dd_set_error("%s: kernel_size %d is above the device kernel's %d", who, ksize, DD_MEDFILT_MAX);
        return DD_ERR_UNSUPPORTED;
    }
    if (n == 0) return DD_OK;
    DD_REQUIRE(in && out && in != out, "medfilt: null or aliased buffer");
    const int64_t blocks = (n + DD_MEDFILT_TILE - 1) / DD_MEDFILT_TILE;
    DD_REQUIRE(blocks <= 0x7fffffff, "medfilt: signal too long for one launch");
    hipLaunchKernelGGL(k_medfilt<T>, dim3((unsigned)blocks), dim3(DD_SIG_THREADS), 0, s, in, n, ksize, out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_medfilt_f32(const float* in, float* out, int64_t n, int ksize, void* stream) {
    return medfilt_impl<float>(in, out, n, ksize, dd_stream(stream), "dd_medfilt_f32");
}
extern "C" int dd_medfilt_f64(const double* in, double* out, int64_t n, int ksize, void* stream) {
    return medfilt_impl<double>(in, out, n, ksize, dd_stream(stream), "dd_medfilt_f64");
}

// ---------------------------------------------------------------- "same"-mode convolution
// out[i] = sum_k w[k] x[i + s - k], s = (K - 1) / 2, x zero outside [0, n): np.convolve(x, w)[s : s + n], which is what
// scipy.signal.convolve(x, w, mode='same') returns for odd and even K and for n < K.  The taps are taken DD_CONV_SEG at a time: per pass
// the tile's samples and that pass's halo go to LDS, so K is unbounded.  Sums are float64 for both element types (taps are float64; the
// complex64 result is rounded once, at the store); the tap index is uniform over the wave, the sample index consecutive over its lanes.
__device__ __forceinline__ void dd_conv_fma(double& a, double w, double v) { a = fma(w, v, a); }
__device__ __forceinline__ void dd_conv_fma(double2& a, double w, float2 v) {
    a.x = fma(w, (double)v.x, a.x);
    a.y = fma(w, (double)v.y, a.y);
}
__device__ __forceinline__ void dd_conv_store(double* o, double a) { *o = a; }
__device__ __forceinline__ void dd_conv_store(float2* o, double2 a) { *o = make_float2((float)a.x, (float)a.y); }

template <typename T, typename A>
__global__ void __launch_bounds__(DD_SIG_THREADS) k_conv_same(const T* __restrict__ x, int64_t n, const double* __restrict__ w, int K,
                                                              T* __restrict__ out) {
    __shared__ T tile[DD_MEDFILT_TILE + DD_CONV_SEG - 1];
    const int s = (K - 1) / 2;
    const int64_t t0 = (int64_t)blockIdx.x * DD_MEDFILT_TILE;
    A acc[DD_SIG_PER_LANE] = {};
    for (int k0 = 0; k0 < K; k0 += DD_CONV_SEG) {
        const int kk = min(DD_CONV_SEG, K - k0);
        const int64_t gbase = t0 + s - (k0 + kk - 1);
        if (k0) __syncthreads();
        for (int p = threadIdx.x; p < DD_MEDFILT_TILE + kk - 1; p += DD_SIG_THREADS) {
            const int64_t g = gbase + p;
            T v = {};
            if (g >= 0 && g < n) v = x[g];
            tile[p] = v;
        }
        __syncthreads();
        for (int j = 0; j < kk; ++j) {
            const double wv = w[k0 + j];
#pragma unroll
            for (int r = 0; r < DD_SIG_PER_LANE; ++r)
                dd_conv_fma(acc[r], wv, tile[threadIdx.x + DD_SIG_THREADS * r + kk - 1 - j]);
        }
    }
#pragma unroll
    for (int r = 0; r < DD_SIG_PER_LANE; ++r) {
        const int64_t i = t0 + threadIdx.x + DD_SIG_THREADS * r;
        if (i < n) dd_conv_store(out + i, acc[r]);
    }
}

template <typename T, typename A>
static int conv_same_impl(const T* in, T* out, int64_t n, const double* taps, int ntaps, hipStream_t s) {
    DD_REQUIRE(n >= 0 && ntaps >= 1, "conv_same: n >= 0 and at least one tap");
    if (n == 0) return DD_OK;
    DD_REQUIRE(in && out && taps && in != out, "conv_same: null or aliased buffer");
    const int64_t blocks = (n + DD_MEDFILT_TILE - 1) / DD_MEDFILT_TILE;
    DD_REQUIRE(blocks <= 0x7fffffff, "conv_same: signal too long for one launch");
    hipLaunchKernelGGL((k_conv_same<T, A>), dim3((unsigned)blocks), dim3(DD_SIG_THREADS), 0, s, in, n, taps, ntaps, out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_conv_same_f64(const double* in, double* out, int64_t n, const double* taps, int ntaps, void* stream) {
    return conv_same_impl<double, double>(in, out, n, taps, ntaps, dd_stream(stream));
}
extern "C" int dd_conv_same_c64(const float* in_c64, float* out_c64, int64_t n, const double* taps, int ntaps, void* stream) {
    return conv_same_impl<float2, double2>((const float2*)in_c64, (float2*)out_c64, n, taps, ntaps, dd_stream(stream));
}

// ---------------------------------------------------------------- angle-difference discriminator
// out[j] = wrap(angle(x[j + s]) - angle(x[j + s - 1])), the angle before x[0] being the carried one; wrap is np.unwrap's rule seen through
// np.diff: a difference of magnitude below pi stays, one beyond it moves by 2 pi (exactly +-pi stays).  Each lane forms both angles of its
// difference (the kernel is bound by its 12 bytes per sample, not by the second polynomial).  Lane 0 of the launch leaves angle(x[n - 1])
// for the next call, in the other word of the handle's pair.
struct dd_fmad {
    DDDevBuf<float> last;   // device: [2] ping-pong
    int parity = 0;
    int has_last = 0;       // host mirror of "self.__last is not None" (demod_fm.py:88)
};

__global__ void __launch_bounds__(DD_SIG_THREADS) k_fm_angle_diff(const float2* __restrict__ x, float* __restrict__ out, int64_t no, int s,
                                                                  const float* __restrict__ last_in, float* __restrict__ last_out, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * DD_SIG_THREADS;
    for (int64_t j = (int64_t)blockIdx.x * DD_SIG_THREADS + threadIdx.x; j < no; j += stride) {
        const int64_t i = j + s;
        const float2 c = x[i];
        float prev;
        if (i == 0) {
            prev = *last_in;
        } else {
            const float2 p = x[i - 1];
            prev = dd_atan2_poly(p.y, p.x);
        }
        float d = dd_atan2_poly(c.y, c.x) - prev;
        if (d > 3.14159265358979f) d -= 6.28318530717959f;
        else if (d < -3.14159265358979f) d += 6.28318530717959f;
        out[j] = d;
    }
    if (last_out && blockIdx.x == 0 && threadIdx.x == 0) {
        const float2 e = x[n - 1];
        *last_out = dd_atan2_poly(e.y, e.x);
    }
}

extern "C" int dd_fmad_create(dd_fmad** h) {
    DD_REQUIRE(h, "h");
    dd_fmad* f = new dd_fmad();
    hipError_t e = f->last.alloc(2);
    if (e == hipSuccess) e = hipMemset(f->last, 0, 2 * sizeof(float));
    if (e != hipSuccess) {
        delete f;
        dd_set_error("dd_fmad_create: %s", hipGetErrorString(e));
        return (e == hipErrorNoDevice) ? DD_ERR_NODEVICE : DD_ERR_HIP;
    }
    *h = f;
    return DD_OK;
}
extern "C" int dd_fmad_destroy(dd_fmad* h) {
    delete h;
    return DD_OK;
}
extern "C" int dd_fmad_reset(dd_fmad* h) {
    DD_REQUIRE(h, "h");
    h->has_last = 0;
    return DD_OK;
}

extern "C" int dd_fm_angle_diff_c64(dd_fmad* h, const float* in_c64, float* out, int64_t n, int carry, int64_t* n_out, void* stream) {
    DD_REQUIRE(h && n >= 0, "h/n");
    // demod_fm.py:89/93 index anglesOfIQ[-1]: an empty chunk is an IndexError in the reference
    DD_REQUIRE(!(carry && n == 0), "empty chunk with storeState (IndexError in the reference)");
    const int s = (carry && h->has_last) ? 0 : 1;
    const int64_t no = n - s > 0 ? n - s : 0;
    if (n_out) *n_out = no;
    if (n == 0) return DD_OK;
    DD_REQUIRE(in_c64 && (out || no == 0), "null buffer");
    int64_t g = (no + DD_SIG_THREADS - 1) / DD_SIG_THREADS;
    if (g < 1) g = 1;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_fm_angle_diff, dim3((unsigned)g), dim3(DD_SIG_THREADS), 0, dd_stream(stream), (const float2*)in_c64, out, no, s,
                       h->last + h->parity, carry ? h->last + (h->parity ^ 1) : (float*)nullptr, n);
    DD_LAUNCH_CHECK();
    if (carry) {
        h->parity ^= 1;
        h->has_last = 1;
    }
    return DD_OK;
}
