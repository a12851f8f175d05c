// D1: the Doppler front end of sandbox/frequency_shift.py -- make_fft (:5-44) as a spectrum waterfall over the raw uint8 I,Q
// recording resident in HBM, and the per-row band argmax of find_shift (:92-95).  Included by dd_runtime.hip.
//
// dd_waterfall_u8 runs two kernels.  k_waterfall_fft: one workgroup of 256 threads per (row, segment of the row's windows); a
// window's pairs are read once, widened in registers (I - 127, Q - 127) and written to LDS as complex f64 (16 B x window, 128 KB
// at 8192), transformed in place by radix-4 decimation-in-frequency passes (one radix-2 pass at the end when log2(window) is
// odd: 8192 = 4^6 x 2), and |X|, rounded to f32, is added to per-thread f32 accumulators in LDS-position order.  The transform
// is float64 like the reference's (np.fft.fft): a row of one window is the log of single bins, and a bin far below the
// spectrum's rms keeps none of its digits through a float32 transform, whose error is 1e-7 of the rms.  The output of an in-place DIF
// is digit reversed; the permutation is undone once per row, not per window, by k_waterfall_rows, which sums a row's segments
// in segment order, applies fftshift and log(sum / window / every) in float64 and stores float32.  The split of a row's windows
// into segments depends on the row length alone, every sum has one order, and nothing is accumulated with atomics.
#pragma once

#define DD_WF_THREADS 256
#define DD_WF_MAXWIN 8192
#define DD_WF_ACC (DD_WF_MAXWIN / DD_WF_THREADS)
#define DD_WF_SEG_WINDOWS 8          // windows per segment aimed at
#define DD_WF_MAX_SEGS 16

struct DDWfGeom {
    int n, log2n;                    // window
    int row_len;                     // ceil(every): slices per row, full or not
    int nseg, per;                   // segments per row, windows per segment (the last may hold fewer)
    long long n_full;                // full windows in the recording
};

// LDS position that holds bin k after the passes: the radix-4 digits of k, least significant first, are the position's digits, most
// significant first (the last digit is binary when log2(window) is odd)
__device__ __forceinline__ int dd_wf_pos_of_bin(int k, int n) {
    int p = 0, len = n;
    while (len >= 4) {
        const int q = len >> 2;
        p += (k & 3) * q;
        k >>= 2;
        len = q;
    }
    if (len == 2) p += k;
    return p;
}

// exp(-2 pi i j / len): 2 j / len is exact, sincospi is good to an ulp of float64
__device__ __forceinline__ double2 dd_wf_twiddle(int j, int len) {
    double sn, cs;
    sincospi(2.0 * (double)j / (double)len, &sn, &cs);
    return make_double2(cs, -sn);
}

__device__ __forceinline__ double2 dd_wf_cmul(double2 a, double2 w) {
    return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

template <bool ALIGN4>
__global__ void __launch_bounds__(DD_WF_THREADS) k_waterfall_fft(const uint8_t* __restrict__ raw, DDWfGeom g, float* __restrict__ partial) {
    extern __shared__ double2 wf_s[];
    const int tid = threadIdx.x;
    const int n = g.n;
    const long long row = blockIdx.x / g.nseg;
    const int seg = blockIdx.x % g.nseg;
    long long w0 = row * g.row_len + (long long)seg * g.per;
    long long w1 = row * g.row_len + min((seg + 1) * g.per, g.row_len);
    if (w1 > g.n_full) w1 = g.n_full;                    // (a partial tail counts towards the row but adds nothing)
    float acc[DD_WF_ACC];
#pragma unroll
    for (int e = 0; e < DD_WF_ACC; e++) acc[e] = 0.0f;

    for (long long w = w0; w < w1; w++) {
        const uint8_t* src = raw + w * 2 * (long long)n;
        if (ALIGN4) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
            for (int v = tid; v < n / 2; v += DD_WF_THREADS) {
                const uint32_t u = s4[v];
                wf_s[2 * v] = make_double2((double)(int)(u & 0xff) - 127.0, (double)(int)((u >> 8) & 0xff) - 127.0);
                wf_s[2 * v + 1] = make_double2((double)(int)((u >> 16) & 0xff) - 127.0, (double)(int)(u >> 24) - 127.0);
            }
        } else {
            const uint16_t* s2 = reinterpret_cast<const uint16_t*>(src);
            for (int v = tid; v < n; v += DD_WF_THREADS) {
                const uint32_t u = s2[v];
                wf_s[v] = make_double2((double)(int)(u & 0xff) - 127.0, (double)(int)(u >> 8) - 127.0);
            }
        }
        __syncthreads();
        int len = n;
        for (int lq = g.log2n - 2; len >= 4; len >>= 2, lq -= 2) {
            const int q = 1 << lq;
            for (int b = tid; b < n / 4; b += DD_WF_THREADS) {
                const int j = b & (q - 1);
                const int base = ((b >> lq) << (lq + 2)) + j;
                const double2 a0 = wf_s[base], a1 = wf_s[base + q], a2 = wf_s[base + 2 * q], a3 = wf_s[base + 3 * q];
                const double2 t0 = make_double2(a0.x + a2.x, a0.y + a2.y), t1 = make_double2(a0.x - a2.x, a0.y - a2.y);
                const double2 t2 = make_double2(a1.x + a3.x, a1.y + a3.y);
                const double2 t3 = make_double2(a1.y - a3.y, -(a1.x - a3.x));          // -j (a1 - a3)
                const double2 tw1 = dd_wf_twiddle(j, len);
                const double2 tw2 = dd_wf_cmul(tw1, tw1), tw3 = dd_wf_cmul(tw2, tw1);
                wf_s[base] = make_double2(t0.x + t2.x, t0.y + t2.y);
                wf_s[base + q] = dd_wf_cmul(make_double2(t1.x + t3.x, t1.y + t3.y), tw1);
                wf_s[base + 2 * q] = dd_wf_cmul(make_double2(t0.x - t2.x, t0.y - t2.y), tw2);
                wf_s[base + 3 * q] = dd_wf_cmul(make_double2(t1.x - t3.x, t1.y - t3.y), tw3);
            }
            __syncthreads();
        }
        if (len == 2) {
            for (int b = tid; b < n / 2; b += DD_WF_THREADS) {
                const double2 a0 = wf_s[2 * b], a1 = wf_s[2 * b + 1];
                wf_s[2 * b] = make_double2(a0.x + a1.x, a0.y + a1.y);
                wf_s[2 * b + 1] = make_double2(a0.x - a1.x, a0.y - a1.y);
            }
            __syncthreads();
        }
#pragma unroll
        for (int e = 0; e < DD_WF_ACC; e++) {
            const int p = tid + e * DD_WF_THREADS;
            if (p < n) {
                const double2 x = wf_s[p];
                acc[e] += (float)sqrt(x.x * x.x + x.y * x.y);
            }
        }
        __syncthreads();                                 // (the next window's samples overwrite the spectrum)
    }
    float* dst = partial + (long long)blockIdx.x * n;
#pragma unroll
    for (int e = 0; e < DD_WF_ACC; e++) {
        const int p = tid + e * DD_WF_THREADS;
        if (p < n) dst[p] = acc[e];
    }
}

__global__ void __launch_bounds__(256) k_waterfall_rows(const float* __restrict__ partial, float* __restrict__ out, int64_t total,
                                                        int n, int log2n, int nseg, double every) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i >> log2n;
        const int c = (int)(i & (n - 1));
        const int p = dd_wf_pos_of_bin((c + n / 2) & (n - 1), n);      // fftshift: column c holds bin c - n/2
        const float* src = partial + row * nseg * (int64_t)n + p;
        float s = src[0];
        for (int k = 1; k < nseg; k++) s += src[(int64_t)k * n];
        out[i] = (float)log((double)s / (double)n / every);
    }
}

static int dd_wf_geometry(int64_t raw_bytes, int window, double every, DDWfGeom* g, int64_t* rows) {
    DD_REQUIRE(window >= 16 && window <= DD_WF_MAXWIN && (window & (window - 1)) == 0, "dd_waterfall_u8: window must be a power of two in 16..8192");
    DD_REQUIRE(raw_bytes >= 0 && (raw_bytes & 1) == 0, "dd_waterfall_u8: raw_bytes must be even (I,Q pairs)");
    DD_REQUIRE(every > 0.0 && every < 1e15, "dd_waterfall_u8: every");
    const int64_t span = 2 * (int64_t)window;
    const int64_t n_full = raw_bytes / span, n_slices = (raw_bytes + span - 1) / span;
    DD_REQUIRE(n_full >= 1, "dd_waterfall_u8: the recording is shorter than one window");
    DD_REQUIRE(n_slices < ((int64_t)1 << 31), "dd_waterfall_u8: more than 2^31 windows");
    const double r = ceil(every);
    DD_REQUIRE(!(r <= 1.0 && n_slices != n_full), "dd_waterfall_u8: every <= 1 with a partial last window (the reference fails in fftshift)");
    g->n = window;
    g->log2n = 0;
    while ((1 << g->log2n) < window) g->log2n++;
    g->n_full = n_full;
    if (r > (double)n_slices) {          // no row closes
        *rows = 0;
        g->row_len = 1; g->nseg = 1; g->per = 1;
        return DD_OK;
    }
    g->row_len = (int)r;                 // 1 <= r <= n_slices < 2^31
    *rows = n_slices / g->row_len;
    g->nseg = (g->row_len + DD_WF_SEG_WINDOWS - 1) / DD_WF_SEG_WINDOWS;
    if (g->nseg > DD_WF_MAX_SEGS) g->nseg = DD_WF_MAX_SEGS;
    g->per = (g->row_len + g->nseg - 1) / g->nseg;
    return DD_OK;
}

extern "C" int dd_waterfall_u8(const uint8_t* raw_iq, int64_t raw_bytes, int window, double every, float* out_rows, int64_t max_rows,
                               int64_t* n_rows, void* stream) {
    DDWfGeom g;
    int64_t rows = 0;
    const int rc = dd_wf_geometry(raw_bytes, window, every, &g, &rows);
    if (rc != DD_OK) return rc;
    if (n_rows) *n_rows = rows;
    if (!out_rows || rows == 0) return DD_OK;
    DD_REQUIRE(raw_iq != nullptr, "dd_waterfall_u8: null recording");
    DD_REQUIRE(((uintptr_t)raw_iq & 1) == 0, "dd_waterfall_u8: the recording must start on an I,Q pair boundary");
    DD_REQUIRE(rows <= max_rows, "dd_waterfall_u8: out_rows holds fewer than the row count");
    DD_REQUIRE(rows * g.nseg < (int64_t)1 << 31, "dd_waterfall_u8: too many workgroups");
    hipStream_t s = dd_stream(stream);
    DDScratchLock scr;
    const int src = scr.get(sizeof(float) * (size_t)rows * g.nseg * window, s);
    if (src != DD_OK) return src;
    float* partial = reinterpret_cast<float*>(scr.ptr);
    const dim3 grid((unsigned)(rows * g.nseg)), block(DD_WF_THREADS);
    const size_t lds = sizeof(double2) * (size_t)window;             // 128 KB at 8192: above the 64 KB a launch gets unasked
    static DDOncePerDevice attr;
    if (attr.need()) {
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_waterfall_fft<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(sizeof(double2) * DD_WF_MAXWIN)));
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_waterfall_fft<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(sizeof(double2) * DD_WF_MAXWIN)));
        attr.mark();
    }
    if (((uintptr_t)raw_iq & 3) == 0) hipLaunchKernelGGL(k_waterfall_fft<true>, grid, block, lds, s, raw_iq, g, partial);
    else hipLaunchKernelGGL(k_waterfall_fft<false>, grid, block, lds, s, raw_iq, g, partial);
    DD_LAUNCH_CHECK();
    const int64_t total = rows * window;
    hipLaunchKernelGGL(k_waterfall_rows, dim3(dd_grid_for(total, 256)), dim3(256), 0, s, partial, out_rows, total, window, g.log2n,
                       g.nseg, every);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// np.argmax over [band_start, band_stop) of each row: the first maximum, and like np.argmax a NaN counts as larger than every
// number, so the first NaN of the band wins.  One workgroup per row; a thread keeps the best of its strided columns, the 256
// candidates are reduced pairwise in one fixed order, the lower index winning a tie (two NaNs tie).  A thread without a column
// offers (-inf, 0x7fffffff), which loses every tie: thread 0 always has a column, so the result lies inside the band.
__device__ __forceinline__ bool dd_argmax_better(float v, int c, float best, int idx) {
    if (v != v) return best == best || c < idx;
    return best == best && (v > best || (v == best && c < idx));
}

__global__ void __launch_bounds__(256) k_band_argmax_f32(const float* __restrict__ rows, int width, int band_start, int band_stop,
                                                         int32_t* __restrict__ out) {
    __shared__ float sv[256];
    __shared__ int si[256];
    const float* r = rows + (int64_t)blockIdx.x * width;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int c = band_start + (int)threadIdx.x; c < band_stop; c += 256) {
        const float v = r[c];
        if (dd_argmax_better(v, c, best, idx)) { best = v; idx = c; }
    }
    sv[threadIdx.x] = best;
    si[threadIdx.x] = idx;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const float v = sv[threadIdx.x + h];
            const int c = si[threadIdx.x + h];
            if (dd_argmax_better(v, c, sv[threadIdx.x], si[threadIdx.x])) { sv[threadIdx.x] = v; si[threadIdx.x] = c; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = si[0] - band_start;
}

extern "C" int dd_band_argmax_f32(const float* rows_f32, int64_t rows, int width, int band_start, int band_stop, int32_t* out_idx,
                                  void* stream) {
    DD_REQUIRE(rows >= 0 && rows < ((int64_t)1 << 31) && width > 0, "dd_band_argmax_f32: rows / width");
    DD_REQUIRE(band_start >= 0 && band_start < band_stop && band_stop <= width, "dd_band_argmax_f32: the band leaves [0, width)");
    if (rows == 0) return DD_OK;
    DD_REQUIRE(rows_f32 && out_idx, "dd_band_argmax_f32: null buffer");
    hipLaunchKernelGGL(k_band_argmax_f32, dim3((unsigned)rows), dim3(256), 0, dd_stream(stream), rows_f32, width, band_start, band_stop,
                       out_idx);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
