// Slow-scan television, PD modes (beyond the reference; DESIGN.md section 4.21 defines every stage, sstv.py restates each kernel in
// NumPy), included by dd_afsk.hip; built with -ffp-contract=off.  All arithmetic is float64 with + - * / comparisons, ceil and rint,
// each rounded on its own, so the device and the restatement agree bit for bit.  No math-library call: the taps, the band-edge
// phasors and rate / 2 pi come from the host.
//
//   k_sstv_lag        -- one thread per output: z[n] = sum_k h[k] x[n-k] (complex taps, k ascending), d[n] = z[n] conj(z[n-1])
//   k_sstv_classes    -- one thread per sample: the tone class of d[n] by cross-product signs against six band-edge phasors
//   k_sstv_scan_*     -- P[i] = how many of v[0..i) equal a value: block sums, their scan (dd_candidates.h's k_scan_tops), the blocks'
//                        own scans
//   k_sstv_run_*      -- maximal runs of window counts >= a threshold, one wave per run for the first index of its maximum
//   k_sstv_pixels     -- one wave per segment, one lane per pixel: sum of d over the pixel, polynomial arctangent, level
//   k_sstv_color      -- one thread per pixel column of a line pair: Y0, Cr, Cb, Y1 -> two RGB rows, integer arithmetic
#pragma once

#define DD_SSTV_TILE 256              // outputs per workgroup of k_sstv_lag (mirrored by sstv.LAG_TILE)
#define DD_SSTV_MAX_K 511             // taps at most (odd)
#define DD_SSTV_SCAN 1024             // elements per workgroup of the scans: 256 threads, 4 each

__global__ void __launch_bounds__(DD_SSTV_TILE) k_sstv_lag(const double* __restrict__ x, int64_t n, const double* __restrict__ taps, int K,
                                                           double2* __restrict__ d) {
    __shared__ double xs[DD_SSTV_TILE + DD_SSTV_MAX_K + 1];          // xs[j] = x[base - K + j], 0 outside the input
    __shared__ double hr[DD_SSTV_MAX_K], hi[DD_SSTV_MAX_K];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * DD_SSTV_TILE;
    for (int j = tid; j < DD_SSTV_TILE + K; j += DD_SSTV_TILE) {
        const int64_t i = base - K + j;
        xs[j] = (i >= 0 && i < n) ? x[i] : 0.0;
    }
    for (int k = tid; k < K; k += DD_SSTV_TILE) {
        hr[k] = taps[k];
        hi[k] = taps[K + k];
    }
    __syncthreads();
    const int64_t i = base + tid;
    if (i >= n) return;
    double zr = 0.0, zi = 0.0, pr = 0.0, pi = 0.0;                   // z[i] and z[i-1], the same sums in the same order
    for (int k = 0; k < K; ++k) {
        const double a = xs[tid + K - k], b = xs[tid + K - 1 - k];
        const double r = hr[k], m = hi[k];
        zr = zr + r * a;
        zi = zi + m * a;
        pr = pr + r * b;
        pi = pi + m * b;
    }
    if (i == 0) pr = pi = 0.0;
    d[i] = make_double2(zr * pr + zi * pi, zi * pr - zr * pi);
}

struct DDSstvEdges {
    double c[6], s[6];                // cos and sin of the six band edges' angles, ascending, all in (0, pi)
};

// class 0 none, 1 / 2 / 3 the 1100 / 1200 / 1300 Hz bands [edge 0, 1), [1, 2), [2, 3), 4 the leader band [edge 4, 5).
// angle(d) >= angle(e) <=> e.re * d.im >= e.im * d.re for two angles in (0, pi); im <= 0, zero and NaN give no class
__global__ void __launch_bounds__(256) k_sstv_classes(const double2* __restrict__ d, int64_t n, const DDSstvEdges e,
                                                      int8_t* __restrict__ cls) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double2 v = d[i];
    int c = 0;
    if (v.y > 0.0) {
        bool ge[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) ge[j] = e.c[j] * v.y >= e.s[j] * v.x;
        if (ge[0] && !ge[1]) c = 1;
        else if (ge[1] && !ge[2]) c = 2;
        else if (ge[2] && !ge[3]) c = 3;
        else if (ge[4] && !ge[5]) c = 4;
    }
    cls[i] = (int8_t)c;
}

// bsum[b] = how many of v[1024 b .. 1024 b + 1024) equal target
__global__ void __launch_bounds__(256) k_sstv_scan_blocks(const int8_t* __restrict__ v, int64_t n, int target, int* __restrict__ bsum) {
    __shared__ int sh[256];
    const int64_t at = (int64_t)blockIdx.x * DD_SSTV_SCAN + 4 * threadIdx.x;
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) c += (at + j < n && v[at + j] == target) ? 1 : 0;
    const int s = dd_scan256(c, sh);
    if (threadIdx.x == 255) bsum[blockIdx.x] = s;
}

// P[0] = 0, P[i + 1] = how many of v[0..i] equal target; boff = the scanned block sums
__global__ void __launch_bounds__(256) k_sstv_scan_write(const int8_t* __restrict__ v, int64_t n, int target, const int* __restrict__ boff,
                                                         int* __restrict__ P) {
    __shared__ int sh[256];
    const int64_t at = (int64_t)blockIdx.x * DD_SSTV_SCAN + 4 * threadIdx.x;
    int f[4], c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[j] = (at + j < n && v[at + j] == target) ? 1 : 0;
        c += f[j];
    }
    int run = boff[blockIdx.x] + dd_scan256(c, sh) - c;
    if (blockIdx.x == 0 && threadIdx.x == 0) P[0] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        run += f[j];
        if (at + j < n) P[at + j + 1] = run;
    }
}

// the three scan launches; bsum holds n / 1024 + 2 ints
static int dd_sstv_scan(const int8_t* v, int64_t n, int target, int* bsum, int* P, hipStream_t s) {
    const int64_t nb = (n + DD_SSTV_SCAN - 1) / DD_SSTV_SCAN;
    hipLaunchKernelGGL(k_sstv_scan_blocks, dim3((unsigned)nb), dim3(256), 0, s, v, n, target, bsum);
    DD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_scan_tops, dim3(1), dim3(256), 0, s, bsum, nb);
    DD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sstv_scan_write, dim3((unsigned)nb), dim3(256), 0, s, v, n, target, (const int*)bsum, P);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// count(i) = P[i + W] - P[i], the class count in [i, i + W), for i < m = n - W + 1; mask[i] = 1 where a run of count >= T starts
__global__ void __launch_bounds__(256) k_sstv_run_starts(const int* __restrict__ P, int64_t m, int64_t W, int T, int8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const bool above = P[i + W] - P[i] >= T;
    const bool before = i > 0 && P[i - 1 + W] - P[i - 1] >= T;
    mask[i] = (above && !before) ? 1 : 0;
}

// starts[Q[i]] = i for every run start below the capacity (Q = the scan of mask: ordered, and nothing written past cap)
__global__ void __launch_bounds__(256) k_sstv_run_list(const int8_t* __restrict__ mask, const int* __restrict__ Q, int64_t m,
                                                       int64_t* __restrict__ starts, int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m || !mask[i]) return;
    const int64_t at = Q[i];
    if (at < cap) starts[at] = i;
}

// one wave per run: from its start to the first count below T, the first index of the largest count; pos[r] = start in, peak out
__global__ void __launch_bounds__(64) k_sstv_run_peak(const int* __restrict__ P, int64_t m, int64_t W, int T, int64_t* __restrict__ pos) {
    const int lane = threadIdx.x;
    int best = -1;
    int64_t at = 0;
    for (int64_t base = pos[blockIdx.x]; ; base += 64) {
        const int64_t i = base + lane;
        const int c = i < m ? P[i + W] - P[i] : -1;
        const unsigned long long below = __ballot(c < T);
        const int stop = below ? __ffsll((long long)below) - 1 : 64;         // lanes before the run's end
        if (lane < stop && c > best) {                                       // (strictly greater: the first maximum stays)
            best = c;
            at = i;
        }
        if (below) break;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int ob = __shfl_xor(best, o);
        const int64_t oa = __shfl_xor(at, o);
        if (ob > best || (ob == best && oa < at)) {
            best = ob;
            at = oa;
        }
    }
    if (lane == 0) pos[blockIdx.x] = at;
}

struct DDSstvPix {
    double step, c1;                  // samples per pixel; rate / 2 pi (computed by the host)
};

// The angle of (x, y), y >= 0 and not both zero, in [0, pi]: t = min / max of |x| and y, u = (t - 1) / (t + 1) above tan(pi / 8),
// the odd series of the arctangent to u^17 by Horner in u * u (sstv.atan_host is this line by line)
__device__ __forceinline__ double dd_sstv_angle(double x, double y) {
    const double ax = x < 0.0 ? -x : x;
    const bool swap = y > ax;
    const double t = (swap ? ax : y) / (swap ? y : ax);
    const bool big = t > 0.41421356237309503;
    const double u = big ? (t - 1.0) / (t + 1.0) : t;
    const double w = u * u;
    double p = 1.0 / 17.0;
    p = p * w + (-1.0 / 15.0);
    p = p * w + (1.0 / 13.0);
    p = p * w + (-1.0 / 11.0);
    p = p * w + (1.0 / 9.0);
    p = p * w + (-1.0 / 7.0);
    p = p * w + (1.0 / 5.0);
    p = p * w + (-1.0 / 3.0);
    p = p * w + 1.0;
    double r = u * p;
    if (big) r = 0.78539816339744828 + r;
    if (swap) r = 1.5707963267948966 - r;
    if (x < 0.0) r = 3.1415926535897931 - r;
    return r;
}

// ceil(v) clipped to [0, n]; a NaN gives 0
__device__ __forceinline__ int64_t dd_sstv_edge(double v, int64_t n) {
    const double c = ceil(v);
    if (!(c >= 0.0)) return 0;
    return c > (double)n ? n : (int64_t)c;
}

__global__ void __launch_bounds__(64) k_sstv_pixels(const double2* __restrict__ d, int64_t n, const double* __restrict__ t0s, int W,
                                                    const DDSstvPix prm, uint8_t* __restrict__ levels, unsigned long long* __restrict__ empty) {
    const int lane = threadIdx.x;
    const double t0 = t0s[blockIdx.x];
    uint8_t* out = levels + (int64_t)blockIdx.x * W;
    int none = 0;
    for (int p = lane; p < W; p += 64) {
        const int64_t a = dd_sstv_edge(t0 + (double)p * prm.step, n);
        const int64_t b = dd_sstv_edge(t0 + (double)(p + 1) * prm.step, n);
        double sr = 0.0, si = 0.0;
        for (int64_t i = a; i < b; ++i) {
            const double2 v = d[i];
            sr = sr + v.x;
            si = si + v.y;
        }
        double lv = 0.0;
        if (b <= a || (sr == 0.0 && si == 0.0)) {
            ++none;
        } else {
            const double ang = si < 0.0 ? 0.0 : dd_sstv_angle(sr, si);
            const double v = rint((ang * prm.c1 - 1500.0) * 255.0 / 800.0);
            lv = v >= 255.0 ? 255.0 : (v > 0.0 ? v : 0.0);                   // (a NaN gives 0)
        }
        out[p] = (uint8_t)lv;
    }
    for (int o = 32; o > 0; o >>= 1) none += __shfl_xor(none, o);
    if (lane == 0 && none) atomicAdd(empty, (unsigned long long)none);
}

__device__ __forceinline__ uint8_t dd_sstv_clip100(int v) {                  // floor(v / 100) clipped to 0..255
    return v < 0 ? 0 : (v >= 25600 ? 255 : (uint8_t)(v / 100));
}

// levels[pair][4][W] = Y0, Cr, Cb, Y1 -> rgb[2 pair][W][3], rgb[2 pair + 1][W][3]
__global__ void __launch_bounds__(256) k_sstv_color(const uint8_t* __restrict__ levels, int64_t npairs, int W, uint8_t* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs * W) return;
    const int64_t pair = i / W;
    const int p = (int)(i - pair * W);
    const uint8_t* seg = levels + pair * 4 * W + p;
    const int cr = seg[W], cb = seg[2 * W];
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        const int y = seg[row ? 3 * W : 0];
        uint8_t* o = rgb + ((2 * pair + row) * W + p) * 3;
        o[0] = dd_sstv_clip100(100 * y + 140 * cr - 17850);
        o[1] = dd_sstv_clip100(100 * y - 71 * cr - 33 * cb + 13260);
        o[2] = dd_sstv_clip100(100 * y + 178 * cb - 22695);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the C entries
extern "C" int dd_sstv_lag(const double* x, int64_t n, const double* taps_host, int K, void* d, void* stream) {
    DD_REQUIRE(n >= 0, "dd_sstv_lag: negative size");
    DD_REQUIRE(K >= 1 && K <= DD_SSTV_MAX_K && (K & 1) == 1, "dd_sstv_lag: the tap count must be odd and at most 511");
    DD_REQUIRE(taps_host != nullptr, "dd_sstv_lag: taps");
    if (n == 0) return DD_OK;
    DD_REQUIRE(x != nullptr && d != nullptr, "dd_sstv_lag: null buffer");
    hipStream_t s = dd_stream(stream);
    DDScratchLock scr;
    int rc = scr.get(2 * (size_t)K * sizeof(double), s);
    if (rc != DD_OK) return rc;
    DD_HIP_CHECK(hipMemcpyAsync(scr.ptr, taps_host, 2 * (size_t)K * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_sstv_lag, dim3((unsigned)((n + DD_SSTV_TILE - 1) / DD_SSTV_TILE)), dim3(DD_SSTV_TILE), 0, s, x, n,
                       (const double*)scr.ptr, K, (double2*)d);
    DD_LAUNCH_CHECK();
    DD_HIP_CHECK(hipStreamSynchronize(s));                                   // (the taps left pageable host memory)
    return DD_OK;
}

extern "C" int dd_sstv_classes(const void* d, int64_t n, const double* edges_host, int8_t* cls, void* stream) {
    DD_REQUIRE(n >= 0, "dd_sstv_classes: negative size");
    DD_REQUIRE(edges_host != nullptr, "dd_sstv_classes: edges");
    if (n == 0) return DD_OK;
    DD_REQUIRE(d != nullptr && cls != nullptr, "dd_sstv_classes: null buffer");
    DDSstvEdges e;
    memcpy(&e, edges_host, sizeof(e));
    hipLaunchKernelGGL(k_sstv_classes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dd_stream(stream), (const double2*)d, n, e, cls);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_sstv_runs(const int8_t* cls, int64_t n, int target, int64_t window, int64_t thresh, int64_t* pos, int64_t cap,
                            int64_t* count_host, void* stream) {
    DD_REQUIRE(n >= 0 && cap >= 0 && n <= 0x7FFFFFF0LL, "dd_sstv_runs: sizes");
    DD_REQUIRE(window >= 1 && window <= 0x7FFFFFF0LL, "dd_sstv_runs: the window must hold at least one sample");
    DD_REQUIRE(thresh >= 1 && thresh <= window, "dd_sstv_runs: need 1 <= threshold <= window");
    DD_REQUIRE(count_host != nullptr, "dd_sstv_runs: count");
    *count_host = 0;
    if (n == 0 || n < window) return DD_OK;
    DD_REQUIRE(cls != nullptr && (cap == 0 || pos != nullptr), "dd_sstv_runs: null buffer");
    hipStream_t s = dd_stream(stream);
    const int64_t m = n - window + 1;
    const size_t bP = dd_up16(((size_t)n + 1) * 4), bQ = dd_up16(((size_t)m + 1) * 4), bM = dd_up16((size_t)m),
                 bB = dd_up16(((size_t)n / DD_SSTV_SCAN + 2) * 4);
    DDScratchLock scr;
    int rc = scr.get(bP + bQ + bM + bB, s);
    if (rc != DD_OK) return rc;
    int* P = (int*)scr.ptr;
    int* Q = (int*)(scr.ptr + bP);
    int8_t* mask = (int8_t*)(scr.ptr + bP + bQ);
    int* bsum = (int*)(scr.ptr + bP + bQ + bM);
    rc = dd_sstv_scan(cls, n, target, bsum, P, s);
    if (rc != DD_OK) return rc;
    const unsigned g = (unsigned)((m + 255) / 256);
    hipLaunchKernelGGL(k_sstv_run_starts, dim3(g), dim3(256), 0, s, (const int*)P, m, window, (int)thresh, mask);
    DD_LAUNCH_CHECK();
    rc = dd_sstv_scan(mask, m, 1, bsum, Q, s);
    if (rc != DD_OK) return rc;
    int total = 0;
    DD_HIP_CHECK(hipMemcpyAsync(&total, Q + m, sizeof(int), hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    *count_host = total;
    const int64_t kept = total < cap ? total : cap;
    if (kept > 0) {
        hipLaunchKernelGGL(k_sstv_run_list, dim3(g), dim3(256), 0, s, (const int8_t*)mask, (const int*)Q, m, pos, kept);
        DD_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sstv_run_peak, dim3((unsigned)kept), dim3(64), 0, s, (const int*)P, m, window, (int)thresh, pos);
        DD_LAUNCH_CHECK();
    }
    DD_REQUIRE(total <= cap, "dd_sstv_runs: position list too small");
    return DD_OK;
}

extern "C" int dd_sstv_pixels(const void* d, int64_t n, const double* t0, int64_t nseg, int W, double step, double c1, uint8_t* levels,
                              int64_t* empty_host, void* stream) {
    DD_REQUIRE(n >= 0 && nseg >= 0 && nseg <= 0x7FFFFFFFLL && W >= 0 && W <= 65536, "dd_sstv_pixels: sizes");
    DD_REQUIRE(step > 0.0 && step <= 65536.0 && c1 > 0.0 && c1 <= 1e12, "dd_sstv_pixels: step or rate");     // (false for a NaN)
    DD_REQUIRE(empty_host != nullptr, "dd_sstv_pixels: count");
    *empty_host = 0;
    if (nseg == 0 || W == 0) return DD_OK;
    DD_REQUIRE(t0 != nullptr && levels != nullptr && (n == 0 || d != nullptr), "dd_sstv_pixels: null buffer");
    hipStream_t s = dd_stream(stream);
    DDScratchLock scr;
    int rc = scr.get(16, s);
    if (rc != DD_OK) return rc;
    DD_HIP_CHECK(hipMemsetAsync(scr.ptr, 0, 16, s));
    DDSstvPix prm;
    prm.step = step;
    prm.c1 = c1;
    hipLaunchKernelGGL(k_sstv_pixels, dim3((unsigned)nseg), dim3(64), 0, s, (const double2*)d, n, t0, W, prm, levels,
                       (unsigned long long*)scr.ptr);
    DD_LAUNCH_CHECK();
    unsigned long long none = 0;
    DD_HIP_CHECK(hipMemcpyAsync(&none, scr.ptr, sizeof(none), hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    *empty_host = (int64_t)none;
    return DD_OK;
}

extern "C" int dd_sstv_color(const uint8_t* levels, int64_t npairs, int W, uint8_t* rgb, void* stream) {
    DD_REQUIRE(npairs >= 0 && W >= 0 && W <= 65536 && npairs <= (1LL << 40), "dd_sstv_color: sizes");
    if (npairs == 0 || W == 0) return DD_OK;
    DD_REQUIRE(levels != nullptr && rgb != nullptr, "dd_sstv_color: null buffer");
    hipLaunchKernelGGL(k_sstv_color, dim3((unsigned)((npairs * W + 255) / 256)), dim3(256), 0, dd_stream(stream), levels, npairs, W, rgb);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
