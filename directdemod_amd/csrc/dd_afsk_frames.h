// AFSK1200 frame logic behind the correlators (decode_afsk1200.getMsg :160-269, peakdetect.peakdetect, framechecksequence.fcs_crc16):
// the lookahead peak detector, the bit slicer (bit_repeated, per-bit means, NRZI, start flags, stuffing marks) and the per-flag-pair
// frame check and byte packing.  Part of dd_afsk.hip (included at its end; fp contract off there).  Internal; not a stand-alone header.
//
// Exactness: the peak walk reproduces the reference's state machine (strict updates, lookahead confirmation, mode switch, dump of the
// first hit) for finite input; non-finite input is rejected.  The per-bit means use NumPy's own summation order for a contiguous
// float64 slice of at most 128 elements (a plain loop below 8, else eight partial sums combined pairwise, then the remainder), so the
// means -- and every bit decision taken from them -- are bit for bit the reference's.
#include <vector>

#define DD_PD_CHUNKS 4                      // 64-sample chunks a lane holds per load of the peak walk

// ---------------------------------------------------------------- lookahead extrema W[i] = max / min y[i .. i+L-1] (van Herk / Gil-Werman)
// Blocks of L samples: pmx / pmn the running extrema from the block's start, smx / smn from its end; W[i] = ext(s*[i], p*[i+L-1]).
__global__ void __launch_bounds__(256) k_pd_blocks(const double* __restrict__ y, int64_t n, int64_t L, double* __restrict__ pmx,
                                                   double* __restrict__ pmn, double* __restrict__ smx, double* __restrict__ smn,
                                                   int* __restrict__ bad) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t a = b * L;
    if (a >= n) return;
    const int64_t e = (a + L < n) ? a + L : n;
    double mx = y[a], mn = mx;
    int nonfinite = 0;
    for (int64_t i = a; i < e; ++i) {
        const double v = y[i];
        nonfinite |= !isfinite(v);
        mx = fmax(mx, v);
        mn = fmin(mn, v);
        pmx[i] = mx;
        pmn[i] = mn;
    }
    mx = y[e - 1];
    mn = mx;
    for (int64_t i = e - 1; i >= a; --i) {
        const double v = y[i];
        mx = fmax(mx, v);
        mn = fmin(mn, v);
        smx[i] = mx;
        smn[i] = mn;
    }
    if (nonfinite) atomicOr(bad, 1);
}

// in place: smx[i] <- max y[i .. i+L-1], smn[i] <- min, for i < m = n - L (every such window lies inside y)
__global__ void __launch_bounds__(256) k_pd_window(const double* __restrict__ pmx, const double* __restrict__ pmn, double* __restrict__ smx,
                                                   double* __restrict__ smn, int64_t m, int64_t L) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    smx[i] = fmax(smx[i], pmx[i + L - 1]);
    smn[i] = fmin(smn[i], pmn[i + L - 1]);
}

__device__ __forceinline__ double dd_wave_incl_max(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, d, 64);
        if (lane >= d) v = fmax(v, o);
    }
    return v;
}
__device__ __forceinline__ double dd_wave_incl_min(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, d, 64);
        if (lane >= d) v = fmin(v, o);
    }
    return v;
}

// ---------------------------------------------------------------- the peak walk: one wave, 64 samples per step
// mode 0: both candidates live (before the first confirmation, whose hit the reference pops), 1: looking for a maximum, 2: a minimum.
// A step takes the running extremum of the lanes from `start` on (carried in from the last step), finds the first lane that
// confirms, records it and restarts behind it in the other mode; confirmations are at least one sample apart, so a step costs
// O(1) wave operations plus O(1) per confirmation, whatever the input's plateaus.
struct DDPdOut {
    int64_t* max_pos; double* max_val; int64_t cap_max;
    int64_t* min_pos; double* min_val; int64_t cap_min;
    int64_t* counts;                        // [0] maxima, [1] minima (after the pop)
};

__global__ void __launch_bounds__(64) k_pd_walk(const double* __restrict__ y, const double* __restrict__ wmx, const double* __restrict__ wmn,
                                                int64_t m, double delta, DDPdOut o) {
    const int lane = threadIdx.x;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    int mode = 0;
    double cmx = -inf, cmn = inf;           // carried running extrema (fresh: -inf / +inf) and their first positions
    int64_t cmxpos = -1, cmnpos = -1;
    int64_t nmax = 0, nmin = 0;
    double ny[DD_PD_CHUNKS], na[DD_PD_CHUNKS], nb[DD_PD_CHUNKS];
#pragma unroll
    for (int k = 0; k < DD_PD_CHUNKS; ++k) {
        const int64_t i = (int64_t)k * 64 + lane;
        ny[k] = i < m ? y[i] : 0.0;
        na[k] = i < m ? wmx[i] : 0.0;
        nb[k] = i < m ? wmn[i] : 0.0;
    }
    for (int64_t base = 0; base < m; base += 64 * DD_PD_CHUNKS) {
        double cy[DD_PD_CHUNKS], ca[DD_PD_CHUNKS], cb[DD_PD_CHUNKS];
#pragma unroll
        for (int k = 0; k < DD_PD_CHUNKS; ++k) { cy[k] = ny[k]; ca[k] = na[k]; cb[k] = nb[k]; }
        const int64_t nxt = base + 64 * DD_PD_CHUNKS;
#pragma unroll
        for (int k = 0; k < DD_PD_CHUNKS; ++k) {          // prefetch the next step's samples while this one walks
            const int64_t i = nxt + (int64_t)k * 64 + lane;
            ny[k] = i < m ? y[i] : 0.0;
            na[k] = i < m ? wmx[i] : 0.0;
            nb[k] = i < m ? wmn[i] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < DD_PD_CHUNKS; ++k) {
            const int64_t p = base + (int64_t)k * 64;
            if (p >= m) break;
            const double v = cy[k], a = ca[k], b = cb[k];
            const bool valid = p + lane < m;
            int start = 0;
            while (start < 64) {
                const bool act = valid && lane >= start;
                double mx = -inf, mn = inf;
                bool cmax = false, cmin = false;
                if (mode != 2) {
                    mx = fmax(cmx, dd_wave_incl_max(act ? v : -inf, lane));
                    cmax = act && (v < mx - delta) && (a < mx);
                }
                if (mode != 1) {
                    mn = fmin(cmn, dd_wave_incl_min(act ? v : inf, lane));
                    cmin = act && (v > mn + delta) && (b > mn);
                }
                const unsigned long long hit = __ballot(cmax || cmin);
                if (hit == 0ull) {                         // no confirmation in this chunk: carry the running extrema on
                    if (mode != 2) {
                        const double t = __shfl(mx, 63, 64);
                        if (t > cmx) {
                            const unsigned long long at = __ballot(act && v == t);
                            cmxpos = p + (__ffsll((long long)at) - 1);
                            cmx = t;
                        }
                    }
                    if (mode != 1) {
                        const double t = __shfl(mn, 63, 64);
                        if (t < cmn) {
                            const unsigned long long at = __ballot(act && v == t);
                            cmnpos = p + (__ffsll((long long)at) - 1);
                            cmn = t;
                        }
                    }
                    break;
                }
                const int c = __ffsll((long long)hit) - 1;
                const bool ismax = (__ballot(cmax) >> c) & 1ull;       // the reference checks for a maximum first
                const double t = __shfl(ismax ? mx : mn, c, 64);
                const double carried = ismax ? cmx : cmn;
                int64_t pos;
                if (carried == t) {
                    pos = ismax ? cmxpos : cmnpos;                      // strict updates: the earlier position keeps a tie
                } else {
                    const unsigned long long at = __ballot(act && lane <= c && v == t);
                    pos = p + (__ffsll((long long)at) - 1);
                }
                if (mode != 0 && lane == 0) {                           // mode 0's hit is the one the reference pops (`dump`)
                    if (ismax) {
                        if (nmax < o.cap_max) { o.max_pos[nmax] = pos; o.max_val[nmax] = t; }
                    } else {
                        if (nmin < o.cap_min) { o.min_pos[nmin] = pos; o.min_val[nmin] = t; }
                    }
                }
                if (mode != 0) {
                    if (ismax) ++nmax; else ++nmin;
                }
                mode = ismax ? 2 : 1;
                cmx = -inf; cmn = inf;
                cmxpos = cmnpos = -1;
                start = c + 1;
            }
        }
    }
    if (lane == 0) { o.counts[0] = nmax; o.counts[1] = nmin; }
}

extern "C" int dd_peakdetect_f64(const double* y, int64_t n, int64_t lookahead, double delta, int64_t* max_pos, double* max_val,
                                 int64_t cap_max, int64_t* min_pos, double* min_val, int64_t cap_min, int64_t* counts_host, void* stream) {
    DD_REQUIRE(n >= 0 && lookahead >= 1 && delta >= 0.0 && cap_max >= 0 && cap_min >= 0 && counts_host, "dd_peakdetect_f64: arguments");
    counts_host[0] = counts_host[1] = 0;
    const int64_t m = n - lookahead;                   // the reference walks x_axis[:-lookahead]
    if (m <= 0) return DD_OK;
    DD_REQUIRE(y != nullptr, "dd_peakdetect_f64: null input");
    DD_REQUIRE((cap_max == 0 || (max_pos && max_val)) && (cap_min == 0 || (min_pos && min_val)), "dd_peakdetect_f64: null output");
    hipStream_t s = dd_stream(stream);
    DDScratchLock scr;
    const size_t nn = (size_t)n;
    int rc = scr.get(4 * nn * sizeof(double) + 64, s);
    if (rc != DD_OK) return rc;
    double* pmx = (double*)scr.ptr;
    double* pmn = pmx + nn;
    double* smx = pmn + nn;
    double* smn = smx + nn;
    int64_t* dcounts = (int64_t*)(smn + nn);
    int* bad = (int*)(dcounts + 2);
    DD_HIP_CHECK(hipMemsetAsync(dcounts, 0, 64, s));
    const int64_t nblk = (n + lookahead - 1) / lookahead;
    hipLaunchKernelGGL(k_pd_blocks, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, s, y, n, lookahead, pmx, pmn, smx, smn, bad);
    DD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pd_window, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, pmx, pmn, smx, smn, m, lookahead);
    DD_LAUNCH_CHECK();
    DDPdOut o{max_pos, max_val, cap_max, min_pos, min_val, cap_min, dcounts};
    hipLaunchKernelGGL(k_pd_walk, dim3(1), dim3(64), 0, s, y, smx, smn, m, delta, o);
    DD_LAUNCH_CHECK();
    int64_t h[3] = {0, 0, 0};
    DD_HIP_CHECK(hipMemcpyAsync(h, dcounts, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    DD_REQUIRE((int)h[2] == 0, "dd_peakdetect_f64: non-finite input");
    counts_host[0] = h[0];
    counts_host[1] = h[1];
    DD_REQUIRE(h[0] <= cap_max && h[1] <= cap_min, "dd_peakdetect_f64: output lists too small");
    return DD_OK;
}

// ---------------------------------------------------------------- ordered scans and compaction (one workgroup; the lists are short)
// out[i] = sum_{j<i} v[j] for i < count, *total = the sum
__global__ void __launch_bounds__(1024) k_afsk_excl_scan(const int64_t* __restrict__ v, int64_t count, int64_t* __restrict__ out,
                                                         int64_t* __restrict__ total) {
    __shared__ int64_t part[1024];
    int64_t carry = 0;
    for (int64_t base = 0; base < count; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const int64_t x = i < count ? v[i] : 0;
        part[threadIdx.x] = x;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int64_t o = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += o;
            __syncthreads();
        }
        if (i < count) out[i] = carry + part[threadIdx.x] - x;
        carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// positions k < count with mask[k] != 0, in order, into out[0 .. cap); *total = how many there are
__global__ void __launch_bounds__(1024) k_afsk_compact(const int8_t* __restrict__ mask, int64_t count, int64_t* __restrict__ out,
                                                       int64_t cap, int64_t* __restrict__ total) {
    __shared__ int part[1024];
    int64_t carry = 0;
    for (int64_t base = 0; base < count; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const int x = (i < count && mask[i]) ? 1 : 0;
        part[threadIdx.x] = x;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int o = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += o;
            __syncthreads();
        }
        const int64_t at = carry + part[threadIdx.x] - x;
        if (x && at < cap) out[at] = i;
        carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// ---------------------------------------------------------------- bit slicing (:189-206)
// bit_repeated[i] = np.round(np.diff(peaks1_x)[i] / (bw / 1200)) -- a true division, rounded half to even
__global__ void __launch_bounds__(256) k_afsk_repeats(const int64_t* __restrict__ px, int64_t m1, double q, int64_t* __restrict__ rep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m1) return;
    const double r = rint(__ddiv_rn((double)(px[i + 1] - px[i]), q));
    rep[i] = r > 0.0 ? (int64_t)r : 0;                   // range(int(r)) is empty for r <= 0
}

// np.add.reduce over a contiguous float64 slice of at most 128 elements, in NumPy's order (pairwise_sum below its block size)
__device__ __forceinline__ double dd_np_sum(const double* __restrict__ x, int64_t n) {
    if (n < 8) {
        double r = 0.0;
        for (int64_t i = 0; i < n; ++i) r = __dadd_rn(r, x[i]);
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = x[j];
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = __dadd_rn(r[j], x[i + j]);
    }
    double res = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), __dadd_rn(r[2], r[3])), __dadd_rn(__dadd_rn(r[4], r[5]), __dadd_rn(r[6], r[7])));
    for (; i < n; ++i) res = __dadd_rn(res, x[i]);
    return res;
}

// bit t: interval i (offs[i] <= t < offs[i] + rep[i]), repeat r = t - offs[i]; mean of bf[x_i + r spb : x_i + (r+1) spb] (Python slice
// semantics: clipped to n; an empty slice gives NaN, as np.mean does).  sgn: np.sign of the mean, NaN as 2.
__global__ void __launch_bounds__(256) k_afsk_means(const double* __restrict__ bf, int64_t n, const int64_t* __restrict__ px,
                                                    const int64_t* __restrict__ offs, int64_t m1, int64_t nbits, int spb,
                                                    double* __restrict__ mean, int8_t* __restrict__ sgn) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nbits) return;
    int64_t lo = 0, hi = m1 - 1;                        // last i with offs[i] <= t (offs is non-decreasing, offs[0] = 0)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (offs[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int64_t r = t - offs[lo];
    int64_t a = px[lo] + r * spb, e = a + spb;
    a = a < 0 ? 0 : (a < n ? a : n);                   // (positions outside [0, n) are the caller's error; clamped, never read)
    e = e < a ? a : (e < n ? e : n);
    const int64_t len = e > a ? e - a : 0;
    double v;
    if (len == 0) v = __longlong_as_double(0x7ff8000000000000ll);
    else v = __ddiv_rn(dd_np_sum(bf + a, len), (double)len);
    mean[t] = v;
    sgn[t] = (v != v) ? 2 : (int8_t)((v > 0.0) - (v < 0.0));
}

// decode_nrzi (:208): bit 0 is 1; bit k is 1 where sign[k-1] == sign[k] (an IEEE compare: NaN equals nothing)
__global__ void __launch_bounds__(256) k_afsk_nrzi(const int8_t* __restrict__ sgn, int64_t nbits, int8_t* __restrict__ bits) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nbits) return;
    if (k == 0) { bits[0] = 1; return; }
    const int8_t a = sgn[k - 1], b = sgn[k];
    bits[k] = (a == b && a != 2) ? 1 : 0;
}

// start flags (:217-224: `01111110` at every bit < nbits - 8) and find_bit_stuffing: bit k is marked 1 (bit 0) or 2 (bit 1) when the
// run of ones immediately before it is exactly 5 long
__global__ void __launch_bounds__(256) k_afsk_flags_marks(const int8_t* __restrict__ bits, int64_t nbits, int8_t* __restrict__ flag,
                                                          int8_t* __restrict__ mark) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nbits) return;
    bool f = k < nbits - 8;
    if (f) {
        f = bits[k] == 0 && bits[k + 7] == 0;
        for (int j = 1; j < 7 && f; ++j) f = bits[k + j] == 1;
    }
    flag[k] = f ? 1 : 0;
    int8_t mk = 0;
    if (k >= 5) {
        bool run = true;
        for (int j = 1; j <= 5 && run; ++j) run = bits[k - j] == 1;
        if (run && (k == 5 || bits[k - 6] == 0)) mk = bits[k] == 1 ? 2 : 1;
    }
    mark[k] = mk;
}

extern "C" int dd_afsk_bits_f64(const double* bf, int64_t n, const int64_t* peaks, int64_t m, double bw, int spb, int64_t cap_bits,
                                double* mean, int8_t* sgn, int8_t* bits, int8_t* marks, int64_t* flags, int64_t cap_flags,
                                int64_t* counts_host, void* stream) {
    DD_REQUIRE(n >= 0 && m >= 0 && cap_bits >= 0 && cap_flags >= 0 && counts_host, "dd_afsk_bits_f64: arguments");
    DD_REQUIRE(spb >= 1 && spb <= DD_AFSK_MAX_BS && bw >= 1200.0, "dd_afsk_bits_f64: need 1 <= bw // 1200 <= 64");
    counts_host[0] = counts_host[1] = 0;
    if (m < 2) return DD_OK;
    DD_REQUIRE(bf && peaks, "dd_afsk_bits_f64: null input");
    hipStream_t s = dd_stream(stream);
    const int64_t m1 = m - 1;
    DDScratchLock scr;
    int rc = scr.get(2 * (size_t)m1 * sizeof(int64_t) + 64 + (size_t)cap_bits + 64, s);
    if (rc != DD_OK) return rc;
    int64_t* rep = (int64_t*)scr.ptr;
    int64_t* offs = rep + m1;
    int64_t* tot = offs + m1;                          // [0] bits, [1] flags
    int8_t* fmask = (int8_t*)(tot + 8);
    const double q = bw / 1200.0;                      // self.__bw / self.__BAUDRATE
    hipLaunchKernelGGL(k_afsk_repeats, dim3((unsigned)((m1 + 255) / 256)), dim3(256), 0, s, peaks, m1, q, rep);
    DD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_afsk_excl_scan, dim3(1), dim3(1024), 0, s, rep, m1, offs, tot);
    DD_LAUNCH_CHECK();
    int64_t nb = 0;
    DD_HIP_CHECK(hipMemcpyAsync(&nb, tot, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    counts_host[0] = nb;
    DD_REQUIRE(nb <= cap_bits, "dd_afsk_bits_f64: bit buffers too small");
    if (nb == 0) return DD_OK;
    DD_REQUIRE(mean && sgn && bits && marks && (cap_flags == 0 || flags), "dd_afsk_bits_f64: null output");
    const unsigned g = (unsigned)((nb + 255) / 256);
    hipLaunchKernelGGL(k_afsk_means, dim3(g), dim3(256), 0, s, bf, n, peaks, offs, m1, nb, spb, mean, sgn);
    DD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_afsk_nrzi, dim3(g), dim3(256), 0, s, sgn, nb, bits);
    DD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_afsk_flags_marks, dim3(g), dim3(256), 0, s, bits, nb, fmask, marks);
    DD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_afsk_compact, dim3(1), dim3(1024), 0, s, fmask, nb, flags, cap_flags, tot + 1);
    DD_LAUNCH_CHECK();
    int64_t nf = 0;
    DD_HIP_CHECK(hipMemcpyAsync(&nf, tot + 1, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    counts_host[1] = nf;
    DD_REQUIRE(nf <= cap_flags, "dd_afsk_bits_f64: flag list too small");
    return DD_OK;
}

// ---------------------------------------------------------------- frames (:236-269): one wave per consecutive flag pair
// The pair's unstuffed bits are bits[f+8 : f_next] where marks == 0, kept in order by ballot and prefix count.  The CRC runs
// bit-serially on wave-uniform values over all of them, FCS included: for CRC-16/X.25 (reflected 0x8408, init and xorout 0xFFFF,
// FCS sent LSB first) the register then ends at 0xF0B8 exactly when the last 16 bits are the FCS of the others (for a fixed
// message register, the 16 trailing bits map one-to-one onto the final register).
#define DD_AX25_RESIDUE 0xF0B8u

__global__ void __launch_bounds__(64) k_afsk_frame_check(const int8_t* __restrict__ bits, const int8_t* __restrict__ marks,
                                                         const int64_t* __restrict__ flags, int64_t* __restrict__ info) {
    const int64_t f = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t a = flags[f] + 8, b = flags[f + 1];
    unsigned crc = 0xFFFFu;
    int64_t nb = 0;
    for (int64_t base = a; base < b; base += 64) {
        const int64_t k = base + lane;
        const bool in = k < b;
        const bool keep = in && marks[k] == 0;
        const bool one = keep && bits[k] == 1;
        unsigned long long km = __ballot(keep);
        const unsigned long long vm = __ballot(one);
        nb += __popcll(km);
        while (km) {
            const int j = __ffsll((long long)km) - 1;
            const unsigned bit = (unsigned)((vm >> j) & 1ull);
            const unsigned sh = crc & 1u;
            crc >>= 1;
            if (sh != bit) crc ^= 0x8408u;
            km &= km - 1ull;
        }
    }
    if (lane == 0) {
        const bool ok = nb % 8 == 0 && nb - 16 > 128 && crc == DD_AX25_RESIDUE;
        info[2 * f] = nb;
        info[2 * f + 1] = ok ? 1 : 0;
    }
}

// accepted pair f: its first nb - 16 unstuffed bits, LSB first, into bytes out[off[f] ...] (out zeroed, 4-byte words)
__global__ void __launch_bounds__(64) k_afsk_frame_pack(const int8_t* __restrict__ bits, const int8_t* __restrict__ marks,
                                                        const int64_t* __restrict__ flags, const int64_t* __restrict__ off,
                                                        const int64_t* __restrict__ info, unsigned* __restrict__ out) {
    const int64_t f = blockIdx.x;
    const int64_t o = off[f];
    if (o < 0) return;
    const int lane = threadIdx.x;
    const int64_t a = flags[f] + 8, b = flags[f + 1];
    const int64_t nmsg = info[2 * f] - 16;
    const unsigned long long below = lane ? ((1ull << lane) - 1ull) : 0ull;
    int64_t u0 = 0;
    for (int64_t base = a; base < b; base += 64) {
        const int64_t k = base + lane;
        const bool in = k < b;
        const bool keep = in && marks[k] == 0;
        const unsigned long long km = __ballot(keep);
        const int64_t u = u0 + __popcll(km & below);
        if (keep && u < nmsg && bits[k] == 1) {
            const int64_t bitpos = o * 8 + u;
            atomicOr(out + (bitpos >> 5), 1u << (unsigned)(bitpos & 31));
        }
        u0 += __popcll(km);
    }
}

extern "C" int dd_afsk_frames_check(const int8_t* bits, const int8_t* marks, int64_t nbits, const int64_t* flags, int64_t nflags,
                                    int64_t* info_host, void* stream) {
    DD_REQUIRE(nbits >= 0 && nflags >= 0 && info_host, "dd_afsk_frames_check: arguments");
    if (nflags < 2) return DD_OK;
    DD_REQUIRE(bits && marks && flags, "dd_afsk_frames_check: null buffer");
    hipStream_t s = dd_stream(stream);
    const int64_t np = nflags - 1;
    std::vector<int64_t> fl((size_t)nflags);
    DD_HIP_CHECK(hipMemcpyAsync(fl.data(), flags, sizeof(int64_t) * (size_t)nflags, hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    for (int64_t i = 0; i < nflags; ++i)               // every pair's span lies inside the stream, in order
        DD_REQUIRE(fl[i] >= 0 && fl[i] <= nbits && (i == 0 || fl[i] >= fl[i - 1]), "dd_afsk_frames_check: flag positions");
    DDScratchLock scr;
    int rc = scr.get(2 * (size_t)np * sizeof(int64_t), s);
    if (rc != DD_OK) return rc;
    int64_t* info = (int64_t*)scr.ptr;
    hipLaunchKernelGGL(k_afsk_frame_check, dim3((unsigned)np), dim3(64), 0, s, bits, marks, flags, info);
    DD_LAUNCH_CHECK();
    DD_HIP_CHECK(hipMemcpyAsync(info_host, info, 2 * (size_t)np * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    return DD_OK;
}

extern "C" int dd_afsk_frames_pack(const int8_t* bits, const int8_t* marks, int64_t nbits, const int64_t* flags, int64_t nflags,
                                   const int64_t* info_host, const int64_t* off_host, uint8_t* out, int64_t out_bytes, void* stream) {
    DD_REQUIRE(nbits >= 0 && nflags >= 0 && out_bytes >= 0 && out_bytes % 4 == 0, "dd_afsk_frames_pack: arguments");
    if (nflags < 2) return DD_OK;
    DD_REQUIRE(bits && marks && flags && info_host && off_host && (out_bytes == 0 || out), "dd_afsk_frames_pack: null buffer");
    DD_REQUIRE(((uintptr_t)out & 3) == 0, "dd_afsk_frames_pack: out must be 4-byte aligned");
    hipStream_t s = dd_stream(stream);
    const int64_t np = nflags - 1;
    for (int64_t i = 0; i < np; ++i) {
        if (off_host[i] < 0) continue;
        const int64_t nmsg = info_host[2 * i] - 16;
        DD_REQUIRE(info_host[2 * i + 1] == 1 && nmsg >= 0 && nmsg % 8 == 0 && off_host[i] + nmsg / 8 <= out_bytes,
                   "dd_afsk_frames_pack: offsets must place accepted frames inside out");
    }
    DDScratchLock scr;
    int rc = scr.get(4 * (size_t)np * sizeof(int64_t), s);
    if (rc != DD_OK) return rc;
    int64_t* info = (int64_t*)scr.ptr;
    int64_t* off = info + 2 * np;
    DD_HIP_CHECK(hipMemcpyAsync(info, info_host, 2 * (size_t)np * sizeof(int64_t), hipMemcpyHostToDevice, s));
    DD_HIP_CHECK(hipMemcpyAsync(off, off_host, (size_t)np * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (out_bytes) DD_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)out_bytes, s));
    hipLaunchKernelGGL(k_afsk_frame_pack, dim3((unsigned)np), dim3(64), 0, s, bits, marks, flags, off, info, (unsigned*)out);
    DD_LAUNCH_CHECK();
    DD_HIP_CHECK(hipStreamSynchronize(s));             // the host arrays were pageable sources: done before they go away
    return DD_OK;
}
