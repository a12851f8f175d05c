// APT image extraction (decode_noaa.getImage :255-465, getColor :537-598): the segmented median, the batched line extraction, the
// pixel mapping and the false colour.  One of the parts of dd_audio.hip (included there, after dd_audio_xcorr.h for dd_key_f64 and
// after dd_audio_resample.h for dd_resample_fft_chunks).  Internal; not a stand-alone header.
//
// Medians follow np.median exactly: an odd count gives the middle element, an even count (a + b) / 2 of the two middle ones, an
// empty segment or one holding a NaN gives NaN.  Values are selected by rank, so the result is the same value numpy picks (of two
// equal values -0.0 and +0.0 either sign may come back, as with numpy's partition).
#define DD_APT_PIXELS 1040                 // pixels per half-line (numPixels * 0.5, :296, :346-347)
#define DD_APT_KREG 32                     // per-pixel sample counts up to this are ranked in registers

// ---------------------------------------------------------------- exact median by rank counting (a few values, one lane)
// x[0..k): rank of x[i] is [less, less + equal); the element whose interval holds r is the r-th smallest
__device__ __forceinline__ double dd_rank_pick(const double* __restrict__ x, int64_t k, int64_t r) {
    for (int64_t i = 0; i < k; ++i) {
        const double v = x[i];
        int64_t lt = 0, eq = 0;
        for (int64_t j = 0; j < k; ++j) {
            const double w = x[j];
            lt += w < v;
            eq += w == v;
        }
        if (lt <= r && r < lt + eq) return v;
    }
    return __longlong_as_double(0x7ff8000000000000ll);
}
__device__ __forceinline__ double dd_median_small(const double* __restrict__ x, int64_t k) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (k <= 0) return nan;
    if (k <= DD_APT_KREG) {
        double v[DD_APT_KREG];
        bool bad = false;
#pragma unroll
        for (int i = 0; i < DD_APT_KREG; ++i) {
            v[i] = i < k ? x[i] : 0.0;
            bad |= i < k && v[i] != v[i];
        }
        if (bad) return nan;
        const int r1 = (int)(k / 2), r0 = (k & 1) ? r1 : r1 - 1;
        double lo = nan, hi = nan;
#pragma unroll
        for (int i = 0; i < DD_APT_KREG; ++i) {
            int lt = 0, eq = 0;
#pragma unroll
            for (int j = 0; j < DD_APT_KREG; ++j) {
                lt += (j < k) & (v[j] < v[i]);
                eq += (j < k) & (v[j] == v[i]);
            }
            if (i < k) {
                if (lt <= r0 && r0 < lt + eq) lo = v[i];
                if (lt <= r1 && r1 < lt + eq) hi = v[i];
            }
        }
        return (k & 1) ? hi : (lo + hi) / 2.0;
    }
    for (int64_t i = 0; i < k; ++i)
        if (x[i] != x[i]) return nan;
    const int64_t r1 = k / 2;
    if (k & 1) return dd_rank_pick(x, k, r1);
    return (dd_rank_pick(x, k, r1 - 1) + dd_rank_pick(x, k, r1)) / 2.0;
}

// ---------------------------------------------------------------- segmented median: one workgroup per segment, radix select
// Eight passes over the segment (in global memory: a segment need not fit in LDS), one byte of the order-preserving key each,
// for the two middle ranks at once; the histogram's exclusive scan picks the byte.  Segments of up to DD_APT_KREG values take
// the one-lane path above.
struct DDSeg { int64_t off, len; };

__device__ __forceinline__ double dd_key_to_f64(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// inclusive sum over the 256 lanes of the block; `wsum` is 4 words of LDS
__device__ __forceinline__ unsigned int dd_block_scan256(unsigned int v, unsigned int* wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    unsigned int base = 0;
    for (int i = 0; i < w; ++i) base += wsum[i];
    __syncthreads();
    return v + base;
}

__global__ void __launch_bounds__(256) k_median_segments(const double* __restrict__ src, const DDSeg* __restrict__ segs, double* __restrict__ out) {
    __shared__ unsigned int hist[2][256];
    __shared__ unsigned int wsum[4];
    __shared__ unsigned long long pre[2];
    __shared__ unsigned int rem[2];
    __shared__ int nan_seen;
    const DDSeg sg = segs[blockIdx.x];
    const double* x = src + sg.off;
    const int64_t n = sg.len;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (n <= DD_APT_KREG) {
        if (threadIdx.x == 0) out[blockIdx.x] = dd_median_small(x, n);
        return;
    }
    const int64_t r1 = n / 2, r0 = (n & 1) ? r1 : r1 - 1;
    if (threadIdx.x == 0) {
        pre[0] = pre[1] = 0;
        rem[0] = (unsigned int)r0;
        rem[1] = (unsigned int)r1;
        nan_seen = 0;
    }
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[0][threadIdx.x] = 0;
        hist[1][threadIdx.x] = 0;
        __syncthreads();
        const unsigned long long p0 = pre[0], p1 = pre[1];
        int bad = 0;
        for (int64_t i = threadIdx.x; i < n; i += 256) {
            const double v = x[i];
            if (pass == 0) bad |= v != v;
            const unsigned long long k = dd_key_f64(v);
            const unsigned long long hi = pass ? (k >> (shift + 8)) : 0;
            const unsigned int d = (unsigned int)(k >> shift) & 255u;
            if (hi == p0) atomicAdd(&hist[0][d], 1u);
            if (hi == p1) atomicAdd(&hist[1][d], 1u);
        }
        if (bad) nan_seen = 1;
        __syncthreads();
        if (nan_seen) break;                                   // (uniform: read after the barrier)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned int c = hist[s][threadIdx.x];
            const unsigned int incl = dd_block_scan256(c, wsum);
            const unsigned int r = rem[s];
            __syncthreads();
            if (incl - c <= r && r < incl) {                   // exactly one lane: the byte holding rank r
                pre[s] = ((s ? p1 : p0) << 8) | (unsigned long long)threadIdx.x;
                rem[s] = r - (incl - c);
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        double m;
        if (nan_seen) {
            m = nan;
        } else {
            const double lo = dd_key_to_f64(pre[0]), hi = dd_key_to_f64(pre[1]);
            m = (n & 1) ? hi : (lo + hi) / 2.0;
        }
        out[blockIdx.x] = m;
    }
}

static int apt_upload(DDScratchLock& scr, const void* host, size_t bytes, hipStream_t s, void** dev) {
    const int rc = scr.get(bytes, s);
    if (rc != DD_OK) return rc;
    DD_HIP_CHECK(hipMemcpyAsync(scr.ptr, host, bytes, hipMemcpyHostToDevice, s));       // (pageable source: staged before the call returns)
    *dev = scr.ptr;
    return DD_OK;
}

extern "C" int dd_median_segments_f64(const double* src, const int64_t* off_host, const int64_t* len_host, int count, double* out, void* stream) {
    DD_REQUIRE(count >= 0 && off_host && len_host && out, "arguments");
    if (count == 0) return DD_OK;
    DD_REQUIRE(src, "null source");
    hipStream_t s = dd_stream(stream);
    std::vector<DDSeg> segs(count);
    for (int i = 0; i < count; ++i) {
        DD_REQUIRE(off_host[i] >= 0 && len_host[i] >= 0 && len_host[i] < (1ll << 32), "segment");
        segs[i] = DDSeg{off_host[i], len_host[i]};
    }
    DDScratchLock scr;
    void* d = nullptr;
    const int rc = apt_upload(scr, segs.data(), sizeof(DDSeg) * (size_t)count, s, &d);
    if (rc != DD_OK) return rc;
    hipLaunchKernelGGL(k_median_segments, dim3(count), dim3(256), 0, s, src, (const DDSeg*)d, out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// ---------------------------------------------------------------- line extraction (:330-430)
// Half-line h: its resampled values work[w_off, w_off + 1040 k) (k = num / 1040) reshape to (1040, k); pixel p is the median of
// row p.  A half-line with a sync slot (lo >= 0) also copies the k values of each of its first `nbits` pixels to the low stream
// (sync bit 0) or the high stream (bit 1), pixel after pixel: the concatenation the reference's sync FIFOs keep the tail of.
struct DDAptHalf { int64_t w_off, k, lo, hi; };

__global__ void __launch_bounds__(256) k_apt_pixels(const double* __restrict__ work, const DDAptHalf* __restrict__ halves, double* __restrict__ pix,
                                                    double* __restrict__ stream_out, unsigned long long mask, int nbits) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= DD_APT_PIXELS) return;
    const DDAptHalf h = halves[blockIdx.y];
    const double* x = work + h.w_off + (int64_t)p * h.k;
    pix[(int64_t)blockIdx.y * DD_APT_PIXELS + p] = dd_median_small(x, h.k);
    if (h.lo >= 0 && p < nbits) {
        const bool one = (mask >> p) & 1ull;
        const unsigned long long below = p ? (mask & ((1ull << p) - 1ull)) : 0ull;
        const int ones = __popcll(below), rank = one ? ones : p - ones;
        double* dst = stream_out + (one ? h.hi : h.lo) + (int64_t)rank * h.k;
        for (int64_t j = 0; j < h.k; ++j) dst[j] = x[j];
    }
}

extern "C" int dd_apt_lines_f64(const double* env, int64_t n_env, const int64_t* start_host, const int64_t* len_host, int nhalf,
                                const int64_t* sync_off_host, uint64_t sync_mask, int sync_bits, double* work, double* pix,
                                double* sync_stream, void* stream) {
    DD_REQUIRE(nhalf >= 0 && start_host && len_host && sync_off_host, "arguments");
    DD_REQUIRE(sync_bits >= 0 && sync_bits <= 64 && sync_bits <= DD_APT_PIXELS, "sync bits");
    if (nhalf == 0) return DD_OK;
    DD_REQUIRE(env && pix, "null buffer");
    hipStream_t s = dd_stream(stream);
    std::vector<DDAptHalf> hv(nhalf);
    std::vector<int64_t> r_in, r_n, r_out, r_num;
    int64_t w = 0;
    for (int h = 0; h < nhalf; ++h) {
        const int64_t a = start_host[h], n = len_host[h];
        DD_REQUIRE(a >= 0 && n >= 0 && a + n <= n_env, "half-line outside the envelope");
        const int64_t num = (n / DD_APT_PIXELS) * DD_APT_PIXELS;
        const int64_t lo = sync_off_host[2 * h], hi = sync_off_host[2 * h + 1];
        DD_REQUIRE(lo < 0 || (sync_stream && hi >= 0), "sync slot");
        hv[h] = DDAptHalf{w, num / DD_APT_PIXELS, lo, hi};
        if (num > 0) {
            r_in.push_back(a);
            r_n.push_back(n);
            r_out.push_back(w);
            r_num.push_back(num);
        }
        w += num;
    }
    DD_REQUIRE(w == 0 || work, "null work buffer");
    if (!r_in.empty()) {
        const int rc = dd_resample_fft_chunks(env, 0, r_in.data(), r_n.data(), work, r_out.data(), r_num.data(), (int)r_in.size(), stream);
        if (rc != DD_OK) return rc;
    }
    DDScratchLock scr;
    void* d = nullptr;
    const int rc = apt_upload(scr, hv.data(), sizeof(DDAptHalf) * (size_t)nhalf, s, &d);
    if (rc != DD_OK) return rc;
    hipLaunchKernelGGL(k_apt_pixels, dim3((DD_APT_PIXELS + 255) / 256, nhalf), dim3(256), 0, s, (const double*)work, (const DDAptHalf*)d, pix,
                       sync_stream, (unsigned long long)sync_mask, sync_bits);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// ---------------------------------------------------------------- mapping (:436-455) and false colour (:537-598)
// numpy's operation order, no contraction into fused multiply-adds, np.round = round half to even (rint)
__device__ __forceinline__ unsigned char dd_apt_clip_u8(double v) {
    if (v < 0.0) v = 0.0;
    if (v > 255.0) v = 255.0;
    return v == v ? (unsigned char)(int)v : (unsigned char)0;        // (NaN: numpy's cast is undefined; any value)
}

__global__ void __launch_bounds__(256) k_apt_map(const double* __restrict__ pix, int64_t nrows, int row_len, const double* __restrict__ par,
                                                 unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows * row_len) return;
    const int64_t r = i / row_len;
    const double x = pix[i], a = par[3 * r + 1], b = par[3 * r + 2];
    double v;
    if (par[3 * r] == 0.0) {
        v = x - a;                       // round(255 * (x - low) / (high - low))
        v = 255.0 * v;
        v = v / (b - a);
    } else {
        v = x * a;                       // round(x * slope + intercept)
        v = v + b;
    }
    out[i] = dd_apt_clip_u8(rint(v));
}

extern "C" int dd_apt_map_u8(const double* pix, int64_t nrows, int row_len, const double* par_host, uint8_t* out, void* stream) {
    DD_REQUIRE(nrows >= 0 && row_len >= 0 && par_host, "arguments");
    if (nrows == 0 || row_len == 0) return DD_OK;
    DD_REQUIRE(pix && out, "null buffer");
    hipStream_t s = dd_stream(stream);
    DDScratchLock scr;
    void* d = nullptr;
    const int rc = apt_upload(scr, par_host, sizeof(double) * 3 * (size_t)nrows, s, &d);
    if (rc != DD_OK) return rc;
    const int64_t n = nrows * row_len;
    hipLaunchKernelGGL(k_apt_map, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pix, nrows, row_len, (const double*)d, out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// colorsys.hsv_to_rgb, then int(k * 255.0), then np.uint8 of the int array (modulo 256)
__device__ __forceinline__ unsigned char dd_apt_chan(double k) {
#pragma clang fp contract(off)
    const double y = k * 255.0;
    return (unsigned char)((long long)y & 255ll);
}

__global__ void __launch_bounds__(256) k_apt_color(const unsigned char* __restrict__ img, int64_t nrows, int row_len, unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows * DD_APT_PIXELS) return;
    const int64_t r = i / DD_APT_PIXELS, c = i - r * DD_APT_PIXELS;
    const double v = (double)img[r * row_len + c], t = (double)img[r * row_len + DD_APT_PIXELS + c];
    const double tempLimit = 155.0, seaLimit = 30.0, landLimit = 90.0;
    double minH, minS, minV, maxH, maxS, maxV, sv, st;
    if (t < tempLimit) {                 // clouds
        minH = 230 / 360.0; minS = 0.2; minV = 0.3; maxH = 230 / 360.0; maxS = 0.0; maxV = 1.0;
        sv = v / 256.0;
        st = (256.0 - t) / 256.0;
    } else if (v < seaLimit) {           // sea
        minH = 200.0 / 360.0; minS = 0.7; minV = 0.6; maxH = 240.0 / 360.0; maxS = 0.6; maxV = 0.4;
        sv = v / seaLimit;
        st = (256.0 - t) / (256.0 - tempLimit);
    } else {                             // ground
        minH = 60.0 / 360.0; minS = 0.6; minV = 0.2; maxH = 100.0 / 360.0; maxS = 0.0; maxV = 0.5;
        sv = (v - seaLimit) / (landLimit - seaLimit);
        st = (256.0 - t) / (256.0 - tempLimit);
    }
    const double fs = maxS + st * (minS - maxS);
    const double fv = maxV + sv * (minV - maxV);
    const double fh = maxH + sv * st * (minH - maxH);
    double R, G, B;
    if (fs == 0.0) {
        R = G = B = fv;
    } else {
        const double h6 = fh * 6.0;
        long long ii = (long long)h6;                   // int(): truncation toward zero
        const double f = h6 - (double)ii;
        const double p = fv * (1.0 - fs);
        const double q = fv * (1.0 - fs * f);
        const double tt = fv * (1.0 - fs * (1.0 - f));
        ii = ((ii % 6) + 6) % 6;                        // Python's modulo
        switch (ii) {
            case 0: R = fv; G = tt; B = p; break;
            case 1: R = q; G = fv; B = p; break;
            case 2: R = p; G = fv; B = tt; break;
            case 3: R = p; G = q; B = fv; break;
            case 4: R = tt; G = p; B = fv; break;
            default: R = fv; G = p; B = q; break;
        }
    }
    out[3 * i] = dd_apt_chan(R);
    out[3 * i + 1] = dd_apt_chan(G);
    out[3 * i + 2] = dd_apt_chan(B);
}

extern "C" int dd_apt_color_u8(const uint8_t* img, int64_t nrows, int row_len, uint8_t* out, void* stream) {
    DD_REQUIRE(nrows >= 0 && row_len >= 2 * DD_APT_PIXELS, "arguments");
    if (nrows == 0) return DD_OK;
    DD_REQUIRE(img && out, "null buffer");
    const int64_t n = nrows * DD_APT_PIXELS;
    hipLaunchKernelGGL(k_apt_color, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dd_stream(stream), img, nrows, row_len, out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
