// Meteor-M2 QPSK sync detection (the reference's decode_meteorm2.getSyncs, decode_meteorm2.py:229-324), included by dd_afsk.hip
// after dd_symbol_walk.h, which holds the walk's state and parameters, its body, agc.adjust, costas.loop, hyp, lim, the run skipping
// and the mixer's rotation (built with -ffp-contract=off: every float64 operation is the reference's, in its
// order, rounded on its own).  Here: the QPSK policy of the walk, the sync scoring, the block-sum correlation and the mixer.
//
//   k_meteor_mix      -- the reference's float64 mixer (offsetFreq), rounded to complex64 as there
//   k_meteor_walk     -- dd_sym_walk with agc.adjust's cap of 200 and the QPSK cross-term error
//   k_meteor_lim      -- lim(real(x * out) / 2), lim(imag(x * out) / 2) per sample, out = the Costas phasor active at that sample
//   k_meteor_bits     -- limBin(real), limBin(imag) of each corrected symbol
//   k_meteor_minsync  -- the two 120-bit sync scores over contiguous symbol windows; symbols where either fires are candidates
//   k_meteor_maxcorr  -- |np.correlate(buffer, template, 'same')| and its first argmax, one workgroup per correlation buffer
#pragma once

#define DD_MET_SYNC 120               // sync bits
#define DD_MET_REP 28                 // int(2048000 / 72000): template samples per sync bit
#define DD_MET_TLEN (DD_MET_SYNC * DD_MET_REP)
#define DD_MET_MAXL 20480             // longest correlation buffer (entries): 2 * (3360 + 6721) = 20162 occur
#define DD_MET_WN (DD_MET_MAXL + DD_MET_TLEN - DD_MET_REP)

struct DDMeteorSync {
    uint64_t s0[2], s1[2];            // sync72khz and sync72khz1, bit i of the 120 in word i / 64
};

struct DDMeteorTemplates {
    signed char t[2][DD_MET_SYNC];    // sync2mhz and sync2mhz2 before np.repeat: 127 / -128 per bit
};

struct DDMeteorBuf {                  // a correlation buffer: samples [lo0, lo0 + n0) then [lo1, lo1 + n1), two entries each
    int64_t lo0, n0, lo1, n1, tmpl;
};
static_assert(sizeof(DDMeteorBuf) == 5 * sizeof(int64_t), "dd_sym_with_descriptors uploads five words per buffer");

// decode_meteorm2's agc.adjust cap and costas.loop error (decode_meteorm2.py:29, :63)
struct DDMeteorQpsk {
    static constexpr int CAP = 200;
    static __device__ __forceinline__ double error(double cr, double ci, const double* __restrict__ tbl) {
        return (ci * dd_met_hyp(cr, tbl) - cr * dd_met_hyp(ci, tbl)) / 255.0;
    }
};

__global__ void __launch_bounds__(128) k_meteor_walk(const double2* __restrict__ x, int64_t n, int64_t base, DDMeteorState* __restrict__ stp,
                                                      const DDMeteorParams prm, int64_t cap, int64_t* __restrict__ bidx,
                                                      int64_t* __restrict__ aidx, double2* __restrict__ agc, double2* __restrict__ ph,
                                                      double2* __restrict__ sym, double2* __restrict__ pf) {
    dd_sym_walk<DDMeteorQpsk>(x, n, base, stp, prm, cap, bidx, aidx, agc, ph, sym, pf);
}

// sample base + j takes the phasor of the last costas.loop before it: ph[c - 1] with c = #{k : aidx[k] < base + j}, 1 before any
__global__ void __launch_bounds__(256) k_meteor_lim(const double2* __restrict__ x, int64_t n, int64_t base, const int64_t* __restrict__ aidx,
                                                     int64_t nsym, const double2* __restrict__ ph, char2* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int64_t s = base + j;
    int64_t lo = 0, hi = nsym;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (aidx[mid] < s) lo = mid + 1;
        else hi = mid;
    }
    const double2 o = lo == 0 ? make_double2(1.0, -0.0) : ph[lo - 1];
    const double2 v = x[j];
    const double re = v.x * o.x - v.y * o.y, im = v.x * o.y + v.y * o.x;
    out[s] = make_char2((signed char)dd_met_lim(re / 2.0), (signed char)dd_met_lim(im / 2.0));
}

__global__ void __launch_bounds__(256) k_meteor_bits(const double2* __restrict__ sym, int64_t nsym, uint8_t* __restrict__ bits) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nsym) return;
    const double2 v = sym[k];
    bits[k] = (uint8_t)((!(v.x <= 0.0) ? 1 : 0) | (!(v.y <= 0.0) ? 2 : 0));       // limBin
}

__device__ __forceinline__ int dd_met_bit(const uint64_t* w, int i) { return (int)((w[i >> 6] >> (i & 63)) & 1); }

// window of symbols k-59 .. k: minResBuff1 = (re, im) bits against sync72khz, minResBuff2 = (im, re) bits against sync72khz1;
// cand[3c .. 3c+2] = (k, mismatches1, mismatches2) where |mismatches - 60| > 30 for either
__global__ void __launch_bounds__(256) k_meteor_minsync(const uint8_t* __restrict__ bits, int64_t nsym, const DDMeteorSync sy,
                                                         int64_t cap, int64_t* __restrict__ cand, unsigned long long* __restrict__ count) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nsym || k < DD_MET_SYNC / 2 - 1) return;
    int m1 = 0, m2 = 0;
    for (int t = 0; t < DD_MET_SYNC / 2; ++t) {
        const int b = bits[k - (DD_MET_SYNC / 2 - 1) + t];
        const int re = b & 1, im = b >> 1;
        m1 += (re != dd_met_bit(sy.s0, 2 * t)) + (im != dd_met_bit(sy.s0, 2 * t + 1));
        m2 += (im != dd_met_bit(sy.s1, 2 * t)) + (re != dd_met_bit(sy.s1, 2 * t + 1));
    }
    if (abs(m1 - DD_MET_SYNC / 2) > 30 || abs(m2 - DD_MET_SYNC / 2) > 30) {
        const unsigned long long c = atomicAdd(count, 1ull);
        if ((int64_t)c < cap) {
            cand[3 * c] = k;
            cand[3 * c + 1] = m1;
            cand[3 * c + 2] = m2;
        }
    }
}

__device__ __forceinline__ int dd_met_entry(const char2* __restrict__ lim, const DDMeteorBuf& b, int64_t e) {
    const int64_t smp = e >> 1;
    const int64_t idx = smp < b.n0 ? b.lo0 + smp : b.lo1 + (smp - b.n0);
    const char2 v = lim[idx];
    return (e & 1) ? v.y : v.x;
}

// np.correlate(buf, np.repeat(t, 28), 'same')[i] = sum_j buf[i - 1680 + j] * tmpl[j] = sum_b t[b] * W[i + 28 b], with
// W[q] = sum_{u < 28} buf[q - 1680 + u] (zero outside the buffer): 120 terms per lag, exact in int32 (|c| < 3360 * 128^2)
__global__ void __launch_bounds__(256) k_meteor_maxcorr(const char2* __restrict__ lim, const DDMeteorBuf* __restrict__ bufs,
                                                         const DDMeteorTemplates T, int64_t* __restrict__ out) {
    __shared__ short W[DD_MET_WN];
    __shared__ int rv[256];
    __shared__ int ri[256];
    const DDMeteorBuf b = bufs[blockIdx.x];
    const int L = (int)(2 * (b.n0 + b.n1));
    const int nw = L + DD_MET_TLEN - DD_MET_REP;
    const int tid = threadIdx.x;
    for (int q = tid; q < nw; q += 256) {
        int acc = 0;
        const int e0 = q - DD_MET_TLEN / 2;
        for (int u = 0; u < DD_MET_REP; ++u) {
            const int e = e0 + u;
            if (e >= 0 && e < L) acc += dd_met_entry(lim, b, e);
        }
        W[q] = (short)acc;
    }
    __syncthreads();
    const signed char* t = T.t[b.tmpl ? 1 : 0];
    int best = -1, bi = 0;
    for (int i = tid; i < L; i += 256) {
        int c = 0;
        for (int k = 0; k < DD_MET_SYNC; ++k) c += (int)t[k] * (int)W[i + DD_MET_REP * k];
        c = abs(c);
        if (c > best) { best = c; bi = i; }
    }
    dd_sym_first_max<256>(best, bi, rv, ri, out);
}

// commSignal.offsetFreq as the reference computes it (comm.py:77 there): x (complex64) *= np.exp(-1.0j*2.0*np.pi*f*np.arange(n)/fs),
// i.e. theta = (w * k) * (1 / fs) with w = -2 pi f (NumPy's complex products with zero parts and Smith's division by the real fs),
// the product in float64, rounded to complex64.  Input: raw u8 pairs (x = u8 - 127.5, exact in float32) or complex64.
__global__ void __launch_bounds__(256) k_meteor_mix(const uchar2* __restrict__ raw, const float2* __restrict__ c64, int64_t n, double w,
                                                     double inv_fs, float2* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const float2 x = dd_met_sample(raw, c64, k);
    out[k] = dd_met_rotate(x, (w * (double)k) * inv_fs);
}

extern "C" int dd_meteor_mix(const void* raw_u8, const void* c64, int64_t n, double w, double inv_fs, void* out, void* stream) {
    DD_REQUIRE(n >= 0, "dd_meteor_mix: sizes");
    if (n == 0) return DD_OK;
    DD_REQUIRE((raw_u8 != nullptr) != (c64 != nullptr) && out != nullptr, "dd_meteor_mix: one input and an output");
    hipLaunchKernelGGL(k_meteor_mix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dd_stream(stream), (const uchar2*)raw_u8,
                       (const float2*)c64, n, w, inv_fs, (float2*)out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_meteor_walk(const void* x, int64_t n, int64_t base, void* state, const double* params_host, int64_t cap,
                              int64_t* bidx, int64_t* aidx, void* agc, void* ph, void* sym, void* pf, void* stream) {
    return dd_sym_walk_launch(k_meteor_walk, "dd_meteor_walk", x, n, base, state, params_host, cap, bidx, aidx, agc, ph, sym, pf, stream);
}

extern "C" int dd_meteor_lim(const void* x, int64_t n, int64_t base, const int64_t* aidx, int64_t nsym, const void* ph, void* out,
                             int64_t out_len, void* stream) {
    DD_REQUIRE(n >= 0 && base >= 0 && nsym >= 0 && base + n <= out_len, "dd_meteor_lim: sizes");
    if (n == 0) return DD_OK;
    DD_REQUIRE(x != nullptr && out != nullptr && (nsym == 0 || (aidx != nullptr && ph != nullptr)), "dd_meteor_lim: null buffer");
    hipLaunchKernelGGL(k_meteor_lim, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dd_stream(stream), (const double2*)x, n, base,
                       aidx, nsym, (const double2*)ph, (char2*)out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_meteor_minsync(const void* sym, int64_t nsym, const uint8_t* sync_bits_host, uint8_t* bits, int64_t cap,
                                 int64_t* cand, unsigned long long* count, void* stream) {
    DD_REQUIRE(nsym >= 0 && cap >= 0 && sync_bits_host != nullptr, "dd_meteor_minsync: sizes");
    if (nsym == 0) return DD_OK;
    DD_REQUIRE(sym != nullptr && bits != nullptr && cand != nullptr && count != nullptr, "dd_meteor_minsync: null buffer");
    DDMeteorSync sy;
    memset(&sy, 0, sizeof(sy));
    for (int i = 0; i < DD_MET_SYNC; ++i) {
        if (sync_bits_host[i]) sy.s0[i >> 6] |= 1ull << (i & 63);
        if (sync_bits_host[DD_MET_SYNC + i]) sy.s1[i >> 6] |= 1ull << (i & 63);
    }
    const dim3 g((unsigned)((nsym + 255) / 256));
    hipLaunchKernelGGL(k_meteor_bits, g, dim3(256), 0, dd_stream(stream), (const double2*)sym, nsym, bits);
    DD_LAUNCH_CHECK();
    DD_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned long long), dd_stream(stream)));
    hipLaunchKernelGGL(k_meteor_minsync, g, dim3(256), 0, dd_stream(stream), (const uint8_t*)bits, nsym, sy, cap, cand, count);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_meteor_maxcorr(const void* lim, int64_t lim_len, const int64_t* bufs_host, int64_t nbuf, const int8_t* templates_host,
                                 int64_t* out, void* stream) {
    DD_REQUIRE(nbuf >= 0 && templates_host != nullptr, "dd_meteor_maxcorr: sizes");
    if (nbuf == 0) return DD_OK;
    DD_REQUIRE(lim != nullptr && bufs_host != nullptr && out != nullptr, "dd_meteor_maxcorr: null buffer");
    for (int64_t i = 0; i < nbuf; ++i) {
        const int64_t* d = bufs_host + 5 * i;
        const int64_t L = 2 * (d[1] + d[3]);
        DD_REQUIRE(d[1] >= 0 && d[3] >= 0 && L >= DD_MET_TLEN && L <= DD_MET_MAXL, "dd_meteor_maxcorr: buffer length");
        DD_REQUIRE(d[0] >= 0 && d[0] + d[1] <= lim_len && d[2] >= 0 && d[2] + d[3] <= lim_len, "dd_meteor_maxcorr: buffer outside the samples");
    }
    DDMeteorTemplates T;
    memcpy(T.t, templates_host, sizeof(T.t));
    return dd_sym_with_descriptors(bufs_host, nbuf, "dd_meteor_maxcorr", stream, [&](void* dbufs) {
        hipLaunchKernelGGL(k_meteor_maxcorr, dim3((unsigned)nbuf), dim3(256), 0, dd_stream(stream), (const char2*)lim,
                           (const DDMeteorBuf*)dbufs, T, out);
    });
}
