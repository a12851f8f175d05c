// Funcube BPSK sync detection (the reference's decode_funcube.getSyncs, decode_funcube.py:148-306), included by dd_afsk.hip after
// dd_symbol_walk.h, which holds the walk's state and parameters, its body, agc.adjust, costas.loop, hyp, lim, the run skipping and the
// mixer's rotation (built with -ffp-contract=off: every float64 operation is the reference's, in its order,
// rounded on its own).  Here: the BPSK policy of the walk, the low-pass, the ramp mixer, the sync scoring and the prefix-sum
// correlation.
//
//   k_funcube_mix_ramp -- the reference's float64 mixer with the frequency ramp of decode_funcube.py:215-226 formed per sample
//   k_funcube_lowpass  -- scipy.signal.lfilter's recurrence sample by sample in its own operation order: bit for bit its output
//   k_funcube_walk     -- dd_sym_walk with agc.adjust's cap of 20 and the BPSK error imag * hyp(real) / 255
//   k_funcube_lim      -- lim(real(x * out) / 2) per sample, out = the Costas phasor active at that sample
//   k_funcube_minsync  -- limBin(real) per symbol and the 330-bit sync score of every full window; firing symbols are compacted
//   k_funcube_maxcorr  -- |np.correlate(buffer, np.repeat(template, rep), 'same')| and its first argmax from a prefix sum of the
//                         buffer kept in device scratch, one workgroup per correlation buffer
#pragma once

#define DD_FC_SYNC 33                 // sync bits
#define DD_FC_SYMS 10                 // symbols per sync bit at 12000 symbols/s
#define DD_FC_WIN (DD_FC_SYNC * DD_FC_SYMS)
#define DD_FC_CORR_THREADS 1024

struct DDFuncubeBuf {                 // a correlation buffer: samples [lo0, lo0 + n0) then [lo1, lo1 + n1); its n0 + n1 + 1 prefix sums
    int64_t lo0, n0, lo1, n1, scratch;    // start at scratch[scratch]
};
static_assert(sizeof(DDFuncubeBuf) == 5 * sizeof(int64_t), "dd_sym_with_descriptors uploads five words per buffer");

#define DD_FC_IIR_N 7                 // coefficients of butter(fs, bw)'s sixth-order low-pass
#define DD_FC_IIR_TILE 1024

struct DDFuncubeIir {
    double b[DD_FC_IIR_N], a[DD_FC_IIR_N];
};

// sig.filter(bf) (decode_funcube.py:230 -> scipy.signal.lfilter, complex64 in, complex128 out): the transposed direct form II
//   y = z0 + b0 x;  z_k = (z_{k+1} + b_{k+1} x) - a_{k+1} y;  z_5 = b_6 x - a_6 y
// per real component, every product and sum rounded on its own in lfilter's order (its complex products with the real coefficients
// add only zeros), so the output and the carried state are lfilter's bit for bit.  The block-parallel dd_iir_c64 is 5.6e-6 off at
// the 7 kHz default -- enough to move Gardner decisions -- so this walk, like the symbol walk, is serial: one
// wave stages tiles through LDS (the next tile in flight), lane 0 runs the real parts and lane 1 the imaginary parts.
__global__ void __launch_bounds__(64) k_funcube_lowpass(const float2* __restrict__ in, double2* __restrict__ out, int64_t n, const DDFuncubeIir C,
                                                        double* __restrict__ state) {
    constexpr int R = DD_FC_IIR_TILE / 64, N = DD_FC_IIR_N;
    __shared__ float2 tin[DD_FC_IIR_TILE];
    __shared__ double2 tout[DD_FC_IIR_TILE];
    const int lane = threadIdx.x;
    double z[N - 1];
#pragma unroll
    for (int k = 0; k < N - 1; ++k) z[k] = lane < 2 ? state[lane * (N - 1) + k] : 0.0;
    float2 pre[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = (int64_t)r * 64 + lane;
        pre[r] = i < n ? in[i] : make_float2(0.0f, 0.0f);
    }
    const int64_t ntiles = (n + DD_FC_IIR_TILE - 1) / DD_FC_IIR_TILE;
    for (int64_t it = 0; it < ntiles; ++it) {
        const int64_t t0 = it * DD_FC_IIR_TILE;
#pragma unroll
        for (int r = 0; r < R; ++r) tin[r * 64 + lane] = pre[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = t0 + DD_FC_IIR_TILE + (int64_t)r * 64 + lane;
            if (i < n) pre[r] = in[i];
        }
        if (lane < 2) {
            const int m = (int)min((int64_t)DD_FC_IIR_TILE, n - t0);
            const float* xs = (const float*)tin;
            double* ys = (double*)tout;
            for (int j = 0; j < m; ++j) {
                const double x = (double)xs[2 * j + lane];
                const double y = z[0] + C.b[0] * x;
#pragma unroll
                for (int k = 0; k < N - 2; ++k) z[k] = (z[k + 1] + C.b[k + 1] * x) - C.a[k + 1] * y;
                z[N - 2] = C.b[N - 1] * x - C.a[N - 1] * y;
                ys[2 * j + lane] = y;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = t0 + (int64_t)r * 64 + lane;
            if (i < n) out[i] = tout[r * 64 + lane];
        }
        __syncthreads();
    }
    if (lane < 2) {
#pragma unroll
        for (int k = 0; k < N - 1; ++k) state[lane * (N - 1) + k] = z[k];
    }
}

// decode_funcube's agc.adjust cap and costas.loop error (decode_funcube.py:30, :65)
struct DDFuncubeBpsk {
    static constexpr int CAP = 20;
    static __device__ __forceinline__ double error(double cr, double ci, const double* __restrict__ tbl) {
        return ci * dd_met_hyp(cr, tbl) / 255.0;
    }
};

__global__ void __launch_bounds__(128) k_funcube_walk(const double2* __restrict__ x, int64_t n, int64_t base, DDMeteorState* __restrict__ stp,
                                                       const DDMeteorParams prm, int64_t cap, int64_t* __restrict__ bidx,
                                                       int64_t* __restrict__ aidx, double2* __restrict__ agc, double2* __restrict__ ph,
                                                       double2* __restrict__ sym, double2* __restrict__ pf) {
    dd_sym_walk<DDFuncubeBpsk>(x, n, base, stp, prm, cap, bidx, aidx, agc, ph, sym, pf);
}

// sample base + j takes pllObj.output as the loop before it left it -- costas.loop sets it on entry, so it is the phasor the last
// symbol was corrected with: ph[c - 1] with c = #{k : aidx[k] < base + j} (the reference's ctr at that sample), 1 before any
__global__ void __launch_bounds__(256) k_funcube_lim(const double2* __restrict__ x, int64_t n, int64_t base, const int64_t* __restrict__ aidx,
                                                      int64_t nsym, const double2* __restrict__ ph, signed char* __restrict__ out) {
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
    out[s] = (signed char)dd_met_lim((v.x * o.x - v.y * o.y) / 2.0);
}

__global__ void __launch_bounds__(256) k_funcube_bits(const double2* __restrict__ sym, int64_t nsym, uint8_t* __restrict__ bits) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nsym) return;
    bits[k] = (uint8_t)(!(sym[k].x <= 0.0) ? 1 : 0);                    // limBin
}

// window of symbols k-329 .. k against sync12khz (each sync bit ten times): cand[2c], cand[2c+1] = (k, mismatches) where
// |mismatches - 165| > 120 -- either polarity
__global__ void __launch_bounds__(256) k_funcube_minsync(const uint8_t* __restrict__ bits, int64_t nsym, uint64_t sync, int64_t cap,
                                                          int64_t* __restrict__ cand, unsigned long long* __restrict__ count) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nsym || k < DD_FC_WIN - 1) return;
    const uint8_t* w = bits + (k - (DD_FC_WIN - 1));
    int m = 0;
    for (int b = 0; b < DD_FC_SYNC; ++b) {
        const int want = (int)((sync >> b) & 1);
        for (int u = 0; u < DD_FC_SYMS; ++u) m += (int)w[b * DD_FC_SYMS + u] != want;
    }
    if (abs(m - DD_FC_WIN / 2) > 120) {
        const unsigned long long c = atomicAdd(count, 1ull);
        if ((int64_t)c < cap) {
            cand[2 * c] = k;
            cand[2 * c + 1] = m;
        }
    }
}

__device__ __forceinline__ int dd_fc_entry(const signed char* __restrict__ lim, const DDFuncubeBuf& b, int64_t e) {
    return lim[e < b.n0 ? b.lo0 + e : b.lo1 + (e - b.n0)];
}

// np.correlate(buf, np.repeat(t, rep), 'same')[i] = sum_j buf[i - (33 rep) / 2 + j] * tmpl[j] = sum_b t[b] * (S[e_b + rep] - S[e_b]),
// e_b = i - (33 rep) / 2 + rep b, S[q] = the sum of the buffer's first q entries (q clamped to 0 .. L: zero outside the buffer):
// 34 prefix sums per lag.  |S| <= 128 L fits int32 for L < 2^24 (checked by the host); a lag's sum is below 33 * 128 * 128 rep.
__global__ void __launch_bounds__(DD_FC_CORR_THREADS) k_funcube_maxcorr(const signed char* __restrict__ lim, const DDFuncubeBuf* __restrict__ bufs,
                                                                         uint64_t sync, int rep, int* __restrict__ scratch,
                                                                         int64_t* __restrict__ out) {
    __shared__ int part[DD_FC_CORR_THREADS];
    __shared__ long long rv[DD_FC_CORR_THREADS];
    __shared__ int ri[DD_FC_CORR_THREADS];
    const DDFuncubeBuf b = bufs[blockIdx.x];
    const int L = (int)(b.n0 + b.n1);
    int* __restrict__ S = scratch + b.scratch;
    const int tid = threadIdx.x;
    const int per = (L + DD_FC_CORR_THREADS - 1) / DD_FC_CORR_THREADS;
    const int e0 = min(tid * per, L), e1 = min(e0 + per, L);
    int acc = 0;
    for (int e = e0; e < e1; ++e) acc += dd_fc_entry(lim, b, e);
    part[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < DD_FC_CORR_THREADS; ++i) {
            const int v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    acc = part[tid];
    for (int e = e0; e < e1; ++e) {
        S[e] = acc;
        acc += dd_fc_entry(lim, b, e);
    }
    if (e1 == L && e0 < L) S[L] = acc;
    if (L == 0 && tid == 0) S[0] = 0;
    __threadfence_block();
    __syncthreads();
    const int left = (DD_FC_SYNC * rep) / 2;
    long long best = -1;
    int bi = 0;
    for (int i = tid; i < L; i += DD_FC_CORR_THREADS) {
        long long c = 0;
        int prev = S[min(max(i - left, 0), L)];
        for (int k = 0; k < DD_FC_SYNC; ++k) {
            const int nxt = S[min(max(i - left + rep * (k + 1), 0), L)];
            c += (long long)(((sync >> k) & 1) ? 127 : -128) * (long long)(nxt - prev);
            prev = nxt;
        }
        if (c < 0) c = -c;
        if (c > best) { best = c; bi = i; }
    }
    dd_sym_first_max<DD_FC_CORR_THREADS>(best, bi, rv, ri, out);
}

// commSignal.offsetFreq with decode_funcube.py:215-226's frequency array: x (complex64) *= np.exp(-1.0j*2.0*np.pi*f*np.arange(n)/fs),
// theta = ((w * f[k]) * k) * (1 / fs) with w = -2 pi, f[k] = f0 + k * delta as np.arange fills it (a product and a sum, each rounded),
// clipped to the target from above when rising and from below when falling.  A constant f gives dd_meteor_mix's bits.
__global__ void __launch_bounds__(256) k_funcube_mix_ramp(const uchar2* __restrict__ raw, const float2* __restrict__ c64, int64_t n, double w,
                                                           double f0, double delta, double target, double inv_fs, float2* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    double f = f0 + (double)k * delta;
    if (target > f0 ? f > target : f < target) f = target;
    out[k] = dd_met_rotate(dd_met_sample(raw, c64, k), ((w * f) * (double)k) * inv_fs);
}

extern "C" int dd_funcube_mix_ramp(const void* raw_u8, const void* c64, int64_t n, double w, double f0, double delta, double target,
                                   double inv_fs, void* out, void* stream) {
    DD_REQUIRE(n >= 0, "dd_funcube_mix_ramp: sizes");
    if (n == 0) return DD_OK;
    DD_REQUIRE((raw_u8 != nullptr) != (c64 != nullptr) && out != nullptr, "dd_funcube_mix_ramp: one input and an output");
    hipLaunchKernelGGL(k_funcube_mix_ramp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dd_stream(stream), (const uchar2*)raw_u8,
                       (const float2*)c64, n, w, f0, delta, target, inv_fs, (float2*)out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_funcube_lowpass(const void* in_c64, void* out_c128, int64_t n, const double* b_host, const double* a_host, int ncoef,
                                  double* state, void* stream) {
    DD_REQUIRE(n >= 0 && b_host != nullptr && a_host != nullptr && state != nullptr, "dd_funcube_lowpass: arguments");
    DD_REQUIRE(ncoef == DD_FC_IIR_N && a_host[0] == 1.0, "dd_funcube_lowpass: seven coefficients with a[0] = 1 (butter's sixth order)");
    if (n == 0) return DD_OK;
    DD_REQUIRE(in_c64 != nullptr && out_c128 != nullptr && in_c64 != (const void*)out_c128, "dd_funcube_lowpass: buffers");
    DDFuncubeIir C;
    for (int k = 0; k < DD_FC_IIR_N; ++k) {
        C.b[k] = b_host[k];
        C.a[k] = a_host[k];
    }
    hipLaunchKernelGGL(k_funcube_lowpass, dim3(1), dim3(64), 0, dd_stream(stream), (const float2*)in_c64, (double2*)out_c128, n, C, state);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_funcube_walk(const void* x, int64_t n, int64_t base, void* state, const double* params_host, int64_t cap,
                               int64_t* bidx, int64_t* aidx, void* agc, void* ph, void* sym, void* pf, void* stream) {
    return dd_sym_walk_launch(k_funcube_walk, "dd_funcube_walk", x, n, base, state, params_host, cap, bidx, aidx, agc, ph, sym, pf, stream);
}

extern "C" int dd_funcube_lim(const void* x, int64_t n, int64_t base, const int64_t* aidx, int64_t nsym, const void* ph, int8_t* out,
                              int64_t out_len, void* stream) {
    DD_REQUIRE(n >= 0 && base >= 0 && nsym >= 0 && base + n <= out_len, "dd_funcube_lim: sizes");
    if (n == 0) return DD_OK;
    DD_REQUIRE(x != nullptr && out != nullptr && (nsym == 0 || (aidx != nullptr && ph != nullptr)), "dd_funcube_lim: null buffer");
    hipLaunchKernelGGL(k_funcube_lim, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dd_stream(stream), (const double2*)x, n, base,
                       aidx, nsym, (const double2*)ph, (signed char*)out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

static uint64_t dd_fc_sync_word(const uint8_t* sync_bits_host) {
    uint64_t w = 0;
    for (int i = 0; i < DD_FC_SYNC; ++i)
        if (sync_bits_host[i]) w |= 1ull << i;
    return w;
}

extern "C" int dd_funcube_minsync(const void* sym, int64_t nsym, const uint8_t* sync_bits_host, uint8_t* bits, int64_t cap,
                                  int64_t* cand, unsigned long long* count, void* stream) {
    DD_REQUIRE(nsym >= 0 && cap >= 0 && sync_bits_host != nullptr, "dd_funcube_minsync: sizes");
    if (nsym == 0) return DD_OK;
    DD_REQUIRE(sym != nullptr && bits != nullptr && cand != nullptr && count != nullptr, "dd_funcube_minsync: null buffer");
    const dim3 g((unsigned)((nsym + 255) / 256));
    hipLaunchKernelGGL(k_funcube_bits, g, dim3(256), 0, dd_stream(stream), (const double2*)sym, nsym, bits);
    DD_LAUNCH_CHECK();
    DD_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned long long), dd_stream(stream)));
    hipLaunchKernelGGL(k_funcube_minsync, g, dim3(256), 0, dd_stream(stream), (const uint8_t*)bits, nsym, dd_fc_sync_word(sync_bits_host),
                       cap, cand, count);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_funcube_maxcorr(const int8_t* lim, int64_t lim_len, const int64_t* bufs_host, int64_t nbuf, const uint8_t* sync_bits_host,
                                  int rep, int32_t* scratch, int64_t scratch_len, int64_t* out, void* stream) {
    DD_REQUIRE(nbuf >= 0 && sync_bits_host != nullptr && rep >= 1 && rep <= 65536, "dd_funcube_maxcorr: sizes");
    if (nbuf == 0) return DD_OK;
    DD_REQUIRE(lim != nullptr && bufs_host != nullptr && scratch != nullptr && out != nullptr, "dd_funcube_maxcorr: null buffer");
    for (int64_t i = 0; i < nbuf; ++i) {
        const int64_t* d = bufs_host + 5 * i;
        DD_REQUIRE(d[1] >= 0 && d[3] >= 0 && d[1] + d[3] >= 1 && d[1] + d[3] < (1 << 24), "dd_funcube_maxcorr: buffer length");
        DD_REQUIRE(d[0] >= 0 && d[0] + d[1] <= lim_len && d[2] >= 0 && d[2] + d[3] <= lim_len, "dd_funcube_maxcorr: buffer outside the samples");
        DD_REQUIRE(d[4] >= 0 && d[4] + d[1] + d[3] + 1 <= scratch_len, "dd_funcube_maxcorr: prefix sums outside the scratch");
        for (int64_t j = 0; j < i; ++j) {
            const int64_t* o = bufs_host + 5 * j;
            DD_REQUIRE(d[4] + d[1] + d[3] + 1 <= o[4] || o[4] + o[1] + o[3] + 1 <= d[4], "dd_funcube_maxcorr: overlapping scratch");
        }
    }
    return dd_sym_with_descriptors(bufs_host, nbuf, "dd_funcube_maxcorr", stream, [&](void* dbufs) {
        hipLaunchKernelGGL(k_funcube_maxcorr, dim3((unsigned)nbuf), dim3(DD_FC_CORR_THREADS), 0, dd_stream(stream), (const signed char*)lim,
                           (const DDFuncubeBuf*)dbufs, dd_fc_sync_word(sync_bits_host), rep, (int*)scratch, out);
    });
}
