// FM stereo audio from the multiplex of a broadcast station: the 19 kHz pilot, L - R on the suppressed 38 kHz subcarrier and the
// de-emphasis (beyond the reference; DESIGN.md section 4.29 defines every stage, fmstereo.py restates each kernel in NumPy), included by
// dd_afsk.hip after dd_rds.h, whose quantiser dd_rds_q and 1024-entry phasor table it uses.  The multiplex is the FM discriminator's
// float64 output in radians per sample; everything behind the quantiser is integer, so sums in any order equal the restatement bit for
// bit.  Floor divisions are built from the truncating one, shifts of negative numbers are arithmetic.
//
//   k_fms_pilot    -- a wave per block of 256 samples: four products q * table[phase19] per lane in int64, a wave sum, the sum >> 10
//                     as an int32 pair P
//   k_fms_carrier  -- a thread per block: S = (the sum of P over the 17 blocks around it that exist) >> 8, the lock decision
//                     |S|^2 >= thr cnt^2 and the 38 kHz correction u = -S^2 / |S|^2 in Q14 by two int64 floor divisions
//   k_fms_audio    -- a workgroup stages the two mixed signals a = q (2^14 + c2) >> 8 and b = q (2^14 - c2) >> 8 of 256 outputs and
//                     the taps' reach in LDS, each sample mixed once; a thread per output pair runs the decimating FIR over both.  The
//                     sums stay below 2^41, so they are exact in 64-bit integer multiply-adds and in float64 fused multiply-adds
//                     alike: the kernel is built for both routes (profiles/fmstereo.txt: they take the same time)
//   k_fms_mix      -- (a diagnostic) a and b of every sample, before the FIR
#pragma once

#define DD_FMS_B 256                  // samples per pilot block (mirrored by fmstereo.B)
#define DD_FMS_W 8                    // blocks summed to either side of a block for the carrier
#define DD_FMS_PILOT_SHIFT 10         // |q| <= 2^15, |table| <= 2^14, 256 products: |sum| <= 2^37, |P| <= 2^27
#define DD_FMS_CARRIER_SHIFT 8        // 17 blocks: |sum| <= 17 * 2^27, |S| <= 17 * 2^19 < 2^24 per component
#define DD_FMS_Q 14                   // u and the mixer's factor are Q14
#define DD_FMS_GAIN_SHIFT 12          // G = rint(2 g 4096)
#define DD_FMS_G_MAX 12288            // g <= 1.5
#define DD_FMS_MIX_SHIFT 8
#define DD_FMS_OUT_SHIFT 15           // the taps are rint(2^15 h)
#define DD_FMS_TILE 256               // output pairs per workgroup
#define DD_FMS_D_MAX 12               // multiplex samples per audio sample at most (500 000 / 48 000 gives 10)
#define DD_FMS_TAPS_MAX 1024
#define DD_FMS_SPAN ((DD_FMS_TILE - 1) * DD_FMS_D_MAX + DD_FMS_TAPS_MAX)      // samples a tile reads at most
#define DD_FMS_PAD(j) ((j) + ((j) >> 5))                                      // one spare word per 32: lanes D apart meet no bank twice
#define DD_FMS_THR_MAX (1LL << 48)

// the bit budget (section 4.29): |S|^2 <= 2 * (17 * 2^19)^2 < 2^48, << 14 < 2^62 and thr cnt^2 <= 2^48 * 289 < 2^57;
// |u| <= 2^14 per component and |table| <= 2^14 with |u| |table| <= (2^14 + 2)^2, so |c| <= 2^14 + 4, |c2| <= (2^14 + 4) * 12288 >> 12
// <= 3 * 2^14 + 12, |a|, |b| <= 2^15 (2^16 + 12) >> 8 = 2^23 + 1536 < 2^24; with the sum of |taps| <= 2^17 the FIR's sums stay below
// 2^41 and the outputs below 2^26
static_assert(2LL * (17LL << 19) * (17LL << 19) < (1LL << 48), "|S|^2 below 2^48: the Q14 numerators fit int64");
static_assert(DD_FMS_THR_MAX * 17 * 17 < (1LL << 57), "thr cnt^2 fits int64");
static_assert((((1LL << 14) + 4) * DD_FMS_G_MAX >> DD_FMS_GAIN_SHIFT) <= 3 * (1LL << 14) + 12, "|c2| at g = 1.5");
static_assert(((1LL << 15) * ((1LL << 14) + 3 * (1LL << 14) + 12) >> DD_FMS_MIX_SHIFT) < (1LL << 24), "|a|, |b| below 2^24");
static_assert((1LL << 24) * (1LL << 17) < (1LL << 53), "the FIR's sums are exact in float64 as in int64");
static_assert(4 * 2 * (DD_FMS_SPAN + DD_FMS_SPAN / 32 + 2) + 8 * DD_FMS_TAPS_MAX <= 65536, "a workgroup's LDS");

__device__ __forceinline__ int64_t dd_fms_floordiv(int64_t n, int64_t d) {      // d > 0
    const int64_t q = n / d;
    return (n % d != 0 && n < 0) ? q - 1 : q;
}

__device__ __forceinline__ int64_t dd_fms_wave_sum(int64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((long long)v, o);
    return v;
}

// P[k] = (the sum over i < 256 of q[256 k + i] * table[phase19(256 k + i)]) >> 10, phase19(n) = bits 31 .. 22 of n * step19 mod 2^32
__global__ void __launch_bounds__(256) k_fms_pilot(const double* __restrict__ x, int64_t nb, uint64_t step19, const int2* __restrict__ table,
                                                   int2* __restrict__ P) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= nb) return;                                                  // (uniform over the wave)
    int64_t re = 0, im = 0;
    for (int r = 0; r < DD_FMS_B / 64; ++r) {
        const uint64_t n = (uint64_t)k * DD_FMS_B + (uint64_t)(64 * r + lane);
        const int2 w = table[(uint32_t)(n * step19) >> 22];
        const int64_t q = dd_rds_q(x[n]);
        re += q * w.x;
        im += q * w.y;
    }
    re = dd_fms_wave_sum(re);
    im = dd_fms_wave_sum(im);
    if (lane == 0) P[k] = make_int2((int)(re >> DD_FMS_PILOT_SHIFT), (int)(im >> DD_FMS_PILOT_SHIFT));
}

// S[k] = (the sum of P[j], |j - k| <= 8, 0 <= j < nb) >> 8 with cnt[k] summed; lock[k] = |S|^2 > 0 and |S|^2 >= thr cnt^2;
// u[k] = (floor(-((Sr^2 - Si^2) << 14) / |S|^2), floor(-((2 Sr Si) << 14) / |S|^2)) when locked, else (0, 0)
__global__ void __launch_bounds__(256) k_fms_carrier(const int2* __restrict__ P, int64_t nb, int64_t thr, int2* __restrict__ S,
                                                     int2* __restrict__ u, uint8_t* __restrict__ lock) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nb) return;
    const int64_t lo = k - DD_FMS_W < 0 ? 0 : k - DD_FMS_W, hi = k + DD_FMS_W >= nb ? nb - 1 : k + DD_FMS_W;
    int64_t sr = 0, si = 0;
    for (int64_t j = lo; j <= hi; ++j) {
        const int2 p = P[j];
        sr += p.x;
        si += p.y;
    }
    sr >>= DD_FMS_CARRIER_SHIFT;
    si >>= DD_FMS_CARRIER_SHIFT;
    const int64_t cnt = hi - lo + 1, mag = sr * sr + si * si;
    const bool locked = mag > 0 && mag >= thr * cnt * cnt;
    S[k] = make_int2((int)sr, (int)si);
    lock[k] = locked ? 1 : 0;
    u[k] = locked ? make_int2((int)dd_fms_floordiv(-((sr * sr - si * si) << DD_FMS_Q), mag), (int)dd_fms_floordiv(-((2 * sr * si) << DD_FMS_Q), mag))
                  : make_int2(0, 0);
}

// (a, b) of the sample n: q (2^14 + c2) >> 8 and q (2^14 - c2) >> 8 with c = (tr ui + ti ur) >> 14, (tr, ti) = conj(table[phase38(n)]),
// c2 = c G >> 12 and u of the block min(n / 256, nb - 1), (0, 0) without a block; int64 throughout, stored as int32
__device__ __forceinline__ int2 dd_fms_ab(const double* __restrict__ x, int64_t n, uint64_t step38, const int2* __restrict__ table,
                                          const int2* __restrict__ u, int64_t nb, int G) {
    const int64_t q = dd_rds_q(x[n]);
    int64_t c2 = 0;
    if (nb > 0) {
        const int64_t k = n / DD_FMS_B < nb ? n / DD_FMS_B : nb - 1;
        const int2 uk = u[k];
        const int2 t = table[(uint32_t)((uint64_t)n * step38) >> 22];
        const int64_t c = ((int64_t)t.x * uk.y - (int64_t)t.y * uk.x) >> DD_FMS_Q;
        c2 = (c * G) >> DD_FMS_GAIN_SHIFT;
    }
    return make_int2((int)((q * ((1LL << DD_FMS_Q) + c2)) >> DD_FMS_MIX_SHIFT), (int)((q * ((1LL << DD_FMS_Q) - c2)) >> DD_FMS_MIX_SHIFT));
}

__global__ void __launch_bounds__(256) k_fms_mix(const double* __restrict__ x, int64_t n, uint64_t step38, const int2* __restrict__ table,
                                                 const int2* __restrict__ u, int64_t nb, int G, int2* __restrict__ ab) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) ab[i] = dd_fms_ab(x, i, step38, table, u, nb, G);
}

struct DDFmsGrid {
    int64_t n, nb, nout;              // multiplex samples, pilot blocks, output pairs
    uint64_t step38;
    int G, ntaps, D, d0;
};

// out[2 o], out[2 o + 1] = (the sum over i < ntaps of h[i] * a[o D + d0 - i]) >> 15 and the same of b; samples outside the data are 0.
// F64: the products and sums in float64 (exact below 2^53), else in int64.
template <bool F64>
__global__ void __launch_bounds__(DD_FMS_TILE) k_fms_audio(const double* __restrict__ x, const DDFmsGrid gd, const int2* __restrict__ table,
                                                           const int2* __restrict__ u, const int* __restrict__ taps, int2* __restrict__ out) {
    __shared__ int sa[DD_FMS_SPAN + DD_FMS_SPAN / 32 + 2];
    __shared__ int sb[DD_FMS_SPAN + DD_FMS_SPAN / 32 + 2];
    __shared__ double hs[DD_FMS_TAPS_MAX];                               // the taps: as float64, or as int32 in the same words
    int* hi = reinterpret_cast<int*>(hs);
    const int tid = threadIdx.x;
    const int64_t o0 = (int64_t)blockIdx.x * DD_FMS_TILE;
    const int outs = gd.nout - o0 < DD_FMS_TILE ? (int)(gd.nout - o0) : DD_FMS_TILE;
    const int span = (outs - 1) * gd.D + gd.ntaps;                       // <= DD_FMS_SPAN
    const int64_t first = o0 * gd.D + gd.d0 - (gd.ntaps - 1);            // the sample staged at place 0
    for (int j = tid; j < span; j += DD_FMS_TILE) {
        const int64_t i = first + j;
        const int2 v = (i >= 0 && i < gd.n) ? dd_fms_ab(x, i, gd.step38, table, u, gd.nb, gd.G) : make_int2(0, 0);
        sa[DD_FMS_PAD(j)] = v.x;
        sb[DD_FMS_PAD(j)] = v.y;
    }
    for (int j = tid; j < gd.ntaps; j += DD_FMS_TILE) {
        if (F64) hs[j] = (double)taps[j];
        else hi[j] = taps[j];
    }
    __syncthreads();
    if (tid >= outs) return;
    const int top = tid * gd.D + gd.ntaps - 1;                           // the place of tap 0's sample; tap i reads place top - i >= 0
    int64_t l, r;
    if (F64) {
        double fl = 0.0, fr = 0.0;
        for (int i = 0; i < gd.ntaps; ++i) {
            const int j = top - i;
            const double h = hs[i];
            fl = __builtin_fma(h, (double)sa[DD_FMS_PAD(j)], fl);
            fr = __builtin_fma(h, (double)sb[DD_FMS_PAD(j)], fr);
        }
        l = (int64_t)fl;
        r = (int64_t)fr;
    } else {
        l = 0;
        r = 0;
        for (int i = 0; i < gd.ntaps; ++i) {
            const int j = top - i;
            const int64_t h = hi[i];
            l += h * sa[DD_FMS_PAD(j)];
            r += h * sb[DD_FMS_PAD(j)];
        }
    }
    out[o0 + tid] = make_int2((int)(l >> DD_FMS_OUT_SHIFT), (int)(r >> DD_FMS_OUT_SHIFT));
}

// ---------------------------------------------------------------------------------------------------------------- the C entries
#define DD_FMS_N_MAX 0x7FFFFFF0LL

extern "C" int dd_fms_pilot(const double* mpx, int64_t n, uint64_t step19, const int32_t* table, int32_t* P, void* stream) {
    DD_REQUIRE(n >= 0 && n <= DD_FMS_N_MAX && step19 < (1ULL << 32), "dd_fms_pilot: need 0 <= n < 2^31 and step19 < 2^32");
    const int64_t nb = n / DD_FMS_B;
    if (nb == 0) return DD_OK;
    DD_REQUIRE(mpx != nullptr && table != nullptr && P != nullptr, "dd_fms_pilot: null buffer");
    hipLaunchKernelGGL(k_fms_pilot, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, dd_stream(stream), mpx, nb, step19, (const int2*)table,
                       (int2*)P);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_fms_carrier(const int32_t* P, int64_t nb, int64_t thr, int32_t* S, int32_t* u, uint8_t* lock, void* stream) {
    DD_REQUIRE(nb >= 0 && nb <= DD_FMS_N_MAX / DD_FMS_B && thr >= 0 && thr <= DD_FMS_THR_MAX,
               "dd_fms_carrier: need 0 <= nb < 2^23 and 0 <= thr <= 2^48");
    if (nb == 0) return DD_OK;
    DD_REQUIRE(P != nullptr && S != nullptr && u != nullptr && lock != nullptr, "dd_fms_carrier: null buffer");
    hipLaunchKernelGGL(k_fms_carrier, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, dd_stream(stream), (const int2*)P, nb, thr, (int2*)S,
                       (int2*)u, lock);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// 0 when a size, the gain, the taps or the decimation is not served, else 1 with the grid filled
static int dd_fms_grid(int64_t n, uint64_t step38, int64_t nb, int G, int ntaps, int D, int d0, DDFmsGrid* gd) {
    if (n < 0 || n > DD_FMS_N_MAX || step38 >= (1ULL << 32) || nb < 0 || nb > DD_FMS_N_MAX / DD_FMS_B || G < 0 || G > DD_FMS_G_MAX || ntaps < 1 ||
        ntaps > DD_FMS_TAPS_MAX || D < 1 || D > DD_FMS_D_MAX || d0 < 0 || d0 >= ntaps)
        return 0;
    gd->n = n;
    gd->nb = nb;
    gd->nout = (n + D - 1) / D;
    gd->step38 = step38;
    gd->G = G;
    gd->ntaps = ntaps;
    gd->D = D;
    gd->d0 = d0;
    return 1;
}

static int dd_fms_audio_run(const char* who, bool f64, const double* mpx, const DDFmsGrid& gd, const int32_t* table, const int32_t* u,
                            const int32_t* taps, int32_t* out, void* stream) {
    if (gd.nout == 0) return DD_OK;
    DD_REQUIRE(mpx != nullptr && table != nullptr && (u != nullptr || gd.nb == 0) && taps != nullptr && out != nullptr, who);
    const dim3 grid((unsigned)((gd.nout + DD_FMS_TILE - 1) / DD_FMS_TILE));
    if (f64)
        hipLaunchKernelGGL(k_fms_audio<true>, grid, dim3(DD_FMS_TILE), 0, dd_stream(stream), mpx, gd, (const int2*)table, (const int2*)u, taps,
                           (int2*)out);
    else
        hipLaunchKernelGGL(k_fms_audio<false>, grid, dim3(DD_FMS_TILE), 0, dd_stream(stream), mpx, gd, (const int2*)table, (const int2*)u, taps,
                           (int2*)out);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

#define DD_FMS_AUDIO_F64 false        // the route dd_fms_audio takes: both took 310 us a minute of multiplex (profiles/fmstereo.txt)

extern "C" int dd_fms_audio(const double* mpx, int64_t n, uint64_t step38, const int32_t* table, const int32_t* u, int64_t nb, int G,
                            const int32_t* taps, int ntaps, int D, int d0, int32_t* out, void* stream) {
    DDFmsGrid gd;
    DD_REQUIRE(dd_fms_grid(n, step38, nb, G, ntaps, D, d0, &gd),
               "dd_fms_audio: need 0 <= n < 2^31, step38 < 2^32, 0 <= nb < 2^23, 0 <= G <= 12288, 1 <= ntaps <= 1024, 1 <= D <= 12 and 0 <= d0 < ntaps");
    return dd_fms_audio_run("dd_fms_audio: null buffer", DD_FMS_AUDIO_F64, mpx, gd, table, u, taps, out, stream);
}

extern "C" int dd_debug_fms_audio_route(const double* mpx, int64_t n, uint64_t step38, const int32_t* table, const int32_t* u, int64_t nb, int G,
                                        const int32_t* taps, int ntaps, int D, int d0, int route, int32_t* out, void* stream) {
    DDFmsGrid gd;
    DD_REQUIRE((route == 0 || route == 1) && dd_fms_grid(n, step38, nb, G, ntaps, D, d0, &gd),
               "dd_debug_fms_audio_route: need dd_fms_audio's arguments and route 0 (int64) or 1 (float64)");
    return dd_fms_audio_run("dd_debug_fms_audio_route: null buffer", route == 1, mpx, gd, table, u, taps, out, stream);
}

extern "C" int dd_debug_fms_mix(const double* mpx, int64_t n, uint64_t step38, const int32_t* table, const int32_t* u, int64_t nb, int G,
                                int32_t* ab, void* stream) {
    DDFmsGrid gd;
    DD_REQUIRE(dd_fms_grid(n, step38, nb, G, 1, 1, 0, &gd), "dd_debug_fms_mix: need 0 <= n < 2^31, step38 < 2^32, 0 <= nb < 2^23 and 0 <= G <= 12288");
    if (n == 0) return DD_OK;
    DD_REQUIRE(mpx != nullptr && table != nullptr && (u != nullptr || nb == 0) && ab != nullptr, "dd_debug_fms_mix: null buffer");
    hipLaunchKernelGGL(k_fms_mix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dd_stream(stream), mpx, n, step38, (const int2*)table,
                       (const int2*)u, nb, G, (int2*)ab);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
