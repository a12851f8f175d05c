// Fused hot path on the matrix cores (general real taps, M == 1):
//
//     offsetFreq (NCO) -> FIR as a Toeplitz GEMM on v_mfma_f32_32x32x16_f16 -> demod_fm
//
// Why: in direct form the 255-tap complex FIR costs 1020 flop per 12 algorithmic
// bytes -- compute bound at ~23 % of the HBM roofline on the f32 VALU *or* the f32
// MFMA (same 157 TF peak).  The f16 matrix pipe is 16x faster, and
// float32-grade accuracy is kept by splitting both operands into two f16 limbs
// (x = xh + xl, g = gh + gl, 11+11 significant bits each) and accumulating
//     gh*xh + gh*xl + gl*xh        (the dropped gl*xl term is < 2^-22 relative)
// in the MFMA's f32 accumulator: 3/16 of the f32 cost.
//
// GEMM shape per wave (one "strip" of 1024 consecutive outputs):
//     D[i][j] = y[32 i + j] = sum_m A[i][m] * B[m][j],   i, j in [0, 32)
//     A[i][m] = s[32 i + m]          signal window of segment i   (LDS, f16 limbs)
//     B[m][j] = g2[m - j]            Toeplitz band of the reversed taps (constant fragments)
// K-dimension = 31 + (HALO+1) padded to 16*NKS.  With A = signal, the 32 lanes of
// one accumulator register hold 32 CONSECUTIVE outputs.
//
// LDS image: four f16 planes (re_hi, re_lo, im_hi, im_lo) of the NCO-rotated,
// power-of-two-scaled tile; every 32 samples are followed by 16 B of padding so the
// 64-byte-strided ds_read_b128 of the A fragments is bank-conflict free
// (dword index 20 i + 4 h, distinct for the 16 lanes of every b128 lane group).
//
// Two kernels:
//   k_chain_mfma_ab    interior tiles: persistent, wave-specialised (two sets of 4 matrix
//                      waves + 8 vector waves per CU), see dd_mfma_ab.h; the edge tiles
//                      ride along in the same launch;
//   k_chain_mfma_edge  stream start/end, unaligned or u8 input, partial tiles: one tile
//                      per 4-wave workgroup, fully predicated, same MFMA core.
#include "dd_chain_kernels.h"

typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef _Float16 v2h __attribute__((ext_vector_type(2)));
typedef float v16f __attribute__((ext_vector_type(16)));

#define MF_WAVES 4
#define MF_THREADS (MF_WAVES * 64)
#define MF_STRIP 1024
#define MF_T (MF_WAVES * MF_STRIP)
#define MF_ADV (MF_T - 32)

struct DDMfmaTaps {
    const v8h* frag;     // [limb][ks][lane] B fragments
    float inv_tapscale;  // 1 / (power-of-two scale applied to the taps)
    unsigned long long* stamps;   // unused (always nullptr); kept so that the kernel argument layout stays the same
};

__device__ __forceinline__ float dd_pow2_scale_for(float m) {
    // power of two s with m*s in [2^13, 2^14)  (s = 1 for m == 0 / denormal)
    const uint32_t eb = (__float_as_uint(m) >> 23) & 0xff;
    int se = 267 - (int)eb;
    se = se > 254 ? 254 : (se < 1 ? 1 : se);
    return eb == 0 ? 1.0f : __uint_as_float((uint32_t)se << 23);
}

// atan2 for the discriminator: odd degree-15 minimax polynomial on [0,1] (max error
// 4e-8 rad in exact arithmetic, 1.5e-7 rad evaluated in f32) + octant fix-up.
__device__ __forceinline__ float dd_fast_atan2(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float t = mn * __builtin_amdgcn_rcpf(mx);
    const float z = t * t;
    float p = -4.054567120e-03f;
    p = fmaf(p, z, 2.186295773e-02f);
    p = fmaf(p, z, -5.591232695e-02f);
    p = fmaf(p, z, 9.642197381e-02f);
    p = fmaf(p, z, -1.390862959e-01f);
    p = fmaf(p, z, 1.994656567e-01f);
    p = fmaf(p, z, -3.332986079e-01f);
    p = fmaf(p, z, 9.999993356e-01f);
    float r = p * t;
    r = (mx == 0.f) ? 0.f : r;                          // atan2(0,0) = 0 like np.angle
    r = (ay > ax) ? 1.5707963267948966f - r : r;
    r = (x < 0.f) ? 3.141592653589793f - r : r;
    return copysignf(r, y);
}

// atan(y/x) for x > 0, |y| <= tan(pi/8) x: t + t z (c0 + c1 z + c2 z^2 + c3 z^3), z = t^2
// (minimax fit on [0, tan(pi/8)]; 2.3e-8 rad evaluated in f32), no octant logic
__device__ __forceinline__ float dd_atan_small(float y, float x) {
    const float t = y * __builtin_amdgcn_rcpf(x);
    const float z = t * t;
    float p = fmaf(7.902598251e-02f, z, -1.382445378e-01f);
    p = fmaf(p, z, 1.997187931e-01f);
    p = fmaf(p, z, -3.333275667e-01f);
    return fmaf(t, z * p, t);
}

__device__ __forceinline__ float dd_fm_angle_fast(float cx, float cy, float px, float py) {
    const float re = fmaf(cx, px, cy * py);
    const float im = fmaf(cy, px, -cx * py);
    return dd_fast_atan2(im, re);
}

// value of the lane one to the left (DPP wave_shr:1); lanes 0/32 are patched by the caller
__device__ __forceinline__ float dd_lane_left(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float dd_readlane(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// bytes of LDS used by one tile's staging (planes + phasors + reduction + strip hand-over)
#define MF_LDS_TILE_BYTES(NKS) ((4 * MfmaGeom<NKS>::PLANE + 8 * MfmaGeom<NKS>::NGRP + 4 * MF_WAVES + 8 * MF_WAVES + 15) & ~15)

template <int NKS>
struct MfmaGeom {
    static constexpr int HALO = 16 * NKS - 32;
    static constexpr int SPAN = MF_T + HALO;                     // staged samples (multiple of 32)
    static constexpr int PLANE = SPAN * 2 + (SPAN / 32) * 16;    // bytes per f16 plane incl. padding
    static constexpr int NIT = (SPAN / 2 + MF_THREADS - 1) / MF_THREADS;
    static constexpr int NGRP = (SPAN + 63) / 64;                // 64-sample NCO phasor groups (SPAN need not be a multiple of 64)
};

// samples n0, n0+1 of the chunk as the FIR sees them: stream edges, carried history (already
// NCO-rotated), u8 ingest.  Every load is unconditional on a clamped index and the value is
// selected afterwards: a predicated load makes hipcc branch and drain vmcnt per element
// (measured: one edge tile took 15 us that way).
__device__ __forceinline__ float4 dd_edge_fetch2(const DDChainParams& P, int64_t n0) {
    const bool u8 = (P.flags & DD_CHAIN_U8_INPUT) != 0;
    const int K1 = P.K - 1;
    float v[4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int64_t n = n0 + k;
        const int64_t nc = n < 0 ? 0 : (n >= P.L ? P.L - 1 : n);
        float2 x;
        if (u8) {
            const uchar2 u = reinterpret_cast<const uchar2*>(P.in)[nc];
            x = make_float2((float)u.x - 127.5f, (float)u.y - 127.5f);
        } else {
            x = reinterpret_cast<const float2*>(P.in)[nc];
        }
        const int64_t ti = n + K1;                       // index into the carried history
        const int64_t tc = ti < 0 ? 0 : (ti >= K1 ? (K1 > 0 ? K1 - 1 : 0) : ti);
        const float2 t = P.tail_in[tc];
        const bool in_chunk = n >= 0 && n < P.L;
        const bool in_tail = n < 0 && ti >= 0;
        v[2 * k] = in_chunk ? x.x : (in_tail ? t.x : 0.f);
        v[2 * k + 1] = in_chunk ? x.y : (in_tail ? t.y : 0.f);
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// edge tiles: issue the tile's global loads (two consecutive samples per lane per step)
template <int NKS>
__device__ __forceinline__ void dd_tile_load(const DDChainParams& P, int b, float4 (&raw)[MfmaGeom<NKS>::NIT]) {
    using G = MfmaGeom<NKS>;
    const int tid = threadIdx.x;
    const int64_t ns = (int64_t)b * MF_ADV - 32 - G::HALO;
#pragma unroll
    for (int it = 0; it < G::NIT; ++it) raw[it] = dd_edge_fetch2(P, ns + 2 * (tid + MF_THREADS * it));
}

// phasor of the first sample of this thread's 64-sample group of tile b (threads
// < NGRP); issued together with the tile's loads so its table fetch is off the
// critical path
template <int NKS>
__device__ __forceinline__ float2 dd_tile_w2(const DDChainParams& P, int b) {
    using G = MfmaGeom<NKS>;
    static_assert(G::NGRP <= MF_THREADS, "one group phasor per thread");
    const int64_t ns = (int64_t)b * MF_ADV - 32 - G::HALO;
    const int g = threadIdx.x < G::NGRP ? threadIdx.x : G::NGRP - 1;
    if (!(P.flags & DD_CHAIN_NCO)) return make_float2(1.f, 0.f);
    return dd_phasor((uint64_t)(P.abs0 + ns + (int64_t)g * 64) * P.cyc, P.nco_tbl);
}

// rotate, scale, split into f16 limbs, write the LDS planes.  Returns the tile's
// power-of-two scale.  Contains one barrier (max reduction; it also fences the
// previous tile's LDS reads).
template <int NKS>
__device__ __forceinline__ float dd_tile_stage(const DDChainParams& P, int b, const float4 (&raw)[MfmaGeom<NKS>::NIT],
                                               char* smem, float2 w1a, float2 w1b, float2 w2mine) {
    using G = MfmaGeom<NKS>;
    char* planes = smem;
    float2* w2 = reinterpret_cast<float2*>(smem + 4 * G::PLANE);
    float* red = reinterpret_cast<float*>(w2 + G::NGRP);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t ns = (int64_t)b * MF_ADV - 32 - G::HALO;
    const bool nco = (P.flags & DD_CHAIN_NCO) != 0;
    const int K = P.K;

    float m = 0.f;
#pragma unroll
    for (int it = 0; it < G::NIT; ++it) {
        m = fmaxf(m, fmaxf(fmaxf(fabsf(raw[it].x), fabsf(raw[it].y)), fmaxf(fabsf(raw[it].z), fabsf(raw[it].w))));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __syncthreads();                    // previous tile: all LDS reads (planes, w2, red, wlast) are done
    if (lane == 0) red[wave] = m;
    if (tid < G::NGRP) w2[tid] = w2mine;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float scale = dd_pow2_scale_for(m);
    const float inv_scale = 1.0f / scale;

    const int64_t tail_first = P.L - (K - 1);       // first sample of the new history
    const bool tail_writer = (b == P.nblocks - 1) && P.tail_out != nullptr;
#pragma unroll
    for (int it = 0; it < G::NIT; ++it) {
        const int e = 2 * (tid + MF_THREADS * it);
        if (e >= G::SPAN) continue;
        const int64_t n = ns + e;
        float2 pa = make_float2(scale, 0.f), pb = make_float2(scale, 0.f);
        if (nco) {
            const float2 g = w2[e >> 6];
            const float2 gs = make_float2(g.x * scale, g.y * scale);
            if (n >= 0) pa = dd_cmul(gs, w1a);                 // history samples (n < 0) are already rotated
            if (n + 1 >= 0) pb = dd_cmul(gs, w1b);
        }
        const float2 xa = dd_cmul(make_float2(raw[it].x, raw[it].y), pa);
        const float2 xb = dd_cmul(make_float2(raw[it].z, raw[it].w), pb);
        if (tail_writer) {
            if (n >= tail_first && n < P.L) P.tail_out[n - tail_first] = make_float2(xa.x * inv_scale, xa.y * inv_scale);
            if (n + 1 >= tail_first && n + 1 < P.L) P.tail_out[n + 1 - tail_first] = make_float2(xb.x * inv_scale, xb.y * inv_scale);
        }
        v2h rh, rl, ih, il;
        rh.x = (_Float16)xa.x; rh.y = (_Float16)xb.x;
        ih.x = (_Float16)xa.y; ih.y = (_Float16)xb.y;
        rl.x = (_Float16)(xa.x - (float)rh.x); rl.y = (_Float16)(xb.x - (float)rh.y);
        il.x = (_Float16)(xa.y - (float)ih.x); il.y = (_Float16)(xb.y - (float)ih.y);
        const int off = 2 * e + 16 * (e >> 5);
        *reinterpret_cast<v2h*>(planes + off) = rh;
        *reinterpret_cast<v2h*>(planes + G::PLANE + off) = rl;
        *reinterpret_cast<v2h*>(planes + 2 * G::PLANE + off) = ih;
        *reinterpret_cast<v2h*>(planes + 3 * G::PLANE + off) = il;
    }
    return scale;
}

// epilogue.  lane (j = lane & 31, h = lane >> 5), register r holds output
//   p = P0 + 1024*wave + 32*row + j,  row = (r & 3) + 8 (r >> 2) + 4 h
template <int NKS>
__device__ __forceinline__ void dd_tile_epilogue(const DDChainParams& P, int b, v16f& cre, v16f& cim, float unscale, char* smem) {
    using G = MfmaGeom<NKS>;
    float2* wlast = reinterpret_cast<float2*>(smem + 4 * G::PLANE + sizeof(float2) * G::NGRP + sizeof(float) * MF_WAVES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int64_t P0 = (int64_t)b * MF_ADV - 32;
    const int64_t pw = P0 + (int64_t)wave * MF_STRIP;
    const int64_t p_lo = P0 + 32;                          // first output this tile owns
    const bool fm = (P.flags & DD_CHAIN_FM) != 0;

    if (!fm) {
        float2* out = reinterpret_cast<float2*>(P.out);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int64_t p = pw + 32 * row + j;
            if (p >= p_lo && p < P.Ld)
                out[p] = make_float2(cre[r] * unscale, cim[r] * unscale);
        }
        return;
    }

    if (P.s == 0 && b == 0 && wave == 0 && lane == 31) {   // p == -1: sample carried from the previous chunk
        const float2 ly = *P.lasty_in;                     // (any positive scale: only its angle matters)
        cre[0] = ly.x;
        cim[0] = ly.y;
    }
    if (lane == 63) wlast[wave] = make_float2(cre[15], cim[15]);
    __syncthreads();
    const float2 prev_strip = (wave > 0) ? wlast[wave - 1] : make_float2(0.f, 0.f);

    // column-0 neighbours: row-1 is register r-1 of lane 31/63, or sits across the
    // 4-row split of the accumulator layout (register r+3 / r-1 of the other half)
    float* out = reinterpret_cast<float*>(P.out) + (pw - P.s) + j + 128 * h;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float pre = dd_lane_left(cre[r]);
        float pim = dd_lane_left(cim[r]);
        float a_re, a_im, c_re, c_im;                      // for lane 0 and lane 32
        if ((r & 3) != 0) {
            a_re = dd_readlane(cre[r - 1], 31); a_im = dd_readlane(cim[r - 1], 31);
            c_re = dd_readlane(cre[r - 1], 63); c_im = dd_readlane(cim[r - 1], 63);
        } else {
            if (r > 0) { a_re = dd_readlane(cre[r - 1], 63); a_im = dd_readlane(cim[r - 1], 63); }
            else { a_re = prev_strip.x; a_im = prev_strip.y; }
            c_re = dd_readlane(cre[r + 3], 31); c_im = dd_readlane(cim[r + 3], 31);
        }
        pre = (lane == 0) ? a_re : pre;  pim = (lane == 0) ? a_im : pim;
        pre = (lane == 32) ? c_re : pre; pim = (lane == 32) ? c_im : pim;
        const int rowbase = (r & 3) + 8 * (r >> 2);        // row = rowbase + 4h
        const float ang = dd_fm_angle_fast(cre[r], cim[r], pre, pim);
        const int64_t p = pw + 32 * (rowbase + 4 * h) + j;
        if (p >= p_lo && p >= P.s && p < P.Ld) out[32 * rowbase] = ang;
        if (p == P.Ld - 1) *P.lasty_out = make_float2(cre[r] * unscale, cim[r] * unscale);
    }
}

// Edge tiles (stream start/end, unaligned or u8 input, partial tiles): one tile per 4-wave
// workgroup, fully predicated, tap fragments held in registers (stand-alone edge kernel).
template <int NKS>
__device__ __forceinline__ void dd_edge_tile(const DDChainParams& P, const DDMfmaTaps& taps, int b, char* smem) {
    using G = MfmaGeom<NKS>;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float4 raw[G::NIT];
    dd_tile_load<NKS>(P, b, raw);
    float2 w1a = make_float2(1.f, 0.f), w1b = make_float2(1.f, 0.f);
    if (P.flags & DD_CHAIN_NCO) {
        w1a = dd_phasor((uint64_t)((2 * tid) & 63) * P.cyc, P.nco_tbl);
        w1b = dd_phasor((uint64_t)(((2 * tid) & 63) + 1) * P.cyc, P.nco_tbl);
    }
    const float scale = dd_tile_stage<NKS>(P, b, raw, smem, w1a, w1b, dd_tile_w2<NKS>(P, b));
    v8h bh[NKS], bl[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        bh[ks] = taps.frag[ks * 64 + lane];
        bl[ks] = taps.frag[(NKS + ks) * 64 + lane];
    }
    __syncthreads();
    const int i = lane & 31, h = lane >> 5;
    const int sb = wave * MF_STRIP;
    const char* abase = smem + (2 * sb + (sb >> 1)) + 80 * i + 16 * h;
    v16f cre, cim;
#pragma unroll
    for (int r = 0; r < 16; ++r) { cre[r] = 0.f; cim[r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int off = 32 * ks + 16 * (ks >> 1);
        const v8h arh = *reinterpret_cast<const v8h*>(abase + off);
        const v8h arl = *reinterpret_cast<const v8h*>(abase + G::PLANE + off);
        const v8h aih = *reinterpret_cast<const v8h*>(abase + 2 * G::PLANE + off);
        const v8h ail = *reinterpret_cast<const v8h*>(abase + 3 * G::PLANE + off);
        const v8h th = bh[ks], tl = bl[ks];
        cre = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, th, cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, th, cim, 0, 0, 0);
        cre = __builtin_amdgcn_mfma_f32_32x32x16_f16(arl, th, cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_32x32x16_f16(ail, th, cim, 0, 0, 0);
        cre = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, tl, cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, tl, cim, 0, 0, 0);
    }
    dd_tile_epilogue<NKS>(P, b, cre, cim, taps.inv_tapscale / scale, smem);
}

// The same edge tile inside the register budget of the 16-wave ws kernel (a kernel that
// spills there runs its persistent loop ~12 % slower -- measured -- even though the spills
// sit in this path only): the tile is fetched twice, once for its peak and once to stage
// it, three fetches in flight, instead of being held in 36 registers.
template <int NKS>
__device__ __forceinline__ void dd_edge_tile_lean(const DDChainParams& P, const DDMfmaTaps& taps, int b, char* smem, const v8h* lds_taps) {
    using G = MfmaGeom<NKS>;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t ns = (int64_t)b * MF_ADV - 32 - G::HALO;
    char* planes = smem;
    float* red = reinterpret_cast<float*>(smem + 4 * G::PLANE + 8 * G::NGRP);   // same LDS layout as dd_tile_stage
    const bool nco = (P.flags & DD_CHAIN_NCO) != 0;
    float m = 0.f;
#pragma unroll 3
    for (int it = 0; it < G::NIT; ++it) {
        const float4 v = dd_edge_fetch2(P, ns + 2 * (tid + MF_THREADS * it));
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float scale = dd_pow2_scale_for(m);
    const float inv_scale = 1.0f / scale;
    const int64_t tail_first = P.L - (P.K - 1);     // first sample of the new history
    const bool tail_writer = (b == P.nblocks - 1) && P.tail_out != nullptr;
#pragma unroll 3
    for (int it = 0; it < G::NIT; ++it) {
        const int e = 2 * (tid + MF_THREADS * it);
        if (e >= G::SPAN) continue;
        const int64_t n = ns + e;
        const float4 v = dd_edge_fetch2(P, n);
        float2 pa = make_float2(scale, 0.f), pb = make_float2(scale, 0.f);
        if (nco) {                                  // history samples (n < 0) are already rotated
            if (n >= 0) { const float2 w = dd_phasor((uint64_t)(P.abs0 + n) * P.cyc, P.nco_tbl); pa = make_float2(w.x * scale, w.y * scale); }
            if (n + 1 >= 0) { const float2 w = dd_phasor((uint64_t)(P.abs0 + n + 1) * P.cyc, P.nco_tbl); pb = make_float2(w.x * scale, w.y * scale); }
        }
        const float2 xa = dd_cmul(make_float2(v.x, v.y), pa);
        const float2 xb = dd_cmul(make_float2(v.z, v.w), pb);
        if (tail_writer) {
            if (n >= tail_first && n < P.L) P.tail_out[n - tail_first] = make_float2(xa.x * inv_scale, xa.y * inv_scale);
            if (n + 1 >= tail_first && n + 1 < P.L) P.tail_out[n + 1 - tail_first] = make_float2(xb.x * inv_scale, xb.y * inv_scale);
        }
        v2h rh, rl, ih, il;
        rh.x = (_Float16)xa.x; rh.y = (_Float16)xb.x;
        ih.x = (_Float16)xa.y; ih.y = (_Float16)xb.y;
        rl.x = (_Float16)(xa.x - (float)rh.x); rl.y = (_Float16)(xb.x - (float)rh.y);
        il.x = (_Float16)(xa.y - (float)ih.x); il.y = (_Float16)(xb.y - (float)ih.y);
        const int off = 2 * e + 16 * (e >> 5);
        *reinterpret_cast<v2h*>(planes + off) = rh;
        *reinterpret_cast<v2h*>(planes + G::PLANE + off) = rl;
        *reinterpret_cast<v2h*>(planes + 2 * G::PLANE + off) = ih;
        *reinterpret_cast<v2h*>(planes + 3 * G::PLANE + off) = il;
    }
    __syncthreads();
    const int i = lane & 31, h = lane >> 5;
    const int sb = wave * MF_STRIP;
    const char* abase = smem + (2 * sb + (sb >> 1)) + 80 * i + 16 * h;
    v16f cre, cim;
#pragma unroll
    for (int r = 0; r < 16; ++r) { cre[r] = 0.f; cim[r] = 0.f; }
#pragma unroll 2
    for (int ks = 0; ks < NKS; ++ks) {
        const int off = 32 * ks + 16 * (ks >> 1);
        const v8h arh = *reinterpret_cast<const v8h*>(abase + off);
        const v8h arl = *reinterpret_cast<const v8h*>(abase + G::PLANE + off);
        const v8h aih = *reinterpret_cast<const v8h*>(abase + 2 * G::PLANE + off);
        const v8h ail = *reinterpret_cast<const v8h*>(abase + 3 * G::PLANE + off);
        const v8h th = lds_taps[ks * 64 + lane];
        const v8h tl = lds_taps[(NKS + ks) * 64 + lane];
        cre = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, th, cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, th, cim, 0, 0, 0);
        cre = __builtin_amdgcn_mfma_f32_32x32x16_f16(arl, th, cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_32x32x16_f16(ail, th, cim, 0, 0, 0);
        cre = __builtin_amdgcn_mfma_f32_32x32x16_f16(arh, tl, cre, 0, 0, 0);
        cim = __builtin_amdgcn_mfma_f32_32x32x16_f16(aih, tl, cim, 0, 0, 0);
    }
    dd_tile_epilogue<NKS>(P, b, cre, cim, taps.inv_tapscale / scale, smem);
}

template <int NKS>
__global__ void __launch_bounds__(MF_THREADS, 2) k_chain_mfma_edge(const DDChainParams P, const DDMfmaTaps taps, int t_first, int t_last) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // edge tiles are [0, t_first) and [t_last, nblocks)
    const int b = (int)blockIdx.x < t_first ? (int)blockIdx.x : t_last + ((int)blockIdx.x - t_first);
    dd_edge_tile<NKS>(P, taps, b, smem);
}

// max over the wave in 6 DPP steps (row_shr 1,2,4,8 then row_bcast 15/31); valid in lane 63
__device__ __forceinline__ float dd_wave_max(float m) {
#define DD_DPP_MAX(ctrl, rmask)                                                                              \
    m = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), ctrl, rmask, 0xf, false)));
    DD_DPP_MAX(0x111, 0xf)      // row_shr:1   (values are >= 0, so the 0 filled into invalid lanes is neutral)
    DD_DPP_MAX(0x112, 0xf)      // row_shr:2
    DD_DPP_MAX(0x114, 0xf)      // row_shr:4
    DD_DPP_MAX(0x118, 0xf)      // row_shr:8   -> lane 15 of each row holds the row max
    DD_DPP_MAX(0x142, 0xa)      // row_bcast:15 into rows 1 and 3
    DD_DPP_MAX(0x143, 0xc)      // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave max
#undef DD_DPP_MAX
    return m;
}

#include "dd_mfma_ab.h"

// ============================================================================
// host side
// ============================================================================
struct DDMfmaState {
    int nks = 0;
    DDDevBuf<v8h> frag;         // device
    float inv_tapscale = 1.f;
};

static int mfma_nks_for(int K) {
    const int opts[4] = {6, 10, 12, 18};
    for (int i = 0; i < 4; ++i)
        if (K <= 16 * opts[i] - 31) return opts[i];
    return 0;
}

int dd_mfma_supported(int K, int M) {
    return M == 1 ? mfma_nks_for(K) : 0;
}

int dd_mfma_create(void** st, const double* taps, int K) {
    const int nks = mfma_nks_for(K);
    if (!nks) return DD_ERR_UNSUPPORTED;
    const int HALO = 16 * nks - 32;
    // correlation form: y[o] = sum_j' g2[j'] s[o + j'], j' in [0, HALO], element 0 of
    // the window is HALO samples before the output sample
    double mx = 0.0;
    for (int k = 0; k < K; ++k) mx = fmax(mx, fabs(taps[k]));
    int ex = 0;
    if (mx > 0.0) frexp(mx, &ex);                         // mx = f * 2^ex, f in [0.5, 1)
    const double tapscale = ldexp(1.0, -ex);
    std::vector<double> g2(HALO + 1, 0.0);
    for (int k = 0; k < K; ++k) g2[HALO - k] = taps[k] * tapscale;   // tap k multiplies the sample k before the output
    std::vector<_Float16> frag((size_t)2 * nks * 64 * 8);
    for (int ks = 0; ks < nks; ++ks) {
        for (int lane = 0; lane < 64; ++lane) {
            const int j = lane & 31, h = lane >> 5;
            for (int t = 0; t < 8; ++t) {
                const int m = 16 * ks + 8 * h + t;
                const int idx = m - j;
                const double g = (idx >= 0 && idx <= HALO) ? g2[idx] : 0.0;
                const _Float16 gh = (_Float16)g;
                const _Float16 gl = (_Float16)(g - (double)gh);
                frag[((size_t)(0 * nks + ks) * 64 + lane) * 8 + t] = gh;
                frag[((size_t)(1 * nks + ks) * 64 + lane) * 8 + t] = gl;
            }
        }
    }
    DDMfmaState* s = new DDMfmaState();
    s->nks = nks;
    s->inv_tapscale = (float)(1.0 / tapscale);
    static_assert(sizeof(v8h) == 8 * sizeof(_Float16), "fragment size");
    hipError_t e = s->frag.alloc(frag.size() / 8);
    if (e == hipSuccess) e = hipMemcpy(s->frag, frag.data(), frag.size() * sizeof(_Float16), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete s;
        dd_set_error("dd_mfma_create: %s", hipGetErrorString(e));
        return DD_ERR_HIP;
    }
    *st = s;
    return DD_OK;
}

void dd_mfma_destroy(void* st) {
    delete reinterpret_cast<DDMfmaState*>(st);
}

template <int NKS>
static int mfma_launch_t(DDMfmaState* st, DDChainParams& P, hipStream_t s, int* kernel_id) {
    using G = MfmaGeom<NKS>;
    const size_t lds = (size_t)MF_LDS_TILE_BYTES(NKS);
    static DDOncePerDevice attr_set;
    if (attr_set.need()) {
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_chain_mfma_edge<NKS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_chain_mfma_ab<NKS, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AbGeom<NKS>::LDS_BYTES));
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_chain_mfma_ab<NKS, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AbGeom<NKS>::LDS_BYTES));
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_chain_mfma_ab<NKS, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AbGeom<NKS>::LDS_BYTES));
        DD_HIP_CHECK(hipFuncSetAttribute((const void*)k_chain_mfma_ab<NKS, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AbGeom<NKS>::LDS_BYTES));
        attr_set.mark();
    }
    DDMfmaTaps t;
    t.frag = st->frag;
    t.inv_tapscale = st->inv_tapscale;
    t.stamps = nullptr;
    // interior tiles: whole span inside the chunk, all outputs emitted, aligned complex64
    int t_first = 1, t_last = 1;
    const bool u8in = (P.flags & DD_CHAIN_U8_INPUT) != 0;
    const bool aligned = (reinterpret_cast<uintptr_t>(P.in) & (u8in ? 3 : 15)) == 0;
    if (aligned && P.nblocks > 2) {
        // tile b: ns = b*ADV - 32 - HALO >= 0 ; ns + SPAN <= L ; b*ADV - 32 + T <= Ld
        int64_t lo = (32 + G::HALO + MF_ADV - 1) / MF_ADV;
        if (lo < 1) lo = 1;
        int64_t hi1 = (P.L - G::SPAN + 32 + G::HALO) / MF_ADV;         // last b with ns + SPAN <= L
        int64_t hi2 = (P.Ld - MF_T + 32) / MF_ADV;                     // last b with P0 + T <= Ld
        int64_t hi = hi1 < hi2 ? hi1 : hi2;
        if (hi > P.nblocks - 2) hi = P.nblocks - 2;
        if (hi >= lo) { t_first = (int)lo; t_last = (int)hi + 1; }
    }
    const int n_int = t_last - t_first;
    if (n_int > 0) {
        // one 16-wave workgroup per CU (LDS bound): persistent workgroups for the interior run plus
        // one workgroup per edge tile (both sides of the run), all resident at once -- the edge
        // tiles cost neither a launch of their own nor a tail after the persistent loop
        const int n_edge = t_first + (P.nblocks - t_last);
        const int ncu = dd_cu_count();
        const int cus = n_edge < ncu / 2 ? ncu - n_edge : ncu / 2;
        int grid = (n_int + 3) / 4 < cus ? (n_int + 3) / 4 : cus;
        const bool cx = !(P.flags & DD_CHAIN_FM);
        const dim3 g(grid + n_edge), b(AB_THREADS);
        const size_t lds_ab = (size_t)AbGeom<NKS>::LDS_BYTES;
        if (u8in && cx) hipLaunchKernelGGL((k_chain_mfma_ab<NKS, true, true>), g, b, lds_ab, s, P, t, t_first, t_last, grid);
        else if (u8in) hipLaunchKernelGGL((k_chain_mfma_ab<NKS, true, false>), g, b, lds_ab, s, P, t, t_first, t_last, grid);
        else if (cx) hipLaunchKernelGGL((k_chain_mfma_ab<NKS, false, true>), g, b, lds_ab, s, P, t, t_first, t_last, grid);
        else hipLaunchKernelGGL((k_chain_mfma_ab<NKS, false, false>), g, b, lds_ab, s, P, t, t_first, t_last, grid);
        DD_LAUNCH_CHECK();
        if (kernel_id) *kernel_id = DD_KERNEL_MFMA_AB;
    } else {
        hipLaunchKernelGGL(k_chain_mfma_edge<NKS>, dim3(P.nblocks), dim3(MF_THREADS), lds, s, P, t, P.nblocks, P.nblocks);
        DD_LAUNCH_CHECK();
        if (kernel_id) *kernel_id = DD_KERNEL_MFMA_TILES;
    }
    return DD_OK;
}

int dd_mfma_launch(void* stv, const DDChainParams& Pin, hipStream_t s, int* kernel_id) {
    DDMfmaState* st = reinterpret_cast<DDMfmaState*>(stv);
    DDChainParams P = Pin;
    P.T = MF_T;
    P.nblocks = (int)((P.Ld + MF_ADV - 1) / MF_ADV);
    if (P.nblocks < 1) P.nblocks = 1;
    switch (st->nks) {
        case 6: return mfma_launch_t<6>(st, P, s, kernel_id);
        case 10: return mfma_launch_t<10>(st, P, s, kernel_id);
        case 12: return mfma_launch_t<12>(st, P, s, kernel_id);
        case 18: return mfma_launch_t<18>(st, P, s, kernel_id);
    }
    return DD_ERR_UNSUPPORTED;
}

// dd_code_warmup (dd_runtime.hip): the runtime loads a translation unit's code object when one of its kernels is first named
int dd_code_touch_mfma(void) {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void*)k_chain_mfma_edge<16>) == hipSuccess ? DD_OK : DD_ERR_HIP;
}
