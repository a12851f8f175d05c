// Device code of dd_chain.hip: the f32 direct-form kernels of the fused chain (NCO -> FIR -> decimate -> FM) and their
// helpers.  Included by dd_chain.hip only (which holds the handles, the dispatcher, the launch plans and the C entry points).
//   k_chain_dense        (M == 1)  256 threads x 8 contiguous outputs, register-tiled sliding window, planar skewed LDS
//   k_chain_decim        (M >= 2)  one thread per kept output, one workgroup per tile (edge tiles, short or unaligned chunks)
//   k_chain_decim_p      (M >= 2)  persistent workgroups over the interior tiles, the edge tiles ride along
//   k_chain_decim_multi  (M >= 2)  the same for every chunk of a chunk list in one launch
//   k_tail_update, k_fill_c64, k_fm: history only, constant histories, the stand-alone discriminator
// Taps are wave-uniform and come through the scalar cache (s_load), so the VALU issues only FMAs and LDS reads.
#pragma once
#include "dd_chain_kernels.h"

#define DD_DENSE_R 8
#define DD_DENSE_THREADS 256
#define DD_DENSE_T (DD_DENSE_R * DD_DENSE_THREADS)
#ifndef DD_DECIM_THREADS
#define DD_DECIM_THREADS 256
#endif
#ifndef DD_DECIM_SPAN_MAX
#define DD_DECIM_SPAN_MAX 6144
#endif

// ============================================================================
// dense kernel
// ============================================================================
// LDS: sre[pos(e)], sim[pos(e)], pos(e) = e + (e >> 3)  (thread t reads 9t + ...)
__global__ void __launch_bounds__(DD_DENSE_THREADS) k_chain_dense(const DDChainParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int R = DD_DENSE_R;
    const int T = DD_DENSE_T;
    const int K = P.K;
    const int niter = (K + R - 1 + R - 1) / R;          // window elements / R, rounded up
    const int S = T + niter * R;                        // staged elements (incl. slack)
    const int SP = S + (S >> 3) + 8;                    // skewed length
    float* sre = reinterpret_cast<float*>(smem);
    float* sim = sre + SP;
    float2* w2 = reinterpret_cast<float2*>(sim + SP);   // per-64-group phasors
    float2* ylast = w2 + ((S + 63) / 64 + 1);           // per-thread last output

    const int t = threadIdx.x;
    const int b = dd_xcd_tile(blockIdx.x, P.nblocks);
    const int64_t pfirst = dd_tile_pfirst(P, b);
    const int64_t ns = pfirst - (K - 1);                // chunk-relative index of staged element 0
    const bool fm = (P.flags & DD_CHAIN_FM) != 0;

    // ---- per-group NCO phasors
    const int ngroups = (S + 63) / 64;
    if (P.flags & DD_CHAIN_NCO) {
        for (int g = t; g < ngroups; g += DD_DENSE_THREADS) {
            const uint64_t ph = (uint64_t)(P.abs0 + ns + (int64_t)g * 64) * P.cyc;
            w2[g] = dd_phasor(ph, P.nco_tbl);
        }
    }
    __syncthreads();
    // ---- stage the tile (coalesced), NCO applied on the way in
    {
        const float2 w1 = (P.flags & DD_CHAIN_NCO) ? dd_phasor((uint64_t)(t & 63) * P.cyc, P.nco_tbl) : make_float2(1.f, 0.f);
        // interior tile: batches of 8 unconditional loads in flight per lane (a predicated
        // load makes hipcc branch and wait for every element separately)
        const bool interior = !(P.flags & DD_CHAIN_U8_INPUT) && ns >= 0 && ns + S <= P.L;
        if (interior) {
            const float2* __restrict__ src = reinterpret_cast<const float2*>(P.in) + ns;
            for (int e0 = t; e0 < S; e0 += 8 * DD_DENSE_THREADS) {
                float2 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = e0 + u * DD_DENSE_THREADS;
                    v[u] = src[e < S ? e : S - 1];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = e0 + u * DD_DENSE_THREADS;
                    if (e < S) {
                        float2 x = v[u];
                        if (P.flags & DD_CHAIN_NCO) x = dd_cmul(x, dd_cmul(w2[e >> 6], w1));
                        const int p = e + (e >> 3);
                        sre[p] = x.x;
                        sim[p] = x.y;
                    }
                }
            }
        } else {
            for (int e = t; e < S; e += DD_DENSE_THREADS) {
                float2 ph = make_float2(1.f, 0.f);
                if (P.flags & DD_CHAIN_NCO) ph = dd_cmul(w2[e >> 6], w1);
                const float2 v = dd_load_sample(P, ns + e, ph);
                const int p = e + (e >> 3);
                sre[p] = v.x;
                sim[p] = v.y;
            }
        }
    }
    __syncthreads();

    // ---- new tail: the last tile holds the chunk's final K-1 (post-NCO) samples
    if (b == P.nblocks - 1 && P.tail_out) {
        for (int i = t; i < K - 1; i += DD_DENSE_THREADS) {
            const int64_t e = (P.L - (K - 1) + i) - ns;
            const int p = (int)e + ((int)e >> 3);
            P.tail_out[i] = make_float2(sre[p], sim[p]);
        }
    }

    // ---- register-tiled correlation: y[o] = sum_j g[j] s[o + j], o = tR + r
    float are[DD_DENSE_R], aim[DD_DENSE_R];
#pragma unroll
    for (int r = 0; r < R; ++r) { are[r] = 0.f; aim[r] = 0.f; }
    const float* __restrict__ G = P.taps_rev;           // G[i] = g[i - (R-1)], zero padded
    const int base = 9 * t;                             // pos(tR) = 8t + t
    for (int it = 0; it < niter; ++it) {
        float g[2 * DD_DENSE_R - 1];
#pragma unroll
        for (int i = 0; i < 2 * R - 1; ++i) g[i] = G[it * R + i];   // uniform -> s_load
        float vre[DD_DENSE_R], vim[DD_DENSE_R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            vre[i] = sre[base + it * 9 + i];
            vim[i] = sim[base + it * 9 + i];
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                // element m = it*R + i pairs with tap j = m - r -> g[(R-1) + i - r]
                are[r] = fmaf(g[R - 1 + i - r], vre[i], are[r]);
                aim[r] = fmaf(g[R - 1 + i - r], vim[i], aim[r]);
            }
        }
    }

    // ---- epilogue
    const int64_t p0 = pfirst + (int64_t)t * R;         // FIR-output index of r = 0
    if (!fm) {
        float2* out = reinterpret_cast<float2*>(P.out);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t p = p0 + r;
            if (p < P.Ld) out[p] = make_float2(are[r], aim[r]);
        }
        if (P.lasty_out && p0 <= P.Ld - 1 && P.Ld - 1 < p0 + R) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (p0 + r == P.Ld - 1) *P.lasty_out = make_float2(are[r], aim[r]);
        }
        return;
    }
    if (p0 == -1) {            // y[-1] is the carried sample of the previous chunk
        const float2 ly = *P.lasty_in;
        are[0] = ly.x;
        aim[0] = ly.y;
    }
    ylast[t] = make_float2(are[R - 1], aim[R - 1]);
    __syncthreads();
    float2 prv = (t > 0) ? ylast[t - 1] : make_float2(0.f, 0.f);
    float* out = reinterpret_cast<float*>(P.out);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t p = p0 + r;
        const float2 cur = make_float2(are[r], aim[r]);
        if (p > pfirst && p < P.Ld) {
            out[p - P.s] = dd_fm_angle(cur, prv);
            if (p == P.Ld - 1) *P.lasty_out = cur;
        } else if (p == P.Ld - 1 && p >= 0) {
            *P.lasty_out = cur;       // single kept sample owned only as "previous"
        }
        prv = cur;
    }
}

// ============================================================================
// decimating kernel: one thread per kept output
// ============================================================================
// (device function: the stand-alone kernel k_chain_decim below runs it for every tile of a chunk without
// an interior run; k_chain_decim_p runs it in its trailing workgroups for the tiles around the interior run,
// so a chunk is ONE launch either way)
// in-launch hand-over of the carried state between the chunks of dd_chain_process_chunks (cdna_hip_programming.md,
// Guideline 16): the producer's stores are drained by every wave, the workgroup meets, one lane releases at agent scope
// and sets the flag with an agent-scope atomic; the consumer polls that one word relaxed from one lane, acquires once,
// the workgroup meets, then everybody reads with plain loads.  The flags are zeroed by a memset ahead of every launch.
// Producers have lower workgroup indices than their consumers and only two workgroups per chunk ever wait, so a
// waiting workgroup cannot keep its producer off the device; the spin is bounded all the same.
// A wait that gives up (the producer is not resident -- ascending dispatch order of workgroups is what the hardware does, not an
// architectural promise -- or is held up by a debugger or profiler) counts itself in *err and goes on with whatever the state
// buffers hold: the launch completes, its outputs are wrong, and the host turns the count into DD_ERR_TIMEOUT.
__device__ __forceinline__ void dd_seam_wait(unsigned int* flag, unsigned int* err, int spin_log2) {
    if (threadIdx.x == 0) {
        typedef __attribute__((address_space(1))) unsigned int gu32;
        gu32* f = (gu32*)flag;
        // default bound 2^19 polls of ~0.2 us (s_sleep 8) = ~0.1 s: three orders of magnitude above the ~100 us a producer tile of a
        // resident launch needs, and short enough that a launch whose producer is NOT resident (a GPU shared with another process)
        // fails within a second instead of holding the device for seconds per chunk (round 4's bound was 2^24)
        const unsigned bound = 1u << (spin_log2 > 0 && spin_log2 < 31 ? spin_log2 : 19);
        bool seen = false;
        for (unsigned spins = 0; spins < bound; ++spins) {
            if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { seen = true; break; }
            __builtin_amdgcn_s_sleep(8);
        }
        if (!seen && err) __hip_atomic_fetch_add((gu32*)err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (a word of pinned host memory)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
}
__device__ __forceinline__ void dd_seam_post(unsigned int* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // every storing wave
    __syncthreads();
    if (threadIdx.x == 0) {
        typedef __attribute__((address_space(1))) unsigned int gu32;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (ROCm 7.2 may drop the fence's own wait)
        __hip_atomic_store((gu32*)flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ void dd_decim_edge_tile(const DDChainParams& P, const int bid, char* smem) {
    const int K = P.K, M = P.M, T = P.T;
    const int S = (T - 1) * M + K + (M - 1);
    const int SP = S + 4;                                 // linear image: see the tap loop
    float2* sx = reinterpret_cast<float2*>(smem);
    float2* w2 = sx + SP;
    float2* yblk = w2 + ((S + 63) / 64 + 1);
    // taps, K floats (+ pad to 8), 16-byte aligned.  Offset arithmetic on the LDS base, not on a uintptr_t:
    // a pointer that went through an integer is a generic pointer to the compiler, its reads become
    // flat loads, and a flat load's vmcnt wait in the tap loop drains every tile load in flight
    float* gl = reinterpret_cast<float*>(smem + ((sizeof(float2) * ((size_t)SP + ((S + 63) / 64 + 1) + DD_DECIM_THREADS) + 15) & ~(size_t)15));

    const int t = threadIdx.x;
    int b = dd_xcd_tile(bid, P.nblocks - (P.skip_hi - P.skip_lo));
    if (b >= P.skip_lo) b += P.skip_hi - P.skip_lo;        // those tiles run in the persistent workgroups
    const int64_t pfirst = dd_tile_pfirst(P, b);
    const int64_t ns = (int64_t)P.off + pfirst * M - (K - 1);
    const bool fm = (P.flags & DD_CHAIN_FM) != 0;
    if (P.seam_wait && (ns < 0 || pfirst < 0)) dd_seam_wait(P.seam_wait, P.seam_err, P.seam_spin_log2);      // this tile reads the previous chunk's state

    const int ngroups = (S + 63) / 64;
    // interior tile (whole span inside the chunk, complex64 input): the WHOLE tile is requested at
    // once, before anything else -- up to 12 unconditional 16-byte loads (two samples each) in flight
    // per lane -- so a tile costs one HBM latency and that latency also covers the tap copy and the
    // phasor table fetches below.  (A predicated load -- edges, history, u8 -- makes hipcc branch and
    // wait for every element: those tiles take the loop further down.)
    typedef float v4f_a8 __attribute__((ext_vector_type(4), aligned(8)));     // 16-byte load on an 8-byte boundary
    constexpr int NV = (DD_DECIM_SPAN_MAX / 2 + DD_DECIM_THREADS - 1) / DD_DECIM_THREADS;
    const bool interior = !(P.flags & DD_CHAIN_U8_INPUT) && ns >= 0 && ns + S <= P.L && S <= DD_DECIM_SPAN_MAX;
    const int nq = S / 2;                                     // whole sample pairs in the span
    v4f_a8 v[NV];
    if (interior) {
        const float2* __restrict__ src = reinterpret_cast<const float2*>(P.in) + ns;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            int q = t + u * DD_DECIM_THREADS;
            q = q < nq ? q : nq - 1;                          // past the span: harmless re-read, never used
            v[u] = *reinterpret_cast<const v4f_a8*>(src + 2 * q);
        }
    }
    for (int j = t; j < ((K + 7) & ~7); j += DD_DECIM_THREADS) gl[j] = j < K ? P.taps_rev[(DD_DENSE_R - 1) + j] : 0.f;
    if (P.flags & DD_CHAIN_NCO) {
        for (int g = t; g < ngroups; g += DD_DECIM_THREADS) {
            const uint64_t ph = (uint64_t)(P.abs0 + ns + (int64_t)g * 64) * P.cyc;
            w2[g] = dd_phasor(ph, P.nco_tbl);
        }
    }
    __syncthreads();
    {
        const float2 w1 = (P.flags & DD_CHAIN_NCO) ? dd_phasor((uint64_t)(t & 63) * P.cyc, P.nco_tbl) : make_float2(1.f, 0.f);
        if (interior) {
            const float2* __restrict__ src = reinterpret_cast<const float2*>(P.in) + ns;
            float2 w1a = make_float2(1.f, 0.f), w1b = make_float2(1.f, 0.f);
            if (P.flags & DD_CHAIN_NCO) {
                w1a = dd_phasor((uint64_t)((2 * t) & 63) * P.cyc, P.nco_tbl);
                w1b = dd_phasor((uint64_t)(((2 * t) & 63) + 1) * P.cyc, P.nco_tbl);
            }
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                const int q = t + u * DD_DECIM_THREADS;
                const int e = 2 * q;
                if (q < nq) {
                    float2 xa = make_float2(v[u].x, v[u].y), xb = make_float2(v[u].z, v[u].w);
                    if (P.flags & DD_CHAIN_NCO) {
                        const float2 g = w2[e >> 6];
                        xa = dd_cmul(xa, dd_cmul(g, w1a));
                        xb = dd_cmul(xb, dd_cmul(g, w1b));
                    }
                    sx[e] = xa;
                    sx[e + 1] = xb;
                }
            }
            if ((S & 1) && t == 0) {                          // odd span: its last sample on its own
                const int e = S - 1;
                float2 x = src[e];
                if (P.flags & DD_CHAIN_NCO) x = dd_cmul(x, dd_cmul(w2[e >> 6], dd_phasor((uint64_t)(e & 63) * P.cyc, P.nco_tbl)));
                sx[e] = x;
            }
        } else {
            // edge tile (stream start with the carried history, chunk end, u8 input): batches of 8 UNCONDITIONAL loads
            // on clamped indices, the value selected afterwards.  A predicated load (dd_load_sample) makes hipcc branch
            // and wait per element: 24 dependent round trips, ~20 us for one tile -- which set the duration of the
            // whole launch for chunks of a few million samples (C3: 2^22-sample chunks, 21 us each)
            const bool u8 = (P.flags & DD_CHAIN_U8_INPUT) != 0;
            const bool need_tail = ns < 0;                             // block uniform
            const int K1 = K - 1;
            // the whole span in ONE round of loads (up to 24 per lane): an edge tile is on the critical path of every
            // launch -- each chunk has a first and a last one -- and in three rounds of eight its three memory round
            // trips were most of the ~9 us a launch costs before its first byte of payload
            constexpr int NB = DD_DECIM_SPAN_MAX / DD_DECIM_THREADS;   // 24
            constexpr int NT = 2;                                      // rounds whose samples may lie in the carried history (K - 1 <= 512)
            float2 x[NB], h[NT];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int64_t n = ns + t + u * DD_DECIM_THREADS;
                const int64_t nc = n < 0 ? 0 : (n >= P.L ? P.L - 1 : n);
                if (u8) {
                    const uchar2 q = reinterpret_cast<const uchar2*>(P.in)[nc];
                    x[u] = make_float2((float)q.x - 127.5f, (float)q.y - 127.5f);
                } else {
                    x[u] = reinterpret_cast<const float2*>(P.in)[nc];
                }
            }
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                h[u] = make_float2(0.f, 0.f);
                if (need_tail) {
                    const int64_t ti = ns + t + u * DD_DECIM_THREADS + K1;
                    h[u] = P.tail_in[ti < 0 ? 0 : (ti >= K1 ? (K1 > 0 ? K1 - 1 : 0) : ti)];
                }
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int e = t + u * DD_DECIM_THREADS;
                if (e < S) {
                    const int64_t n = ns + e;
                    float2 v = x[u];
                    if (P.flags & DD_CHAIN_NCO) v = dd_cmul(v, dd_cmul(w2[e >> 6], w1));
                    // history samples are already rotated; before the history and past the chunk: zeros
                    if (n < 0) {
                        if (u < NT) v = (n + K1 >= 0) ? h[u] : make_float2(0.f, 0.f);
                        else v = (n + K1 >= 0) ? P.tail_in[n + K1] : make_float2(0.f, 0.f);     // (filters longer than 513 taps)
                    }
                    if (n >= P.L) v = make_float2(0.f, 0.f);
                    sx[e] = v;
                }
            }
            for (int e = t + NB * DD_DECIM_THREADS; e < S; e += DD_DECIM_THREADS) {     // (spans beyond DD_DECIM_SPAN_MAX: long filters)
                float2 ph = make_float2(1.f, 0.f);
                if (P.flags & DD_CHAIN_NCO) ph = dd_cmul(w2[e >> 6], w1);
                sx[e] = dd_load_sample(P, ns + e, ph);
            }
        }
    }
    __syncthreads();

    if (b == P.nblocks - 1 && P.tail_out) {
        for (int i = t; i < K - 1; i += DD_DECIM_THREADS) {
            const int64_t e = (P.L - (K - 1) + i) - ns;
            P.tail_out[i] = sx[(int)e];
        }
    }

    // Tap loop.  The LDS image is linear (no skew) on purpose: thread t's window starts at sample
    // t*M, so every read is base + immediate offset (ds_read2_b64) and a tap costs one packed FMA.
    // A skewed image avoided the 2-way bank conflict of the stride-M reads but cost ~4 vector
    // instructions of index arithmetic per tap.  Taps are read from their LDS copy: fetched from
    // global memory here they came as per-lane vector loads with a wait every 16 taps.
    float2 acc = make_float2(0.f, 0.f);
    const float* __restrict__ G = gl;                              // g[j] = h[K-1-j]
    if (t < T) {
        const float2* __restrict__ win = sx + t * M;
        int j = 0;
        if ((M & 1) == 0) {
            // even M: every window starts on a 16-byte boundary -> ds_read_b128 (two samples), whose
            // 16-lane groups make the stride-M reads bank-conflict free at 256 B/clk; as ds_read2_b64
            // (128 B/clk, 2-way conflicts) these reads kept the LDS array busy 70 % of the kernel
            // (PMC: SQ_LDS_IDX_ACTIVE, a third of it SQ_LDS_BANK_CONFLICT).
            const float4* __restrict__ win4 = reinterpret_cast<const float4*>(__builtin_assume_aligned(win, 16));
            const float4* __restrict__ G4 = reinterpret_cast<const float4*>(__builtin_assume_aligned(G, 16));
            for (; j + 8 <= K; j += 8) {
                const float4 x0 = win4[j / 2], x1 = win4[j / 2 + 1], x2 = win4[j / 2 + 2], x3 = win4[j / 2 + 3];
                const float4 c0 = G4[j / 4], c1 = G4[j / 4 + 1];
                acc.x = fmaf(c0.x, x0.x, acc.x); acc.y = fmaf(c0.x, x0.y, acc.y);
                acc.x = fmaf(c0.y, x0.z, acc.x); acc.y = fmaf(c0.y, x0.w, acc.y);
                acc.x = fmaf(c0.z, x1.x, acc.x); acc.y = fmaf(c0.z, x1.y, acc.y);
                acc.x = fmaf(c0.w, x1.z, acc.x); acc.y = fmaf(c0.w, x1.w, acc.y);
                acc.x = fmaf(c1.x, x2.x, acc.x); acc.y = fmaf(c1.x, x2.y, acc.y);
                acc.x = fmaf(c1.y, x2.z, acc.x); acc.y = fmaf(c1.y, x2.w, acc.y);
                acc.x = fmaf(c1.z, x3.x, acc.x); acc.y = fmaf(c1.z, x3.y, acc.y);
                acc.x = fmaf(c1.w, x3.z, acc.x); acc.y = fmaf(c1.w, x3.w, acc.y);
            }
        } else {
            for (; j + 8 <= K; j += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float2 v = win[j + u];
                    const float g = G[j + u];
                    acc.x = fmaf(g, v.x, acc.x);
                    acc.y = fmaf(g, v.y, acc.y);
                }
            }
        }
        for (; j < K; ++j) {
            const float2 v = win[j];
            const float g = G[j];
            acc.x = fmaf(g, v.x, acc.x);
            acc.y = fmaf(g, v.y, acc.y);
        }
    }
    const int64_t p = pfirst + t;
    const bool posts = P.seam_post && b == P.nblocks - 1;       // the tile that writes the state the next chunk of this launch reads
    if (!fm) {
        if (t < T && p < P.Ld) {
            reinterpret_cast<float2*>(P.out)[p] = acc;
            if (P.lasty_out && p == P.Ld - 1) *P.lasty_out = acc;
        }
        if (posts) dd_seam_post(P.seam_post);
        return;
    }
    if (p == -1) acc = *P.lasty_in;
    if (t < T) yblk[t] = acc;
    __syncthreads();
    if (t < T && p >= 0 && p < P.Ld) {
        if (t > 0) {
            reinterpret_cast<float*>(P.out)[p - P.s] = dd_fm_angle(acc, yblk[t - 1]);
        }
        if (p == P.Ld - 1) *P.lasty_out = acc;
    }
    if (posts) dd_seam_post(P.seam_post);
}

__global__ void __launch_bounds__(DD_DECIM_THREADS) k_chain_decim(const DDChainParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    dd_decim_edge_tile(P, (int)blockIdx.x, smem);
}

// ============================================================================
// decimating kernel, interior tiles, persistent
// ============================================================================
// One launch-long workgroup per third of a CU (LDS bound, 3 per CU) walks the interior tiles blockIdx.x, blockIdx.x + nwg,
// ... (round 4: the device then works on one moving window of nwg tiles, and the tile loads are non-temporal -- what
// tools/ubench/stream_2to1 found for streaming kernels: C3 / C4 one-chunk passes 0.110 / 0.113 -> 0.0985 / 0.102 ms = 0.69 / 0.67 of
// 8 TB/s, profiles/r04_decim_map.txt, against a contiguous run per workgroup and plain loads) of the
// interior tiles: whole span inside the chunk, every output valid, complex64 input.  The next
// tile's samples are requested (12 x 16 B per lane) the moment the current tile has been staged
// into LDS -- into the same registers, which staging has just freed -- so they are in flight
// during the tap loop, the discriminator and both barriers, and the per-workgroup constants
// (taps in LDS, group and lane phasors) are built once per launch instead of once per tile.  NCO phase is TILE-RELATIVE: the factor exp(-j w (abs0 + ns)) is
// common to a tile, so it cancels in the discriminator (a tile recomputes the output before
// its first one, pairs never straddle tiles) and is applied to the FIR output only for
// complex output.
#define DD_DECIM_NV ((DD_DECIM_SPAN_MAX / 2 + DD_DECIM_THREADS - 1) / DD_DECIM_THREADS)
typedef float dd_v4f_a8 __attribute__((ext_vector_type(4), aligned(8)));     // 16-byte load on an 8-byte boundary

__device__ __forceinline__ void dd_decim_issue(const DDChainParams& P, int b, int nq, int t, dd_v4f_a8 (&v)[DD_DECIM_NV]) {
    const int64_t ns = (int64_t)P.off + dd_tile_pfirst(P, b) * P.M - (P.K - 1);
    const float2* __restrict__ src = reinterpret_cast<const float2*>(P.in) + ns;      // wave uniform
#pragma unroll
    for (int u = 0; u < DD_DECIM_NV; ++u) {
        int q = t + u * DD_DECIM_THREADS;
        q = q < nq ? q : nq - 1;                          // past the span: harmless re-read, never used
        v[u] = __builtin_nontemporal_load(reinterpret_cast<const dd_v4f_a8*>(src + 2 * q));
    }
}

// raw u8 input (DD_CHAIN_U8_INPUT, 2 B/sample): a 16-byte load carries eight samples (I0 Q0 I1 Q1 ...)
#define DD_DECIM_NV8 ((DD_DECIM_SPAN_MAX / 8 + DD_DECIM_THREADS - 1) / DD_DECIM_THREADS)
typedef uint32_t dd_v4u_a4 __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte load on a 4-byte boundary

__device__ __forceinline__ void dd_decim_issue_u8(const DDChainParams& P, int b, int nq8, int t, dd_v4u_a4 (&v)[DD_DECIM_NV8]) {
    const int64_t ns = (int64_t)P.off + dd_tile_pfirst(P, b) * P.M - (P.K - 1);
    const unsigned char* __restrict__ src = reinterpret_cast<const unsigned char*>(P.in) + 2 * ns;   // wave uniform
#pragma unroll
    for (int u = 0; u < DD_DECIM_NV8; ++u) {
        int q = t + u * DD_DECIM_THREADS;
        q = q < nq8 ? q : nq8 - 1;
        v[u] = __builtin_nontemporal_load(reinterpret_cast<const dd_v4u_a4*>(src + 16 * q));
    }
}

// stage one tile of raw u8 samples: widen (source.py:117-118: value - 127.5), rotate, write the LDS image
__device__ __forceinline__ void dd_decim_stage_u8(const DDChainParams& P, int nq8, int t, const dd_v4u_a4 (&v)[DD_DECIM_NV8],
                                                  float2* sx, const float2* w2, const float2 (&w1)[8]) {
    const bool nco = (P.flags & DD_CHAIN_NCO) != 0;
#pragma unroll
    for (int u = 0; u < DD_DECIM_NV8; ++u) {
        const int q = t + u * DD_DECIM_THREADS;
        if (q < nq8) {
            const float2 g = nco ? w2[(8 * q) >> 6] : make_float2(1.f, 0.f);
            const uint32_t d[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float2 xa = make_float2((float)(d[k] & 0xff) - 127.5f, (float)((d[k] >> 8) & 0xff) - 127.5f);
                float2 xb = make_float2((float)((d[k] >> 16) & 0xff) - 127.5f, (float)(d[k] >> 24) - 127.5f);
                if (nco) {
                    xa = dd_cmul(xa, dd_cmul(g, w1[2 * k]));
                    xb = dd_cmul(xb, dd_cmul(g, w1[2 * k + 1]));
                }
                *reinterpret_cast<float4*>(sx + 8 * q + 2 * k) = make_float4(xa.x, xa.y, xb.x, xb.y);
            }
        }
    }
}

template <bool U8>
__device__ __forceinline__ void dd_decim_tile(const DDChainParams& P, int b, const DDChainParams& Pn, int b_next, int nq, int t, dd_v4f_a8 (&v)[DD_DECIM_NV],
                                              dd_v4u_a4 (&v8)[DD_DECIM_NV8], const float2 (&w18)[8],
                                              float2* sx, const float2* w2, float2* yblk, const float* gl, float2 w1a, float2 w1b) {
    const int K = P.K, M = P.M, T = P.T;
    const bool nco = (P.flags & DD_CHAIN_NCO) != 0, fm = (P.flags & DD_CHAIN_FM) != 0;
    const int64_t pfirst = dd_tile_pfirst(P, b);
    float2 tilew = make_float2(1.f, 0.f);
    if (nco && !fm) {                                      // absolute phase of the tile start (table fetch issued early)
        const int64_t ns = (int64_t)P.off + pfirst * M - (K - 1);
        tilew = dd_phasor((uint64_t)(P.abs0 + ns) * P.cyc, P.nco_tbl);
    }
    if (U8) {
        dd_decim_stage_u8(P, nq, t, v8, sx, w2, w18);      // (nq counts octets here)
        if (b_next >= 0) dd_decim_issue_u8(Pn, b_next, nq, t, v8);
    } else {
        float2 g[DD_DECIM_NV];
        if (nco) {
#pragma unroll
            for (int u = 0; u < DD_DECIM_NV; ++u) {
                const int q = t + u * DD_DECIM_THREADS;
                g[u] = w2[(q < nq ? 2 * q : 0) >> 6];
            }
        }
#pragma unroll
        for (int u = 0; u < DD_DECIM_NV; ++u) {
            const int q = t + u * DD_DECIM_THREADS;
            if (q < nq) {
                float2 xa = make_float2(v[u].x, v[u].y), xb = make_float2(v[u].z, v[u].w);
                if (nco) {
                    xa = dd_cmul(xa, dd_cmul(g[u], w1a));
                    xb = dd_cmul(xb, dd_cmul(g[u], w1b));
                }
                *reinterpret_cast<float4*>(sx + 2 * q) = make_float4(xa.x, xa.y, xb.x, xb.y);
            }
        }
        if (b_next >= 0) dd_decim_issue(Pn, b_next, nq, t, v); // next tile (of this chunk or, in a multi-chunk launch, the next): in flight from here to the next staging
    }
    __syncthreads();
    float2 acc = make_float2(0.f, 0.f);
    if (t < T) {
        const float2* __restrict__ win = sx + t * M;
        int j = 0;
        if ((M & 1) == 0) {
            // the taps are wave uniform: they come through the scalar cache (a third of the tap loop's LDS reads were theirs), and a
            // multiply-add handles re and im at once; two partial sums
            typedef float dd_v2f __attribute__((ext_vector_type(2)));
            typedef const __attribute__((address_space(4))) float* dd_cfp;
            const dd_cfp Gs = (dd_cfp)(P.taps_rev + (DD_DENSE_R - 1));
            const float4* __restrict__ win4 = reinterpret_cast<const float4*>(__builtin_assume_aligned(win, 16));
            dd_v2f a0 = (dd_v2f){0.f, 0.f}, a1 = (dd_v2f){0.f, 0.f};
            for (; j + 8 <= K; j += 8) {
                const float4 x0 = win4[j / 2], x1 = win4[j / 2 + 1], x2 = win4[j / 2 + 2], x3 = win4[j / 2 + 3];
                const float c0 = Gs[j], c1 = Gs[j + 1], c2 = Gs[j + 2], c3 = Gs[j + 3], c4 = Gs[j + 4], c5 = Gs[j + 5], c6 = Gs[j + 6], c7 = Gs[j + 7];
                a0 = __builtin_elementwise_fma((dd_v2f){c0, c0}, (dd_v2f){x0.x, x0.y}, a0);
                a1 = __builtin_elementwise_fma((dd_v2f){c1, c1}, (dd_v2f){x0.z, x0.w}, a1);
                a0 = __builtin_elementwise_fma((dd_v2f){c2, c2}, (dd_v2f){x1.x, x1.y}, a0);
                a1 = __builtin_elementwise_fma((dd_v2f){c3, c3}, (dd_v2f){x1.z, x1.w}, a1);
                a0 = __builtin_elementwise_fma((dd_v2f){c4, c4}, (dd_v2f){x2.x, x2.y}, a0);
                a1 = __builtin_elementwise_fma((dd_v2f){c5, c5}, (dd_v2f){x2.z, x2.w}, a1);
                a0 = __builtin_elementwise_fma((dd_v2f){c6, c6}, (dd_v2f){x3.x, x3.y}, a0);
                a1 = __builtin_elementwise_fma((dd_v2f){c7, c7}, (dd_v2f){x3.z, x3.w}, a1);
            }
            acc.x = a0.x + a1.x; acc.y = a0.y + a1.y;
        }
        for (; j + 8 <= K; j += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float2 x = win[j + u];
                const float c = gl[j + u];
                acc.x = fmaf(c, x.x, acc.x);
                acc.y = fmaf(c, x.y, acc.y);
            }
        }
        for (; j < K; ++j) {
            const float2 x = win[j];
            const float c = gl[j];
            acc.x = fmaf(c, x.x, acc.x);
            acc.y = fmaf(c, x.y, acc.y);
        }
    }
    const int64_t p = pfirst + t;
    if (!fm) {
        if (t < T) reinterpret_cast<float2*>(P.out)[p] = dd_cmul(acc, tilew);
        __syncthreads();                                   // tap loop done everywhere before the image is overwritten
        return;
    }
    if (t < T) yblk[t] = acc;
    __syncthreads();                                       // (also: tap loop done everywhere)
    if (t > 0 && t < T) reinterpret_cast<float*>(P.out)[p - P.s] = dd_fm_angle(acc, yblk[t - 1]);
}

template <bool U8>
__global__ void __launch_bounds__(DD_DECIM_THREADS, 3) k_chain_decim_p(const DDChainParams P, int b_lo, int b_hi, int nwg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // workgroups [nwg, gridDim.x): one edge tile each (stream start with the carried history, chunk end with the
    // new tail / last sample, partial tiles) -- resident beside the persistent ones from the start, so they cost
    // neither a launch of their own nor a tail after the persistent loop
    if ((int)blockIdx.x >= nwg) {
        dd_decim_edge_tile(P, (int)blockIdx.x - nwg, smem);
        return;
    }
    const int K = P.K, M = P.M, T = P.T;
    // span, rounded up to whole load granules: sample pairs (complex64) or octets (u8)
    const int S = U8 ? (((T - 1) * M + K + (M - 1) + 7) & ~7) : (((T - 1) * M + K + (M - 1) + 1) & ~1);
    const int nq = U8 ? S / 8 : S / 2;
    float2* sx = reinterpret_cast<float2*>(smem);
    float2* w2 = sx + S + 4;
    float2* yblk = w2 + (S / 64 + 2);
    float* gl = reinterpret_cast<float*>(smem + ((sizeof(float2) * ((size_t)S + 4 + (S / 64 + 2) + DD_DECIM_THREADS) + 15) & ~(size_t)15));   // (LDS offset arithmetic: see k_chain_decim)
    const int t = threadIdx.x;
    // tiles blockIdx.x, blockIdx.x + nwg, ...: the device works on one moving window of nwg tiles (tools/ubench/stream_2to1)
    const int begin = b_lo + (int)blockIdx.x, end = b_hi, step = nwg;
    if (begin >= end) return;

    dd_v4f_a8 v[DD_DECIM_NV];
    dd_v4u_a4 v8[DD_DECIM_NV8];
    if (U8) dd_decim_issue_u8(P, begin, nq, t, v8);        // in flight while the constants are built
    else dd_decim_issue(P, begin, nq, t, v);
    for (int j = t; j < ((K + 7) & ~7); j += DD_DECIM_THREADS) gl[j] = j < K ? P.taps_rev[(DD_DENSE_R - 1) + j] : 0.f;
    float2 w1a = make_float2(1.f, 0.f), w1b = make_float2(1.f, 0.f);
    if (P.flags & DD_CHAIN_NCO) {
        for (int g = t; g < S / 64 + 1; g += DD_DECIM_THREADS) w2[g] = dd_phasor((uint64_t)g * 64 * P.cyc, P.nco_tbl);
        w1a = dd_phasor((uint64_t)((2 * t) & 63) * P.cyc, P.nco_tbl);
        w1b = dd_phasor((uint64_t)(((2 * t) & 63) + 1) * P.cyc, P.nco_tbl);
    }
    float2 w18[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        w18[k] = (U8 && (P.flags & DD_CHAIN_NCO)) ? dd_phasor((uint64_t)(((8 * t) & 63) + k) * P.cyc, P.nco_tbl) : make_float2(1.f, 0.f);
    __syncthreads();
    for (int b = begin; b < end; b += step) dd_decim_tile<U8>(P, b, P, b + step < end ? b + step : -1, nq, t, v, v8, w18, sx, w2, yblk, gl, w1a, w1b);
}

// ---- several chunks, ONE launch (dd_chain_process_chunks) -------------------------------------------------------------
// The reference's chunk loops (decode_fm.py:54-70: 2^22-sample chunks; decode_noaa.py:614-624) make one call per chunk;
// a launch per chunk costs ~7 us of kernel boundary, fill and drain around ~15 us of work (C3).  Here the persistent
// workgroups walk the CONCATENATED list of every chunk's interior tiles, and every chunk's edge tiles (its first, with
// the carried history, and its last, which writes the new state) ride along as trailing workgroups.  Each tile is
// computed exactly as in the chunk's own launch -- same tile grid per chunk, same tile-relative constants -- so the
// outputs are bit-identical to the loop's; the state a chunk hands to the next travels through device memory behind
// the seam flags above.  Per chunk: its full parameter block (edge tiles) and the few fields an interior tile needs.
struct DDSeg {
    const void* in;
    void* out;
    int64_t abs0;
    int off, s, lo, pad;
};
template <bool U8>
__global__ void __launch_bounds__(DD_DECIM_THREADS, 3) k_chain_decim_multi(const DDChainParams* __restrict__ Pc, const DDSeg* __restrict__ seg,
                                                                           const int* __restrict__ ipre, const int* __restrict__ epre, int nchunks, int nwg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if ((int)blockIdx.x >= nwg) {
        const int e = (int)blockIdx.x - nwg;
        int c = 0;
        while (c + 1 < nchunks && e >= epre[c + 1]) ++c;               // (uniform)
        const DDChainParams P = Pc[c];
        dd_decim_edge_tile(P, e - epre[c], smem);
        return;
    }
    DDChainParams P = Pc[0];                                           // K, M, T, flags, cyc, taps and tables are the same for every chunk
    const int K = P.K, M = P.M, T = P.T;
    const int S = U8 ? (((T - 1) * M + K + (M - 1) + 7) & ~7) : (((T - 1) * M + K + (M - 1) + 1) & ~1);
    const int nq = U8 ? S / 8 : S / 2;
    float2* sx = reinterpret_cast<float2*>(smem);
    float2* w2 = sx + S + 4;
    float2* yblk = w2 + (S / 64 + 2);
    float* gl = reinterpret_cast<float*>(smem + ((sizeof(float2) * ((size_t)S + 4 + (S / 64 + 2) + DD_DECIM_THREADS) + 15) & ~(size_t)15));
    const int t = threadIdx.x;
    const int n = ipre[nchunks];
    const int begin = (int)blockIdx.x, end = n, step = nwg;
    if (begin >= end) return;
    int c = 0;
    while (begin >= ipre[c + 1]) ++c;
    auto load_seg = [&](DDChainParams& Q, int cc) {
        const DDSeg g = seg[cc];
        Q.in = g.in; Q.out = g.out; Q.abs0 = g.abs0; Q.off = g.off; Q.s = g.s;
        return g.lo;
    };
    int lo = load_seg(P, c);
    DDChainParams Pn = P;
    dd_v4f_a8 v[DD_DECIM_NV];
    dd_v4u_a4 v8[DD_DECIM_NV8];
    if (U8) dd_decim_issue_u8(P, lo + (begin - ipre[c]), nq, t, v8);
    else dd_decim_issue(P, lo + (begin - ipre[c]), nq, t, v);
    for (int j = t; j < ((K + 7) & ~7); j += DD_DECIM_THREADS) gl[j] = j < K ? P.taps_rev[(DD_DENSE_R - 1) + j] : 0.f;
    float2 w1a = make_float2(1.f, 0.f), w1b = make_float2(1.f, 0.f);
    if (P.flags & DD_CHAIN_NCO) {
        for (int g = t; g < S / 64 + 1; g += DD_DECIM_THREADS) w2[g] = dd_phasor((uint64_t)g * 64 * P.cyc, P.nco_tbl);
        w1a = dd_phasor((uint64_t)((2 * t) & 63) * P.cyc, P.nco_tbl);
        w1b = dd_phasor((uint64_t)(((2 * t) & 63) + 1) * P.cyc, P.nco_tbl);
    }
    float2 w18[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        w18[k] = (U8 && (P.flags & DD_CHAIN_NCO)) ? dd_phasor((uint64_t)(((8 * t) & 63) + k) * P.cyc, P.nco_tbl) : make_float2(1.f, 0.f);
    __syncthreads();
    for (int g = begin; g < end; g += step) {
        const int b = lo + (g - ipre[c]);
        int b_next = -1, cn = c, lon = lo;
        if (g + step < end) {
            if (g + step >= ipre[c + 1]) {                            // the next tile opens the next chunk with an interior run
                do { ++cn; } while (g + step >= ipre[cn + 1]);
                lon = load_seg(Pn, cn);
            }
            b_next = lon + (g + step - ipre[cn]);
        }
        dd_decim_tile<U8>(P, b, Pn, b_next, nq, t, v, v8, w18, sx, w2, yblk, gl, w1a, w1b);
        if (cn != c) { P = Pn; c = cn; lo = lon; }
    }
}

// rare path (chunk without a kept sample) and shard priming: new tail only
__global__ void k_tail_update(const DDChainParams P) {
    const int K = P.K;
    for (int i = threadIdx.x; i < K - 1; i += blockDim.x) {
        const int64_t n = P.L - (K - 1) + i;
        float2 ph = make_float2(1.f, 0.f);
        if (P.flags & DD_CHAIN_NCO) ph = dd_phasor((uint64_t)(P.abs0 + n) * P.cyc, P.nco_tbl);
        P.tail_out[i] = dd_load_sample(P, n, ph);
    }
}

__global__ void k_fill_c64(float2* p, int n, float re, float im) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = make_float2(re, im);
}

// out[j] = angle(x[j+s] * conj(x[j+s-1])), x[-1] = *last ; s = 1 if no previous sample
__global__ void __launch_bounds__(256) k_fm(const float2* __restrict__ in, float* __restrict__ out, int64_t n_out, int s,
                                            const float2* __restrict__ last, float2* __restrict__ last_out, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_out; j += stride) {
        const int64_t p = j + s;
        const float2 cur = in[p];
        const float2 prv = (p == 0) ? *last : in[p - 1];
        out[j] = dd_fm_angle(cur, prv);
    }
    if (last_out && blockIdx.x == 0 && threadIdx.x == 0) *last_out = in[n - 1];
}
