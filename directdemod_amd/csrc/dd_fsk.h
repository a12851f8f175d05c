// G3RUH 9600 baud FSK: bit-timing recovery on FM-demodulated audio and the descrambler (beyond the reference; DESIGN.md section 4.20
// defines the loop operation by operation, tests/_fsk.py restates it in Python floats), included by dd_afsk.hip after
// dd_afsk_frames.h, whose k_afsk_flags_marks and k_afsk_compact finish the bit stream, and dd_symbol_walk.h (DD_SYM_REQUIRE); built
// with -ffp-contract=off.  The walk is
// the Gardner event structure of dd_symbol_walk.h on one real rail: a dc tracker and a mean-|y| normaliser run on every sample, the
// transition and the eye sample are interpolated linearly between the two samples around their instant, and the clamped error
// (eye - prev) * mid moves the timing.  + - * / comparisons and fabs only, each rounded on its own, so the device and the
// restatement agree bit for bit.  Every sample is visited (dc and am move on each), so the walk ends after n steps whatever the
// samples are: a NaN timing fires no event.
//
//   k_fsk_walk -- one wave: its lanes keep the next 1024-sample tile in flight in registers while lane 0 walks the current one
//   k_fsk_bits -- one thread per symbol: hard decision, descrambler 1 + x^12 + x^17, NRZI
#pragma once

#define DD_FSK_TILE 1024              // samples staged per walk step (8 KiB of LDS; 16 doubles per lane in flight)

struct DDFskState {                   // layout mirrored by fsk.STATE
    double t, dc, am, prev, mid, last;               // timing; the dc and mean-|y| trackers; the last eye and transition samples; a[j-1]
    int64_t ctr, overflow;
};
static_assert(sizeof(DDFskState) == 64, "DDFskState: 6 doubles, 2 int64");

struct DDFskParams {
    double P, halfP, halfP1, g;       // samples per symbol, P / 2, P / 2 + 1 (computed by the host), the loop gain
};
static_assert(sizeof(DDFskParams) == 32, "DDFskParams: 4 doubles");

__global__ void __launch_bounds__(64) k_fsk_walk(const double* __restrict__ x, int64_t n, int64_t base, DDFskState* __restrict__ stp,
                                                  const DDFskParams prm, int64_t cap, double* __restrict__ sym, int64_t* __restrict__ sidx,
                                                  double* __restrict__ tmu) {
    constexpr int R = DD_FSK_TILE / 64;
    __shared__ double tile[DD_FSK_TILE];
    const int lane = threadIdx.x;
    DDFskState s = *stp;
    double pre[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = (int64_t)r * 64 + lane;
        pre[r] = i < n ? x[i] : 0.0;
    }
    const int64_t ntiles = (n + DD_FSK_TILE - 1) / DD_FSK_TILE;
    for (int64_t it = 0; it < ntiles; ++it) {
        const int64_t t0 = it * DD_FSK_TILE;
#pragma unroll
        for (int r = 0; r < R; ++r) tile[r * 64 + lane] = pre[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {                                    // next tile in flight while lane 0 walks this one
            const int64_t i = t0 + DD_FSK_TILE + (int64_t)r * 64 + lane;
            if (i < n) pre[r] = x[i];
        }
        if (lane == 0) {
            const int m = (int)min((int64_t)DD_FSK_TILE, n - t0);
            for (int j = 0; j < m; ++j) {
                const double v = tile[j];
                s.dc = (s.dc * 4095.0 + v) / 4096.0;
                const double y = v - s.dc;
                s.am = (s.am * 1023.0 + fabs(y)) / 1024.0;
                const double a = s.am > 0.0 ? y / s.am : 0.0;
                double t = s.t;
                if (t >= prm.halfP && t < prm.halfP1) {                  // the transition, read back to the instant t = P / 2
                    s.mid = a - (t - prm.halfP) * (a - s.last);
                } else if (t >= prm.P) {                                 // the eye, read back to the instant t = P
                    const double mu = t - prm.P;
                    const double eye = a - mu * (a - s.last);
                    t = t - prm.P;
                    double e = (eye - s.prev) * s.mid;
                    if (e > 1.0) e = 1.0;
                    else if (e < -1.0) e = -1.0;
                    t = t + prm.g * e;
                    s.prev = eye;
                    const int64_t k = s.ctr;
                    if (k < cap) {
                        sym[k] = eye;
                        sidx[k] = base + t0 + j;
                        tmu[k] = t;
                    } else {
                        s.overflow = 1;
                    }
                    s.ctr = k + 1;
                }
                s.last = a;
                s.t = t + 1.0;
            }
        }
        __syncthreads();
    }
    if (lane == 0) *stp = s;
}

// r[k] = sym[k] > 0 (0 before the start, and for a NaN)
__device__ __forceinline__ int dd_fsk_hard(const double* __restrict__ sym, int64_t k) {
    return (k >= 0 && sym[k] > 0.0) ? 1 : 0;
}

// the receiver's order: descramble d[k] = r[k] ^ r[k-12] ^ r[k-17], then NRZI: bit 0 is 1, bit k is 1 where d[k] == d[k-1]
__global__ void __launch_bounds__(256) k_fsk_bits(const double* __restrict__ sym, int64_t nsym, int8_t* __restrict__ r,
                                                  int8_t* __restrict__ bits) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nsym) return;
    const int rk = dd_fsk_hard(sym, k);
    r[k] = (int8_t)rk;
    if (k == 0) { bits[0] = 1; return; }
    const int d1 = rk ^ dd_fsk_hard(sym, k - 12) ^ dd_fsk_hard(sym, k - 17);
    const int d0 = dd_fsk_hard(sym, k - 1) ^ dd_fsk_hard(sym, k - 13) ^ dd_fsk_hard(sym, k - 18);
    bits[k] = d1 == d0 ? 1 : 0;
}

// the checks and the launch of one workgroup of one wave; params_host = DDFskParams
extern "C" int dd_fsk_walk(const double* x, int64_t n, int64_t base, void* state, const double* params_host, int64_t cap, double* sym,
                           int64_t* sidx, double* tmu, void* stream) {
    DD_SYM_REQUIRE(n >= 0 && base >= 0 && cap >= 0, "dd_fsk_walk", "sizes");
    DD_SYM_REQUIRE(state != nullptr && params_host != nullptr, "dd_fsk_walk", "state / params");
    DDFskParams p;
    memcpy(&p, params_host, sizeof(p));
    DD_SYM_REQUIRE(p.P >= 2.0 && p.P <= 64.0, "dd_fsk_walk", "need 2 <= samples per symbol <= 64");     // (false for a NaN)
    DD_SYM_REQUIRE(p.halfP >= 1.0 && p.halfP <= 32.0 && p.halfP1 >= 2.0 && p.halfP1 <= 33.0 && p.g >= 0.0 && p.g <= 1.0,
                   "dd_fsk_walk", "half periods or gain");
    if (n == 0) return DD_OK;
    DD_SYM_REQUIRE(x != nullptr && sym != nullptr && sidx != nullptr && tmu != nullptr, "dd_fsk_walk", "null buffer");
    hipLaunchKernelGGL(k_fsk_walk, dim3(1), dim3(64), 0, dd_stream(stream), x, n, base, (DDFskState*)state, p, cap, sym, sidx, tmu);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// sym[nsym] -> r, bits, marks (int8[nsym]) and the start-flag positions flags[counts_host[1]], counts_host[0] = nsym.
// k_afsk_compact is one workgroup that takes nsym / 1024 passes of ten scan steps: its partial sums stay below 1024 and its carry is
// int64, so no length overflows it, and its time stays a small part of the walk's over the audio the bits came from.
extern "C" int dd_fsk_bits(const double* sym, int64_t nsym, int8_t* r, int8_t* bits, int8_t* marks, int64_t* flags, int64_t cap_flags,
                           int64_t* counts_host, void* stream) {
    DD_REQUIRE(nsym >= 0 && cap_flags >= 0 && counts_host, "dd_fsk_bits: arguments");
    counts_host[0] = counts_host[1] = 0;
    if (nsym == 0) return DD_OK;
    DD_REQUIRE(sym && r && bits && marks && (cap_flags == 0 || flags), "dd_fsk_bits: null buffer");
    hipStream_t s = dd_stream(stream);
    DDScratchLock scr;
    int rc = scr.get(64 + (size_t)nsym + 64, s);
    if (rc != DD_OK) return rc;
    int64_t* tot = (int64_t*)scr.ptr;
    int8_t* fmask = (int8_t*)(tot + 8);
    const unsigned g = (unsigned)((nsym + 255) / 256);
    hipLaunchKernelGGL(k_fsk_bits, dim3(g), dim3(256), 0, s, sym, nsym, r, bits);
    DD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_afsk_flags_marks, dim3(g), dim3(256), 0, s, (const int8_t*)bits, nsym, fmask, marks);
    DD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_afsk_compact, dim3(1), dim3(1024), 0, s, (const int8_t*)fmask, nsym, flags, cap_flags, tot);
    DD_LAUNCH_CHECK();
    int64_t nf = 0;
    DD_HIP_CHECK(hipMemcpyAsync(&nf, tot, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    counts_host[0] = nsym;
    counts_host[1] = nf;
    DD_REQUIRE(nf <= cap_flags, "dd_fsk_bits: flag list too small");
    return DD_OK;
}
