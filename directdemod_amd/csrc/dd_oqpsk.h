// OQPSK symbol recovery from IQ samples for the Meteor-M N2-x satellites (beyond the reference; DESIGN.md section 4.19 defines the
// loop operation by operation, tests/_oqpsk.py restates it in Python floats), included by dd_afsk.hip after dd_symbol_walk.h, whose
// event tests, agc.adjust (dd_met_agc_cap<200>), hyp and run skipping it reuses; built with -ffp-contract=off.  The transmitter sends
// I(t) + j Q(t - T/2): the I rail is read at the A event, the Q rail at the B event half a period later, and each rail's sample at
// the other event is its mid-transition sample for the Gardner detector.  The timing chain has to read derotated samples (the
// Gardner error of a raw staggered rail vanishes at 45 degrees of carrier phase), so timing and carrier are one dependent chain
// and the walk is one lane's.  No libm call in the loop: the phase u is kept in turns in [0, 1), wrapped by t - floor(t), and its
// phasor is a 1024-entry table value rotated by two short polynomials -- + - * / sqrt floor only, each rounded on its own, so the
// device and the restatement agree bit for bit.
//
//   k_oqpsk_walk -- one wave: its lanes keep the next 1024-sample tile in flight in registers while lane 0 walks the current one
#pragma once

#define DD_OQ_N 1024                  // phasor table entries: (cos, sin)(2 pi i / N), float64, made by the host (16 KiB of LDS)

struct DDOqpskState {                 // layout mirrored by oqpsk.STATE
    double timing, dc_re, dc_im, amean;              // Gardner timing; agc.adjust's dc and mean
    double u, freq, pmean, alpha, beta;              // the carrier loop: phase and frequency in turns (per symbol), |error| mean, gains
    double i_k, i_prev, i_mid, q_prev, q_mid, e_q;   // the pending I of symbol k, the rails' last eye and mid samples, the pending Q term
    int64_t lock, ctr, aidx, seen_a, overflow;       // aidx: the sample of the pending I; seen_a: an A event has been seen
};

__device__ __forceinline__ double dd_oq_frac(double t) {
    const double f = t - floor(t);
    return f < 1.0 ? f : 0.0;                                            // (a tiny negative t rounds to 1; no number gives 0)
}

// (cos, sin)(2 pi u), u in [0, 1): entry i = int(u N) rotated by d = (u N - i) (2 pi / N) < 0.00614 through
// 1 - d^2/2 + d^4/24 and d - d^3/6 + d^5/120 (the terms left out are below 1e-16)
__device__ __forceinline__ double2 dd_oq_phasor(double u, const double2* __restrict__ tab) {
    const double t = u * 1024.0;
    const int i = t >= 0.0 ? (int)fmin(t, 1023.0) : 0;
    const double d = (t - (double)i) * (6.283185307179586 / 1024.0);
    const double d2 = d * d;
    const double pc = 1.0 - d2 * (0.5 - d2 * (1.0 / 24.0));
    const double ps = d * (1.0 - d2 * ((1.0 / 6.0) - d2 * (1.0 / 120.0)));
    const double2 e = tab[i];
    return make_double2(e.x * pc - e.y * ps, e.y * pc + e.x * ps);
}

__global__ void __launch_bounds__(64) k_oqpsk_walk(const double2* __restrict__ x, int64_t n, int64_t base, DDOqpskState* __restrict__ stp,
                                                    const DDMeteorParams prm, const double2* __restrict__ table, int64_t cap,
                                                    int64_t* __restrict__ bidx, int64_t* __restrict__ aidx, double2* __restrict__ sym,
                                                    double2* __restrict__ uf) {
    constexpr int R = DD_MET_TILE / 64;
    __shared__ double2 tile[DD_MET_TILE];
    __shared__ double2 tab[DD_OQ_N];
    __shared__ double hyp[256];
    const int lane = threadIdx.x;
    for (int i = lane; i < DD_OQ_N; i += 64) tab[i] = table[i];
    for (int i = lane; i < 256; i += 64) hyp[i] = prm.hyp[i];
    DDOqpskState s = *stp;
    DDMeteorState ag;                                                    // dd_met_agc_cap reads and writes these three
    ag.dc_re = s.dc_re;
    ag.dc_im = s.dc_im;
    ag.amean = s.amean;
    double2 pre[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = (int64_t)r * 64 + lane;
        pre[r] = i < n ? x[i] : make_double2(0.0, 0.0);
    }
    const int64_t ntiles = (n + DD_MET_TILE - 1) / DD_MET_TILE;
    for (int64_t it = 0; it < ntiles; ++it) {
        const int64_t t0 = it * DD_MET_TILE;
#pragma unroll
        for (int r = 0; r < R; ++r) tile[r * 64 + lane] = pre[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {                                    // next tile in flight while lane 0 walks this one
            const int64_t i = t0 + DD_MET_TILE + (int64_t)r * 64 + lane;
            if (i < n) pre[r] = x[i];
        }
        if (lane == 0) {
            const int m = (int)min((int64_t)DD_MET_TILE, n - t0);
            int j = 0;
            while (j < m) {
                const double t = s.timing;
                if (t >= prm.halfP && t < prm.halfP1) {                  // B: the Q rail's eye, the I rail's transition
                    const double2 a = dd_met_agc_cap<200>(tile[j], ag);
                    const double2 o = dd_oq_phasor(s.u, tab);
                    const double re = a.x * o.x + a.y * o.y, im = a.y * o.x - a.x * o.y;      // a * (cos, -sin)
                    s.i_mid = re;
                    if (s.seen_a) {
                        s.e_q = (im - s.q_prev) * s.q_mid;
                        s.q_prev = im;
                        double err = (im * dd_met_hyp(s.i_k, hyp) - s.i_k * dd_met_hyp(im, hyp)) / 255.0;
                        s.pmean = (s.pmean * 39999.0 + fabs(err)) / 40000.0;
                        if (err > 1.0) err = 1.0;
                        else if (err < -1.0) err = -1.0;
                        s.u = dd_oq_frac((s.u + s.freq * 0.5) + s.alpha * err);
                        s.freq = s.freq + s.beta * err;
                        if (!s.lock && s.pmean < 0.2) {
                            s.alpha = prm.alpha_l;
                            s.beta = prm.beta_l;
                            s.lock = 1;
                        } else if (s.lock && s.pmean > 0.5) {
                            s.alpha = prm.alpha_u;
                            s.beta = prm.beta_u;
                            s.lock = 0;
                        }
                        const int64_t k = s.ctr;
                        if (k < cap) {
                            bidx[k] = base + t0 + j;
                            aidx[k] = s.aidx;
                            sym[k] = make_double2(s.i_k, im);
                            uf[k] = make_double2(s.u, s.freq);
                        } else {
                            s.overflow = 1;
                        }
                        s.ctr = k + 1;
                    }
                    s.timing = t + 1.0;
                    ++j;
                } else if (t >= prm.P) {                                 // A: the I rail's eye, the Q rail's transition
                    const double2 a = dd_met_agc_cap<200>(tile[j], ag);
                    const double2 o = dd_oq_phasor(s.u, tab);
                    const double re = a.x * o.x + a.y * o.y, im = a.y * o.x - a.x * o.y;
                    s.i_k = re;
                    s.q_mid = im;
                    const double e_i = (re - s.i_prev) * s.i_mid;
                    s.i_prev = re;
                    const double tt = (t - prm.P) + ((e_i + s.e_q) * prm.P) / 2000000.0;      // both Gardner terms, here only
                    s.e_q = 0.0;
                    s.u = dd_oq_frac(s.u + s.freq * 0.5);
                    s.seen_a = 1;
                    s.aidx = base + t0 + j;
                    s.timing = tt + 1.0;
                    ++j;
                } else {
                    const int mm = t >= 1.0 ? dd_met_skip(t, t < prm.halfP ? prm.halfP : prm.P, m - j) : 0;
                    if (mm > 0) {
                        s.timing = t + (double)mm;
                        j += mm;
                    } else {
                        s.timing = t + 1.0;
                        ++j;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        s.dc_re = ag.dc_re;
        s.dc_im = ag.dc_im;
        s.amean = ag.amean;
        *stp = s;
    }
}

// the checks and the launch of one workgroup of one wave; table = DD_OQ_N (cos, sin) pairs in device memory
extern "C" int dd_oqpsk_walk(const void* x, int64_t n, int64_t base, void* state, const double* params_host, const void* table,
                             int64_t cap, int64_t* bidx, int64_t* aidx, void* sym, void* uf, void* stream) {
    DD_SYM_REQUIRE(n >= 0 && base >= 0 && cap >= 0, "dd_oqpsk_walk", "sizes");
    DD_SYM_REQUIRE(state != nullptr && params_host != nullptr && table != nullptr, "dd_oqpsk_walk", "state / params / table");
    if (n == 0) return DD_OK;
    DD_SYM_REQUIRE(x != nullptr && bidx != nullptr && aidx != nullptr && sym != nullptr && uf != nullptr, "dd_oqpsk_walk", "null buffer");
    DDMeteorParams p;
    memcpy(&p, params_host, sizeof(p));
    hipLaunchKernelGGL(k_oqpsk_walk, dim3(1), dim3(64), 0, dd_stream(stream), (const double2*)x, n, base, (DDOqpskState*)state, p,
                       (const double2*)table, cap, bidx, aidx, (double2*)sym, (double2*)uf);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
