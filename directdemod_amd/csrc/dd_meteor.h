// Meteor-M2 QPSK sync detection (the reference's decode_meteorm2.getSyncs, decode_meteorm2.py:229-324), included by dd_afsk.hip
// (built with -ffp-contract=off: every float64 operation below is the reference's, in its order, rounded on its own -- but for
// agc.adjust's magnitude, (re^2 + im^2) ** 0.5 there, which NumPy takes through pow; sqrt here, correctly rounded, differs from the
// host's pow in the last bit for about 1 in 1000 inputs, inside the trace tolerance of DESIGN.md section 5).
//
//   k_meteor_mix      -- the reference's float64 mixer (offsetFreq), rounded to complex64 as there
//   k_meteor_walk     -- the per-sample Gardner timing walk with agc.adjust on the B and A samples (wave 0, which also stages
//                        the samples through LDS and jumps over runs of plain timing steps) and costas.loop on every A sample
//                        (wave 1, one tile behind, fed through LDS).  State carries across chunks in DDMeteorState.
//   k_meteor_lim      -- lim(real(x * out) / 2), lim(imag(x * out) / 2) per sample, out = the Costas phasor active at that sample
//   k_meteor_bits     -- limBin(real), limBin(imag) of each corrected symbol
//   k_meteor_minsync  -- the two 120-bit sync scores over contiguous symbol windows; symbols where either fires are candidates
//   k_meteor_maxcorr  -- |np.correlate(buffer, template, 'same')| and its first argmax, one workgroup per correlation buffer
#pragma once

#define DD_MET_TILE 1024              // samples staged per walk step (16 KiB of LDS; 16 complex128 per lane in flight)
#define DD_MET_SYNC 120               // sync bits
#define DD_MET_REP 28                 // int(2048000 / 72000): template samples per sync bit
#define DD_MET_TLEN (DD_MET_SYNC * DD_MET_REP)
#define DD_MET_MAXL 20480             // longest correlation buffer (entries): 2 * (3360 + 6721) = 20162 occur
#define DD_MET_WN (DD_MET_MAXL + DD_MET_TLEN - DD_MET_REP)

struct DDMeteorState {                // layout mirrored by qpsk._STATE
    double timing, b_re, b_im, c_re, c_im, dc_re, dc_im, amean;
    double freq, phase, pmean, alpha, beta;
    int64_t lock, ctr, bidx, overflow;
};

struct DDMeteorParams {
    double P, halfP, halfP1;          // symbolPeriod, symbolPeriod / 2, symbolPeriod / 2 + 1
    double alpha_u, beta_u, alpha_l, beta_l;   // compAlphaBeta(damping, bw) and (damping, bw / 2), computed by the host
    double hyp[256];                  // costas.hypstore: np.tanh(i - 128)
};

struct DDMeteorSync {
    uint64_t s0[2], s1[2];            // sync72khz and sync72khz1, bit i of the 120 in word i / 64
};

struct DDMeteorTemplates {
    signed char t[2][DD_MET_SYNC];    // sync2mhz and sync2mhz2 before np.repeat: 127 / -128 per bit
};

struct DDMeteorBuf {                  // a correlation buffer: samples [lo0, lo0 + n0) then [lo1, lo1 + n1), two entries each
    int64_t lo0, n0, lo1, n1, tmpl;
};

// agc.adjust (decode_meteorm2.py:21-34).  dc * 1048575 and inp * 180.0 are complex products with a zero imaginary part, which
// NumPy rounds like the component products; the complex quotients by a real are NumPy's Smith division, (a + b * 0) * (1 / c).
// (decode_funcube.py:22-35 is the same but for the gain's cap: CAP = 200 here, 20 there)
template <int CAP>
__device__ __forceinline__ double2 dd_met_agc_cap(double2 x, DDMeteorState& s) {
    s.dc_re = (s.dc_re * 1048575.0 + x.x) * (1.0 / 1048576.0);
    s.dc_im = (s.dc_im * 1048575.0 + x.y) * (1.0 / 1048576.0);
    const double ir = x.x - s.dc_re, ii = x.y - s.dc_im;
    s.amean = (s.amean * 65535.0 + sqrt(ir * ir + ii * ii)) / 65536.0;
    if (180.0 / s.amean > (double)CAP) return make_double2(ir * (double)CAP, ii * (double)CAP);
    const double scl = 1.0 / s.amean;
    return make_double2((ir * 180.0) * scl, (ii * 180.0) * scl);
}

__device__ __forceinline__ double2 dd_met_agc(double2 x, DDMeteorState& s) { return dd_met_agc_cap<200>(x, s); }

__device__ __forceinline__ double dd_met_hyp(double x, const double* __restrict__ tbl) {
    if (x > 127.0) return 1.0;
    if (x < -128.0) return -1.0;
    const int i = x == x ? (int)(x + 128.0) : 0;         // (NaN: the reference raises in int())
    return tbl[i];
}

// costas.loop from the error on (decode_meteorm2.py:66-80, decode_funcube.py:66-80): the error's running mean, the clamp, phase and
// frequency, and the lock that halves the loop bandwidth
__device__ __forceinline__ void dd_met_loop_update(double err, DDMeteorState& s, const DDMeteorParams& p) {
    s.pmean = (s.pmean * 39999.0 + fabs(err)) / 40000.0;
    if (err > 1.0) err = 1.0;
    else if (err < -1.0) err = -1.0;
    s.phase = fmod(s.phase + s.freq + s.alpha * err, 6.283185307179586);
    s.freq = s.freq + s.beta * err;
    if (!s.lock && s.pmean < 0.2) {
        s.alpha = p.alpha_l;
        s.beta = p.beta_l;
        s.lock = 1;
    } else if (s.lock && s.pmean > 0.5) {
        s.alpha = p.alpha_u;
        s.beta = p.beta_u;
        s.lock = 0;
    }
}

// one call of costas.loop (decode_meteorm2.py:58-83): returns correctedIn, leaves the phasor it used in o
__device__ __forceinline__ double2 dd_met_costas(double2 a, DDMeteorState& s, const DDMeteorParams& p, const double* __restrict__ tbl,
                                                 double2& o) {
    double sn, cs;
    sincos(s.phase, &sn, &cs);                                          // np.exp(-1j * phase) = (cos, -sin)
    o = make_double2(cs, -sn);
    const double cr = a.x * o.x - a.y * o.y, ci = a.x * o.y + a.y * o.x;
    dd_met_loop_update((ci * dd_met_hyp(cr, tbl) - cr * dd_met_hyp(ci, tbl)) / 255.0, s, p);
    return make_double2(cr, ci);
}

// The m samples from here on that are no Gardner event (timing below T, T = P/2 or P) and whose "timing += 1" can be taken at
// once: m = #{k >= 0 : fl(t + k) < T and fl(t + k + 1) < 2U}, at most room, for 1 <= t < 2U / 2 = U (U the power of two above t).
// Inside the binade [U/2, U) adding 1 is exact; the addition that crosses U rounds once to the binade's ulp g; every later one adds
// an even multiple of g (1 / g >= 2^46) inside [U, 2U), which commutes with round-half-even.  So the m steps equal fl(t + m) and
// the k-th intermediate value equals fl(t + k), which is what the two tests evaluate.
__device__ __forceinline__ int dd_met_skip(double t, double T, int room) {
    int e;
    (void)frexp(t, &e);                                                  // t = f 2^e, f in [1/2, 1): U = 2^e
    const double U2 = ldexp(1.0, e + 1);
    double est = fmin(T - t, U2 - 1.0 - t);
    int m = est <= 0.0 ? 0 : (int)fmin(ceil(est), (double)room);
    while (m > 0 && !(t + (double)(m - 1) < T && t + (double)m < U2)) --m;
    while (m < room && t + (double)m < T && t + (double)(m + 1) < U2) ++m;
    return m;
}

// Two waves.  Wave 0 stages the tiles (its lanes load the next tile into registers while lane 0 walks the current one from LDS) and
// runs the timing chain: the Gardner test, timing, agc.adjust on B and A, resync_error -- none of which reads the Costas loop.  It
// hands each tile's AGC'd A samples to wave 1 through LDS; wave 1's lane 0 runs costas.loop over them while wave 0 walks the next
// tile.  Runs of plain "timing += 1" samples are taken in one step (dd_met_skip).
__global__ void __launch_bounds__(128) k_meteor_walk(const double2* __restrict__ x, int64_t n, int64_t base, DDMeteorState* __restrict__ stp,
                                                      const DDMeteorParams prm, int64_t cap, int64_t* __restrict__ bidx,
                                                      int64_t* __restrict__ aidx, double2* __restrict__ agc, double2* __restrict__ ph,
                                                      double2* __restrict__ sym, double2* __restrict__ pf) {
    constexpr int R = DD_MET_TILE / 64;
    __shared__ double2 tile[DD_MET_TILE];
    __shared__ double2 sbuf[2][DD_MET_TILE];                            // a tile yields at most one symbol per sample
    __shared__ int64_t sbase[2];
    __shared__ int scount[2];
    __shared__ double hyp[256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 256; i += 128) hyp[i] = prm.hyp[i];
    DDMeteorState s = *stp;
    double2 pre[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = (int64_t)r * 64 + lane;
        pre[r] = (wave == 0 && i < n) ? x[i] : make_double2(0.0, 0.0);
    }
    const int64_t ntiles = (n + DD_MET_TILE - 1) / DD_MET_TILE;
    for (int64_t it = 0; it <= ntiles; ++it) {
        const int64_t t0 = it * DD_MET_TILE;
        if (wave == 0 && it < ntiles) {
#pragma unroll
            for (int r = 0; r < R; ++r) tile[r * 64 + lane] = pre[r];
        }
        __syncthreads();
        if (wave == 0) {
            if (it < ntiles) {
#pragma unroll
                for (int r = 0; r < R; ++r) {                           // next tile in flight while lane 0 walks this one
                    const int64_t i = t0 + DD_MET_TILE + (int64_t)r * 64 + lane;
                    if (i < n) pre[r] = x[i];
                }
                if (lane == 0) {
                    const int buf = (int)(it & 1);
                    const int m = (int)min((int64_t)DD_MET_TILE, n - t0);
                    int cnt = 0;
                    sbase[buf] = s.ctr;
                    int j = 0;
                    while (j < m) {
                        const double t = s.timing;
                        if (t >= prm.halfP && t < prm.halfP1) {
                            const double2 b = dd_met_agc(tile[j], s);
                            s.b_re = b.x;
                            s.b_im = b.y;
                            s.bidx = base + t0 + j;
                            s.timing = t + 1.0;
                            ++j;
                        } else if (t >= prm.P) {
                            const double2 a = dd_met_agc(tile[j], s);
                            double tt = t - prm.P;
                            const double rerr = (a.y - s.c_im) * s.b_im;
                            tt += rerr * prm.P / 2000000.0;
                            s.c_re = a.x;
                            s.c_im = a.y;
                            const int64_t k = s.ctr;
                            if (k < cap) {
                                bidx[k] = s.bidx;
                                aidx[k] = base + t0 + j;
                                agc[k] = a;
                            } else {
                                s.overflow = 1;
                            }
                            sbuf[buf][cnt++] = a;
                            s.ctr = k + 1;
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
                    scount[buf] = cnt;
                }
            }
        } else if (it > 0 && lane == 0) {
            const int buf = (int)((it - 1) & 1);
            const int cnt = scount[buf];
            const int64_t k0 = sbase[buf];
            for (int i = 0; i < cnt; ++i) {
                double2 o;
                const double2 c = dd_met_costas(sbuf[buf][i], s, prm, hyp, o);
                const int64_t k = k0 + i;
                if (k < cap) {
                    ph[k] = o;
                    sym[k] = c;
                    pf[k] = make_double2(s.phase, s.freq);
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {                                            // the timing chain's fields
        stp->timing = s.timing;
        stp->b_re = s.b_re;
        stp->b_im = s.b_im;
        stp->c_re = s.c_re;
        stp->c_im = s.c_im;
        stp->dc_re = s.dc_re;
        stp->dc_im = s.dc_im;
        stp->amean = s.amean;
        stp->ctr = s.ctr;
        stp->bidx = s.bidx;
        stp->overflow = s.overflow;
    } else if (threadIdx.x == 64) {                                    // the Costas chain's
        stp->freq = s.freq;
        stp->phase = s.phase;
        stp->pmean = s.pmean;
        stp->alpha = s.alpha;
        stp->beta = s.beta;
        stp->lock = s.lock;
    }
}

__device__ __forceinline__ int dd_met_lim(double v) {
    if (v < -128.0) return -128;
    if (v > 127.0) return 127;
    if (v > 0.0 && v < 1.0) return 1;
    if (v > -1.0 && v < 0.0) return -1;
    if (v != v) return 0;
    return (int)v;
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
    rv[tid] = best;
    ri[tid] = bi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            const int v2 = rv[tid + w], i2 = ri[tid + w];
            if (v2 > rv[tid] || (v2 == rv[tid] && i2 < ri[tid])) { rv[tid] = v2; ri[tid] = i2; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[2 * blockIdx.x] = ri[0];
        out[2 * blockIdx.x + 1] = rv[0];
    }
}

// x * exp(1j * th) in float64, rounded to complex64
__device__ __forceinline__ float2 dd_met_rotate(float2 x, double th) {
    const double c = cos(th), s = sin(th);
    const double xr = x.x, xi = x.y;
    return make_float2((float)(xr * c - xi * s), (float)(xr * s + xi * c));
}

// raw u8 pairs (x = u8 - 127.5, exact in float32) or complex64
__device__ __forceinline__ float2 dd_met_sample(const uchar2* __restrict__ raw, const float2* __restrict__ c64, int64_t k) {
    if (raw != nullptr) {
        const uchar2 r = raw[k];
        return make_float2((float)r.x - 127.5f, (float)r.y - 127.5f);
    }
    return c64[k];
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
    DD_REQUIRE(n >= 0 && base >= 0 && cap >= 0, "dd_meteor_walk: sizes");
    DD_REQUIRE(state != nullptr && params_host != nullptr, "dd_meteor_walk: state / params");
    if (n == 0) return DD_OK;
    DD_REQUIRE(x != nullptr && bidx != nullptr && aidx != nullptr && agc != nullptr && ph != nullptr && sym != nullptr && pf != nullptr,
               "dd_meteor_walk: null buffer");
    DDMeteorParams p;
    memcpy(&p, params_host, sizeof(p));
    hipLaunchKernelGGL(k_meteor_walk, dim3(1), dim3(128), 0, dd_stream(stream), (const double2*)x, n, base, (DDMeteorState*)state, p, cap,
                       bidx, aidx, (double2*)agc, (double2*)ph, (double2*)sym, (double2*)pf);
    DD_LAUNCH_CHECK();
    return DD_OK;
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
    DDMeteorBuf* dbufs = nullptr;
    DD_HIP_CHECK(hipMalloc((void**)&dbufs, (size_t)nbuf * sizeof(DDMeteorBuf)));
    int rc = DD_OK;
    if (hipMemcpyAsync(dbufs, bufs_host, (size_t)nbuf * sizeof(DDMeteorBuf), hipMemcpyHostToDevice, dd_stream(stream)) != hipSuccess) rc = DD_ERR_HIP;
    if (rc == DD_OK) {
        hipLaunchKernelGGL(k_meteor_maxcorr, dim3((unsigned)nbuf), dim3(256), 0, dd_stream(stream), (const char2*)lim,
                           (const DDMeteorBuf*)dbufs, T, out);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(dd_stream(stream)) != hipSuccess) rc = DD_ERR_HIP;
    }
    hipFree(dbufs);
    DD_REQUIRE(rc == DD_OK, "dd_meteor_maxcorr: launch failed");
    return DD_OK;
}
