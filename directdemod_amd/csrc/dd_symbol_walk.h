// What the Meteor-M2 QPSK and the Funcube BPSK sync detectors share (decode_meteorm2.py:229-324, decode_funcube.py:148-306: the two
// references' agc, costas and Gardner loop are the same text but for what a modulation policy M states: CAP, agc.adjust's gain cap,
// and error(cr, ci, t), costas.loop's error of the corrected sample, t the hyp table).  Included by dd_afsk.hip before dd_meteor.h
// and dd_funcube.h, built with -ffp-contract=off: every float64 operation below is the reference's, in its order, rounded on its
// own -- but for agc.adjust's magnitude, (re^2 + im^2) ** 0.5 there, which NumPy takes through pow; sqrt here, correctly rounded,
// differs from the host's pow in the last bit for about 1 in 1000 inputs, inside the trace tolerance of DESIGN.md section 5.
#pragma once

#define DD_MET_TILE 1024              // samples staged per walk step (16 KiB of LDS; 16 complex128 per lane in flight)

struct DDMeteorState {                // layout mirrored by symbolsync._STATE
    double timing, b_re, b_im, c_re, c_im, dc_re, dc_im, amean;
    double freq, phase, pmean, alpha, beta;
    int64_t lock, ctr, bidx, overflow;
};

struct DDMeteorParams {
    double P, halfP, halfP1;          // symbolPeriod, symbolPeriod / 2, symbolPeriod / 2 + 1
    double alpha_u, beta_u, alpha_l, beta_l;   // compAlphaBeta(damping, bw) and (damping, bw / 2), computed by the host
    double hyp[256];                  // costas.hypstore: np.tanh(i - 128)
};

// agc.adjust (decode_meteorm2.py:21-34, decode_funcube.py:22-35: the same but for the gain's cap, 200 and 20).  dc * 1048575 and
// inp * 180.0 are complex products with a zero imaginary part, which NumPy rounds like the component products; the complex
// quotients by a real are NumPy's Smith division, (a + b * 0) * (1 / c).
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

// one call of costas.loop (decode_meteorm2.py:58-83, decode_funcube.py:60-81): returns correctedIn, leaves the phasor it used in o
template <class M>
__device__ __forceinline__ double2 dd_sym_costas(double2 a, DDMeteorState& s, const DDMeteorParams& p, const double* __restrict__ tbl,
                                                 double2& o) {
    double sn, cs;
    sincos(s.phase, &sn, &cs);                                          // np.exp(-1j * phase) = (cos, -sin)
    o = make_double2(cs, -sn);
    const double cr = a.x * o.x - a.y * o.y, ci = a.x * o.y + a.y * o.x;
    dd_met_loop_update(M::error(cr, ci, tbl), s, p);
    return make_double2(cr, ci);
}

// The m samples from here on that are no Gardner event (timing below T, T = P/2 or P) and whose "timing += 1" can be taken at
// once: m = #{k >= 0 : fl(t + k) < T and fl(t + k + 1) < 2U}, at most room, for 1 <= t < 2U / 2 = U (U the power of two above t).
// Inside the binade [U/2, U) adding 1 is exact; the addition that crosses U rounds once to the binade's ulp g; every later one adds
// an even multiple of g (1 / g >= 2^46) inside [U, 2U), which commutes with round-half-even.  So the m steps equal fl(t + m) and
// the k-th intermediate value equals fl(t + k), which is what the two tests evaluate.  A jump ends below twice the power of two
// above the timing, whatever the symbol period, so it crosses one binade at most.
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
// tile.  Runs of plain "timing += 1" samples are taken in one step (dd_met_skip).  State carries across chunks in DDMeteorState.
// Called by a kernel of one workgroup of 128 threads.
template <class M>
__device__ __forceinline__ void dd_sym_walk(const double2* __restrict__ x, int64_t n, int64_t base, DDMeteorState* __restrict__ stp,
                                            const DDMeteorParams& prm, int64_t cap, int64_t* __restrict__ bidx,
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
                            const double2 b = dd_met_agc_cap<M::CAP>(tile[j], s);
                            s.b_re = b.x;
                            s.b_im = b.y;
                            s.bidx = base + t0 + j;
                            s.timing = t + 1.0;
                            ++j;
                        } else if (t >= prm.P) {
                            const double2 a = dd_met_agc_cap<M::CAP>(tile[j], s);
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
                const double2 c = dd_sym_costas<M>(sbuf[buf][i], s, prm, hyp, o);
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

// the end of a correlation kernel of N threads: the largest of the threads' maxima `best` at lags `bi`, the smaller lag among equal
// ones, to out[2 blockIdx.x] (the lag) and out[2 blockIdx.x + 1]
template <int N, class T>
__device__ __forceinline__ void dd_sym_first_max(T best, int bi, T* rv, int* ri, int64_t* __restrict__ out) {
    const int tid = threadIdx.x;
    rv[tid] = best;
    ri[tid] = bi;
    __syncthreads();
    for (int w = N / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const T v2 = rv[tid + w];
            const int i2 = ri[tid + w];
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

#define DD_SYM_REQUIRE(cond, who, what) /* DD_REQUIRE(cond, "<who>: <what>") */ \
    do { if (!(cond)) { dd_set_error("invalid argument: %s: %s", who, what); return DD_ERR_INVALID; } } while (0)

// dd_meteor_walk and dd_funcube_walk: the checks and the launch of one workgroup of two waves
template <class Kernel>
static int dd_sym_walk_launch(Kernel kernel, const char* who, const void* x, int64_t n, int64_t base, void* state,
                              const double* params_host, int64_t cap, int64_t* bidx, int64_t* aidx, void* agc, void* ph, void* sym,
                              void* pf, void* stream) {
    DD_SYM_REQUIRE(n >= 0 && base >= 0 && cap >= 0, who, "sizes");
    DD_SYM_REQUIRE(state != nullptr && params_host != nullptr, who, "state / params");
    if (n == 0) return DD_OK;
    DD_SYM_REQUIRE(x != nullptr && bidx != nullptr && aidx != nullptr && agc != nullptr && ph != nullptr && sym != nullptr && pf != nullptr,
                   who, "null buffer");
    DDMeteorParams p;
    memcpy(&p, params_host, sizeof(p));
    hipLaunchKernelGGL(kernel, dim3(1), dim3(128), 0, dd_stream(stream), (const double2*)x, n, base, (DDMeteorState*)state, p, cap, bidx,
                       aidx, (double2*)agc, (double2*)ph, (double2*)sym, (double2*)pf);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// the tail of dd_meteor_maxcorr and dd_funcube_maxcorr: the nbuf five-word buffer descriptors go up to a device array of the call,
// launch(that array) enqueues the correlation kernel, and the stream is drained before the array is freed
template <class Launch>
static int dd_sym_with_descriptors(const int64_t* bufs_host, int64_t nbuf, const char* who, void* stream, Launch launch) {
    DDDevBuf<int64_t> dbufs;
    DD_HIP_CHECK(dbufs.alloc((size_t)nbuf * 5));
    int rc = DD_OK;
    if (hipMemcpyAsync(dbufs, bufs_host, dbufs.bytes(), hipMemcpyHostToDevice, dd_stream(stream)) != hipSuccess) rc = DD_ERR_HIP;
    if (rc == DD_OK) {
        launch(dbufs.get());
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(dd_stream(stream)) != hipSuccess) rc = DD_ERR_HIP;
    }
    DD_SYM_REQUIRE(rc == DD_OK, who, "launch failed");
    return DD_OK;
}
