// getAccurateSync's windows, batched (decode_noaa.py:808-880): dd_noaa_sync_windows(_multi), and dd_noaa_prepare.  The
// windows' envelope is ONE stage (sync_envelope_stage: own transform, the library's padded real transforms, the library's length-N
// complex pair), which the production entry runs per batch and dd_debug_sync_envelope runs alone; likewise the envelope's pre-filter
// (sync_prefilter_stage, dd_debug_sync_prefilter) and the scan / correlation / peak tail (sync_tail_stage, dd_debug_sync_tail).  Its Hilbert-kernel spectra and
// the padded convolution's body are those of dd_audio_envelope.h; the scan and the needle's run table those of dd_audio_xcorr.h.
// One of the six parts of dd_audio.hip (one translation unit: the parts share the plan cache, the float64 transform and the scratch
// buffers of dd_audio.hip and are included there, each using only the parts before it).  Internal; not a stand-alone header.
// ---------------------------------------------------------------- 8f-2: accurate-sync windows, batched
// getAccurateSync (decode_noaa.py:808-880) cuts one +-width window of IQ samples around every crude sync
// and runs, per window:  offsetFreq -> filter(blackmanHarris(151, zeroPhase)) -> demod_fm -> demod_am
// (:852) and then __correlateAndFindPeaks with the zero-phase hamming(492) pre-filter (:677-767, :853).
// The windows are independent and equally long, so the whole chain runs once over [windows][samples]
// arrays: a dozen launches per batch instead of ~40 launches, ~25 allocations and 8 host round trips per
// window.  Each stage is the arithmetic of the per-window entry points (same kernels or the same
// device functions); only the prefix sums and the batched FFT plan may
// round differently, at the 1e-13 level of the correlation.
#include "dd_chain_kernels.h"
#include "dd_filtfilt_kernels.h"

template <bool U8>
__global__ void __launch_bounds__(256) k_sync_front(const void* __restrict__ iq, const int64_t* __restrict__ starts, int64_t L,
                                                    uint64_t cyc, const float2* __restrict__ tbl, float2* __restrict__ X) {
    // four samples per lane: four loads in flight, 32 contiguous bytes stored
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (i0 >= L) return;
    const int64_t g = starts[blockIdx.y] + i0;
    float2 v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t ge = i0 + e < L ? g + e : g;
        if (U8) {
            const uchar2 u = reinterpret_cast<const uchar2*>(iq)[ge];
            v[e] = make_float2((float)u.x - 127.5f, (float)u.y - 127.5f);
        } else {
            v[e] = reinterpret_cast<const float2*>(iq)[ge];
        }
    }
    float2* out = X + (int64_t)blockIdx.y * L + i0;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = dd_cmul(v[e], dd_phasor((uint64_t)(i0 + e) * cyc, tbl));      // sample index restarts per window (Q5)
    if (i0 + 3 < L && ((reinterpret_cast<uintptr_t>(out) & 15) == 0)) {
        reinterpret_cast<float4*>(out)[0] = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
        reinterpret_cast<float4*>(out)[1] = make_float4(v[2].x, v[2].y, v[3].x, v[3].y);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (i0 + e < L) out[e] = v[e];
    }
}

// demod_fm (stateless) straight into the FFT buffer: W[b][j] = (angle(Y[j+1] conj Y[j]), 0)
__global__ void __launch_bounds__(256) k_sync_fm(const float2* __restrict__ Y, int64_t L, double2* __restrict__ W) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= L - 1) return;
    const float2* y = Y + (int64_t)blockIdx.y * L;
    W[(int64_t)blockIdx.y * (L - 1) + j] = make_double2((double)dd_fm_angle(y[j + 1], y[j]), 0.0);
}

// Peak pick of one window (decode_noaa.py:713-762) when the window is shorter than the 0.45 s group
// distance: expectedPeaks K = 2, every candidate falls in one group, and the pick is the first index of
// the maximum provided it exceeds the threshold.  Also the two "extras": peak height and the mean of the
// next needle-length of the envelope.  The correlation values are reduced where they are produced (first
// maximum, two largest, two smallest per tile of 1024 outputs); the correlation array itself is never stored.
// A window whose maximum does not exceed the threshold (every correlation the same value), or whose correlation holds a NaN (a NaN
// sample; a stretch without energy as long as the needle, 0 / 0) -- where the reference would append None or sort NaNs -- comes back
// as (INT64_MIN, NaN, NaN); a peak with i + 2 m >= n has its height and a NaN mean (:755).
struct DDPk {
    double m1, m2, l1, l2;
    int64_t i1;
    int nan;
};
__device__ __forceinline__ DDPk dd_pk_merge(const DDPk& a, const DDPk& b) {
    DDPk r;
    if (b.m1 > a.m1 || (b.m1 == a.m1 && b.i1 < a.i1)) {
        r.m1 = b.m1; r.i1 = b.i1; r.m2 = fmax(a.m1, b.m2);
    } else {
        r.m1 = a.m1; r.i1 = a.i1; r.m2 = fmax(a.m2, b.m1);
    }
    if (b.l1 < a.l1) { r.l1 = b.l1; r.l2 = fmin(a.l1, b.l2); }
    else { r.l1 = a.l1; r.l2 = fmin(a.l2, b.l1); }
    r.nan = a.nan | b.nan;
    return r;
}
__device__ __forceinline__ DDPk dd_pk_shfl(const DDPk& a, int d) {
    DDPk r;
    r.m1 = __shfl_down(a.m1, d); r.m2 = __shfl_down(a.m2, d);
    r.l1 = __shfl_down(a.l1, d); r.l2 = __shfl_down(a.l2, d);
    r.i1 = __shfl_down(a.i1, d); r.nan = __shfl_down(a.nan, d);
    return r;
}
__device__ __forceinline__ DDPk dd_pk_empty() {
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    DDPk a = {-inf, -inf, inf, inf, INT64_MAX, 0};
    return a;
}

// Normalised correlation in the run-length form (k_xcorr_runs_n, dd_audio_xcorr.h) of a batch of windows, reduced per tile.
// Workgroups are dealt to the XCDs window by window (dispatch is round-robin over the 8 XCDs), so the ~14
// reads of every prefix-sum element come out of one XCD's L2.
#define DD_XC_TILE 1024
// (Tried in round 4 and not kept, same call, 64 windows: the run table in scalar registers with the loop unrolled -- all 64
// look-ups of a lane in flight, 169 registers, 2 waves per SIMD -- 129 us; the look-ups staged in LDS along the comb of the
// needle's run-boundary grid (984 / 492 samples: 1.5-2.7 loads from L2 per output instead of 16, but 32 KB of LDS per wave =
// 5 waves per CU) 107-162 us; this loop, 8 waves per SIMD walking the runs in step so that neighbouring workgroups read
// neighbouring prefix sums at the same time: 80 us.  Two runs' look-ups in flight (66 registers, 7 waves): 79-82 against 81-86, noise;
// fewer workgroups per CU (so that one XCD's workgroups stay inside one window's prefix sums): 87 us at 7 per CU, 98 at 4, 146 at 2.
// profiles/r04_noaa_timeline.txt)
__global__ void __launch_bounds__(256) k_xcorr_runs_pk(const double* __restrict__ P, const double* __restrict__ Q, int64_t n, int m,
                                                       const DDRuns2 R2, const int* __restrict__ group, int tiles, int nwin, DDPk* __restrict__ part) {
    __shared__ DDPk sw[4];
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int win = (k / tiles) * 8 + xcd, tile = k % tiles;
    if (win >= nwin) return;
    const int gsel = group ? __builtin_amdgcn_readfirstlane(group[win]) : 0;        // which needle this window is searched for
    const DDRuns& R = R2.r[gsel];
    const double vv = R2.vv[gsel];
    P += (int64_t)win * (n + 1);
    Q += (int64_t)win * (n + 1);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    auto at = [&](const double* S, int64_t x) { return S[x < 0 ? 0 : (x > n ? n : x)]; };
    const double qn = 1e-13 * Q[n];
    // four outputs per lane, the run loop outermost: the four lookups of a run boundary are independent loads
    constexpr int NJ = DD_XC_TILE / 256;
    int64_t a0[NJ];
    double c[NJ], lo[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        a0[j] = (int64_t)tile * DD_XC_TILE + j * 256 + t + (m - 1) / 2 - (m - 1);
        c[j] = 0.0;
        lo[j] = at(P, a0[j]);
    }
    for (int r = 0; r < R.nr; ++r) {
        double hi[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) hi[j] = at(P, a0[j] + R.start[r + 1]);
#pragma unroll
        for (int j = 0; j < NJ; ++j) { c[j] = fma(R.val[r], hi[j] - lo[j], c[j]); lo[j] = hi[j]; }
    }
    DDPk a = dd_pk_empty();
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int64_t i = (int64_t)tile * DD_XC_TILE + j * 256 + t;
        double e = at(Q, a0[j] + m) - at(Q, a0[j]);
        double cc = c[j];
        if (!(e > qn)) { cc = 0.0; e = 0.0; }
        const double x = cc / sqrt(e * vv);
        if (i < n) {
            DDPk bq = {x, -inf, x, inf, i, (x != x) ? 1 : 0};
            a = dd_pk_merge(a, bq);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a = dd_pk_merge(a, dd_pk_shfl(a, d));
    if (lane == 0) sw[wv] = a;
    __syncthreads();
    if (t == 0) part[(int64_t)win * tiles + tile] = dd_pk_merge(dd_pk_merge(sw[0], sw[1]), dd_pk_merge(sw[2], sw[3]));
}

__global__ void __launch_bounds__(256) k_sync_peak(const DDPk* __restrict__ part, int tiles, const double* __restrict__ env, int64_t n, int m,
                                                   int64_t* __restrict__ peak, double* __restrict__ height, double* __restrict__ tsync) {
    __shared__ DDPk sw[4];
    __shared__ double ssum[4];
    const double* ev = env + (int64_t)blockIdx.x * n;
    part += (int64_t)blockIdx.x * tiles;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    DDPk a = dd_pk_empty();
    for (int k = t; k < tiles; k += 256) a = dd_pk_merge(a, part[k]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a = dd_pk_merge(a, dd_pk_shfl(a, d));
    if (lane == 0) sw[wv] = a;
    __syncthreads();
    a = dd_pk_merge(dd_pk_merge(sw[0], sw[1]), dd_pk_merge(sw[2], sw[3]));
    double avgpk = (0.0 + a.m2 + a.m1) / 2.0;                       // mean of the K = 2 largest (:717-721)
    avgpk -= 0.25 * (avgpk - (0.0 + a.l1 + a.l2) / 2.0);            // NOAA_PEAKHEIGHTWIGGLE (:723)
    const bool found = !a.nan && a.m1 > avgpk;
    const int64_t i = a.i1 - m / 2;                                 // :749
    const bool tail = found && i + 2 * (int64_t)m < n;              // :755
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (tail) {
        int64_t j = i + m + t;
        const int64_t end = i + 2 * (int64_t)m;
        for (; j + 768 < end; j += 1024) { s0 += ev[j]; s1 += ev[j + 256]; s2 += ev[j + 512]; s3 += ev[j + 768]; }
        for (; j < end; j += 256) s0 += ev[j];
    }
    double sacc = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sacc += __shfl_down(sacc, d);
    if (lane == 0) ssum[wv] = sacc;
    __syncthreads();
    if (t == 0) {
        const double tot = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
        peak[blockIdx.x] = found ? i : INT64_MIN;
        height[blockIdx.x] = found ? a.m1 : __longlong_as_double(0x7ff8000000000000ll);
        tsync[blockIdx.x] = tail ? tot / (double)m : __longlong_as_double(0x7ff8000000000000ll);
    }
}

// demod_fm into the zero-padded real image of the envelope's cyclic convolution (the library's padded real transforms; dd_audio_envelope.h)
__global__ void __launch_bounds__(256) k_sync_fm_pad(const float2* __restrict__ Y, int64_t L, double* __restrict__ XR, int64_t M) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const float2* y = Y + (int64_t)blockIdx.y * L;
    XR[(int64_t)blockIdx.y * M + j] = j < L - 1 ? (double)dd_fm_angle(y[j + 1], y[j]) : 0.0;
}

// The envelope stage of a batch of b windows: X [b][L] filtered IQ -> ENV [b][L - 1] = abs(hilbert(angle(X[n+1] conj X[n]))).
// route 0: dd_hconv_kernels.h (hc_length_ok(M); W: c128 [(b+1)/2][M], two windows per image), route 1 ("lib"): the library's padded real
// transforms (W as f64 [b][M], SP: c128 [b][M/2 + 1], YR: f64 [b][M]), route 2 ("fft"): the library's length-(L-1) complex pair in W
// (c128 [b][L - 1]).  HH: hilbert_spectrum(L - 1, M, false) for routes 0 and 1
static int sync_envelope_stage(int route, const float2* X, int64_t L, int b, int64_t M, const double2* HH, double2* W, double2* SP, double* YR,
                               double* ENV, hipStream_t s) {
    const int64_t L2 = L - 1;
    if (route == 0) return hc_envelope(M, X, L, b, HH + (M / 2 + 1), W, ENV, s);
    if (route == 1) {
        hipLaunchKernelGGL(k_sync_fm_pad, dim3(grid1(M), b), dim3(256), 0, s, X, L, (double*)W, M);
        return envelope_padded((double*)W, SP, YR, HH, M, L2, b, ENV, s);
    }
    const dim3 gL2(grid1(L2), b);
    hipfftHandle plan;
    const int rc = get_plan(&plan, HIPFFT_Z2Z, L2, b, s);
    if (rc != DD_OK) return rc;
    hipLaunchKernelGGL(k_sync_fm, gL2, dim3(256), 0, s, X, L, W);
    DD_FFT_CHECK(hipfftExecZ2Z(plan, (hipfftDoubleComplex*)W, (hipfftDoubleComplex*)W, HIPFFT_FORWARD));
    hipLaunchKernelGGL(k_hilbert_mask_b, gL2, dim3(256), 0, s, W, L2);
    DD_FFT_CHECK(hipfftExecZ2Z(plan, (hipfftDoubleComplex*)W, (hipfftDoubleComplex*)W, HIPFFT_BACKWARD));
    hipLaunchKernelGGL(k_cplx_abs_b, gL2, dim3(256), 0, s, W, ENV, L2, 1.0 / (double)L2);
    return DD_OK;
}

// The envelope pre-filter of a batch of b windows: ENV [b][n] -> H [b][n] = filtfilt(taps, [1], ENV) (decode_noaa.py:677).  fit != NULL:
// the prefix-sum form of a cosine series (dd_filtfilt_kernels.h; tab: dd_cos_table(K, fit->Q) on the device), else the tiled direct form
// over `taps` (device, float64).  F1: f64 [b][n + 6 K], the first pass.
static int sync_prefilter_stage(const double* ENV, int64_t n, int b, int K, const DDCosFit* fit, const double2* tab, const double* taps,
                                double* F1, double* H, hipStream_t s) {
    if (fit) return dd_filtfilt_cos_launch(ENV, n, F1, H, n, n, K, *fit, tab, b, s);
    dd_filtfilt_launch<double>(ENV, n, F1, H, n, n, K, taps, b, s);
    return DD_OK;
}

// The correlation/peak tail of a batch of b windows: hay [b][n] (the pre-filtered envelope) is searched for its window's needle (group:
// device, one needle index per window, or NULL), ENV [b][n] gives the post-sync mean -> peak / height / tsync [b] on the device.
// PQ: f64 [2][b][n + 1], the prefix sums of hay and hay^2; work: sync_tail_work_bytes(n, b), the scan's tile sums and the per-tile peak records.
static size_t sync_tail_work_bytes(int64_t n, int b) {
    const size_t stiles = (size_t)((n + DD_SCAN_TILE - 1) / DD_SCAN_TILE), xtiles = (size_t)((n + DD_XC_TILE - 1) / DD_XC_TILE);
    return sizeof(double2) * b * stiles + sizeof(DDPk) * b * xtiles;
}
static void sync_tail_stage(const double* hay, const double* ENV, int64_t n, int b, int m, const DDRuns2& R2, const int* group,
                            double* PQ, void* work, int64_t* peak, double* height, double* tsync, hipStream_t s) {
    double* P = PQ;
    double* Q = P + (size_t)b * (n + 1);
    const int stiles = (int)((n + DD_SCAN_TILE - 1) / DD_SCAN_TILE), xtiles = (int)((n + DD_XC_TILE - 1) / DD_XC_TILE);
    double2* spart = (double2*)work;
    DDPk* ppart = (DDPk*)(spart + (size_t)b * stiles);
    hipLaunchKernelGGL(k_scan_part, dim3(stiles, b), dim3(256), 0, s, hay, n, stiles, spart);
    hipLaunchKernelGGL(k_scan_final, dim3(stiles, b), dim3(256), 0, s, hay, n, stiles, spart, P, Q);
    hipLaunchKernelGGL(k_xcorr_runs_pk, dim3(8 * ((b + 7) / 8) * xtiles), dim3(256), 0, s, P, Q, n, m, R2, group, xtiles, b, ppart);
    hipLaunchKernelGGL(k_sync_peak, dim3(b), dim3(256), 0, s, ppart, xtiles, ENV, n, m, peak, height, tsync);
}

// What dd_noaa_crude_tail will need for `n` audio samples in blocks of `block` -- the Hilbert-kernel spectra of the block and of the ragged
// last block (host transforms: ~20 ms) and the transform's twiddle tables -- built ahead of time.  noaa_sync calls this from a thread of
// its own when the decoder object is created, so that it overlaps the upload of the recording and the audio chain; the result sits in the
// cache the crude tail looks in.  Harmless when the lengths turn out different (the crude tail builds what it needs).
extern "C" int dd_noaa_prepare(int64_t n, int64_t block, int64_t window, void* stream) {
    DD_REQUIRE(n >= 0 && block >= 2 && window >= 0, "arguments");
    (void)stream;
    static const char* tenv = getenv("DD_CRUDE_TRACE");              // tools: host-side time stamps, to stderr
    const auto t0 = std::chrono::steady_clock::now();
    int dev = 0;
    DD_HIP_CHECK(hipGetDevice(&dev));
    struct Job { std::pair<int, int64_t> key; int64_t len, M; bool split; };
    std::vector<Job> jobs;
    if (n >= 1) {
        const DDEnvWalk w = envelope_plan(n, block);
        for (const DDEnvGroup* g : {&w.full, &w.last})
            if (g->route == DD_ENV_OWN_SPLIT || g->route == DD_ENV_OWN_PLAIN) {
                const bool split = g->route == DD_ENV_OWN_SPLIT;
                jobs.push_back(Job{hilbert_key(dev, g->N, g->M, split), g->N, g->M, split});
            }
    }
    if (window >= 4) {                                               // dd_noaa_sync_windows: L2 = window - 1 angles, cyclic length >= 2 L2 + 2
        const int64_t L2 = window - 1;
        int64_t M = 1;
        while (M < 2 * L2 + 2) M <<= 1;
        if (hc_length_ok(M)) jobs.push_back(Job{hilbert_key(dev, L2, M, false), L2, M, false});
    }
    int built = 0;
    for (const Job& j : jobs) {
        {
            std::lock_guard<std::mutex> lk(g_sync_mu);
            if (g_hilb.count(j.key)) continue;                       // on the device already
        }
        if (hilb_host_find(j.key)) continue;
        // closed forms and a radix-2 transform, outside every lock, no device call: in a fresh process the runtime is still busy with its
        // first copy (~100 ms, _hip.require_gpu's warm-up thread) and this thread beside it
        std::vector<double2> h;
        hilbert_host(j.len, j.M, j.split, h);
        (void)hilb_host_keep(j.key, h);
        ++built;
    }
    if (tenv) fprintf(stderr, "noaa prepare host us (n %ld, window %ld): %d spectra built in %ld\n", (long)n, (long)window, built,
                      (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
    return DD_OK;
}

// diagnostic (no GPU needed): is this tap set a cosine series b[k] = sum_q a[q] cos(2 pi q k / (K - 1)), q <= 3, as the windows of
// filters.py:101-226 are?  Returns 1 and fills a[0..3], *Q (highest harmonic) when the zero-phase filter of the accurate-sync
// windows takes the prefix-sum form for it, 0 when it keeps the tiled direct form.
extern "C" int dd_debug_cos_fit(const double* taps_host, int K, double* a_out, int* Q_out) {
    DD_REQUIRE(taps_host && K >= 1 && a_out && Q_out, "arguments");
    DDCosFit f;
    if (!dd_cos_fit(taps_host, K, &f) || !dd_fc_ok(K, f.Q)) return 0;
    for (int q = 0; q < 4; ++q) a_out[q] = f.a[q];
    *Q_out = f.Q;
    return 1;
}

// diagnostic: the envelope stage of dd_noaa_sync_windows alone.  X: device c64 [nwin][L] (what the zero-phase FIR leaves),
// env: device f64 [nwin][L - 1] = abs(hilbert(angle(X[n+1] conj X[n]))).  route 0: dd_hconv_kernels.h (needs the padded length
// 2^17 or 2^18, i.e. 32 768 < L <= 131 072; DD_ERR_INVALID otherwise), route 1: the library's padded real transforms.  Synchronises.
extern "C" int dd_debug_sync_envelope(const void* X_dev, int64_t L, int nwin, int route, double* env_dev, void* stream) {
    DD_REQUIRE(X_dev && env_dev && nwin >= 1 && L >= 4 && L < ((int64_t)1 << 30) && (route == 0 || route == 1), "arguments");
    const int64_t L2 = L - 1;
    int64_t M = 1;
    while (M < 2 * L2 + 2) M <<= 1;
    DD_REQUIRE(route == 1 || hc_length_ok(M), "route 0 needs 32768 < L <= 131072");
    const int64_t nb = M / 2 + 1;
    hipStream_t s = dd_stream(stream);
    std::lock_guard<std::mutex> lk(g_sync_mu);
    const double2* HH = nullptr;
    int rc = hilbert_spectrum(L2, M, false, &HH, s);
    if (rc != DD_OK) return rc;
    DDDevBuf<char> buf;
    const size_t bW = sizeof(double2) * (size_t)((nwin + 1) / 2) * M, bSP = sizeof(double2) * (size_t)nwin * nb, bYR = sizeof(double) * (size_t)nwin * M;
    DD_HIP_CHECK(buf.alloc(bW + (route ? bSP + bYR : 0)));
    rc = sync_envelope_stage(route, (const float2*)X_dev, L, nwin, M, HH, (double2*)buf.get(), (double2*)(buf + bW), (double*)(buf + bW + bSP), env_dev, s);
    hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(s);         // (before buf is freed: every return is behind it)
    if (rc != DD_OK) return rc;
    if (e1 != hipSuccess || e2 != hipSuccess) { dd_set_error("dd_debug_sync_envelope: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2)); return DD_ERR_HIP; }
    return DD_OK;
}

// diagnostic: the envelope pre-filter of dd_noaa_sync_windows alone (sync_prefilter_stage).  x: device f64 [nwin][n] -> out: device f64
// [nwin][n] = filtfilt(taps, [1], x).  route 0: the prefix-sum form of a cosine series (DD_ERR_UNSUPPORTED when the taps are none, or
// too long for it), route 1: the tiled direct form on the same taps.  n <= 3 K is the batch's own error.  Synchronises.
extern "C" int dd_debug_sync_prefilter(const double* x_dev, int64_t n, int nwin, const double* taps_host, int K, int route,
                                       double* out_dev, void* stream) {
    DD_REQUIRE(x_dev && out_dev && taps_host && nwin >= 1 && K >= 1 && n >= 1 && n < ((int64_t)1 << 30) && (route == 0 || route == 1), "arguments");
    if (n <= 3 * (int64_t)K) {
        dd_set_error("The length of the input vector x must be greater than padlen, which is %d.", 3 * K);
        return DD_ERR_INVALID;
    }
    DDCosFit fit;
    std::vector<double2> tabh(1);
    if (route == 0) {
        if (!dd_cos_fit(taps_host, K, &fit) || !dd_fc_ok(K, fit.Q)) {
            dd_set_error("dd_debug_sync_prefilter: the prefix-sum form does not take these %d taps", K);
            return DD_ERR_UNSUPPORTED;
        }
        dd_cos_table(K, fit.Q, tabh);
    } else if (!dd_ff_tiled_ok(K, 8)) {
        dd_set_error("dd_noaa_sync_windows: filter too long for the tiled zero-phase kernel");
        return DD_ERR_INVALID;
    }
    hipStream_t s = dd_stream(stream);
    std::lock_guard<std::mutex> lk(g_sync_mu);
    DDDevBuf<double> taps, F1;
    DDDevBuf<double2> tab;
    DD_HIP_CHECK(taps.alloc((size_t)K));
    DD_HIP_CHECK(tab.alloc(tabh.size()));
    DD_HIP_CHECK(F1.alloc((size_t)nwin * (size_t)(n + 6 * (int64_t)K)));
    hipError_t e0 = hipMemcpyAsync(taps.get(), taps_host, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, s);
    if (e0 == hipSuccess) e0 = hipMemcpyAsync(tab.get(), tabh.data(), sizeof(double2) * tabh.size(), hipMemcpyHostToDevice, s);
    int rc = DD_OK;
    if (e0 == hipSuccess) rc = sync_prefilter_stage(x_dev, n, nwin, K, route == 0 ? &fit : nullptr, tab.get(), taps.get(), F1.get(), out_dev, s);
    hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(s);         // (before the buffers are freed: every return is behind it)
    if (rc != DD_OK) return rc;
    if (e0 != hipSuccess || e1 != hipSuccess || e2 != hipSuccess) {
        dd_set_error("dd_debug_sync_prefilter: %s", hipGetErrorString(e0 != hipSuccess ? e0 : (e1 != hipSuccess ? e1 : e2)));
        return DD_ERR_HIP;
    }
    return DD_OK;
}

// diagnostic: the correlation/peak tail of dd_noaa_sync_windows alone (sync_tail_stage).  hay: device f64 [nwin][n], the signal that is
// searched; env: device f64 [nwin][n], the signal the post-sync mean is taken of; needle_host [n_needles][needle_len], piecewise constant;
// needle_of_window_host [nwin] or NULL (needle 0).  Per window: peak = first index of the largest normalised correlation minus
// needle_len / 2, height = that correlation, tsync = mean(env[peak + m .. peak + 2 m)) when peak + 2 m < n.  A window whose largest value does
// not exceed the threshold of its two largest and two smallest, or whose correlation holds a NaN (a NaN sample, or a stretch of silence as
// long as the needle: 0 / 0), comes back as (INT64_MIN, NaN, NaN); a found peak too close to the end has tsync = NaN alone.  Synchronises.
extern "C" int dd_debug_sync_tail(const double* hay_dev, const double* env_dev, int64_t n, int nwin, const double* needle_host, int needle_len,
                                  int n_needles, const int* needle_of_window_host, int64_t* peak_host, double* height_host, double* tsync_host,
                                  void* stream) {
    DD_REQUIRE(hay_dev && env_dev && needle_host && peak_host && height_host && tsync_host, "null buffer");
    DD_REQUIRE(nwin >= 1 && needle_len >= 1 && needle_len <= n && n < ((int64_t)1 << 30), "nwin / needle_len / n");
    DD_REQUIRE(n_needles >= 1 && n_needles <= DD_CS_MAXNEEDLES, "n_needles (1 or 2)");
    if (needle_of_window_host)
        for (int w = 0; w < nwin; ++w) DD_REQUIRE(needle_of_window_host[w] >= 0 && needle_of_window_host[w] < n_needles, "needle_of_window");
    DDRuns2 R2;
    if (!dd_runs_build(needle_host, needle_len, n_needles, &R2)) {
        dd_set_error("dd_noaa_sync_windows: the needle has more than %d constant runs", DD_XCORR_MAX_RUNS);
        return DD_ERR_INVALID;
    }
    hipStream_t s = dd_stream(stream);
    std::lock_guard<std::mutex> lk(g_sync_mu);
    DDDevBuf<double> PQ;
    DDDevBuf<char> work, res;
    DDDevBuf<int> group;
    DD_HIP_CHECK(PQ.alloc(2 * (size_t)nwin * (size_t)(n + 1)));
    DD_HIP_CHECK(work.alloc(sync_tail_work_bytes(n, nwin)));
    DD_HIP_CHECK(res.alloc(24 * (size_t)nwin));
    DD_HIP_CHECK(group.alloc((size_t)nwin));
    int64_t* d_peak = (int64_t*)res.get();
    double* d_height = (double*)(res.get() + 8 * (size_t)nwin);
    double* d_tsync = (double*)(res.get() + 16 * (size_t)nwin);
    std::vector<char> down(24 * (size_t)nwin);
    hipError_t e0 = hipSuccess;
    if (needle_of_window_host) e0 = hipMemcpyAsync(group.get(), needle_of_window_host, sizeof(int) * (size_t)nwin, hipMemcpyHostToDevice, s);
    if (e0 == hipSuccess) {
        sync_tail_stage(hay_dev, env_dev, n, nwin, needle_len, R2, needle_of_window_host ? group.get() : nullptr, PQ.get(), work.get(),
                        d_peak, d_height, d_tsync, s);
        e0 = hipGetLastError();
    }
    if (e0 == hipSuccess) e0 = hipMemcpyAsync(down.data(), res.get(), down.size(), hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);                            // (before the buffers are freed: every return is behind it)
    if (e0 != hipSuccess || e2 != hipSuccess) {
        dd_set_error("dd_debug_sync_tail: %s", hipGetErrorString(e0 != hipSuccess ? e0 : e2));
        return DD_ERR_HIP;
    }
    memcpy(peak_host, down.data(), 8 * (size_t)nwin);
    memcpy(height_host, down.data() + 8 * (size_t)nwin, 8 * (size_t)nwin);
    memcpy(tsync_host, down.data() + 16 * (size_t)nwin, 8 * (size_t)nwin);
    return DD_OK;
}

extern "C" int dd_noaa_sync_windows(const void* iq, int iq_kind, const int64_t* starts_host, int n_windows, int64_t win_len,
                                    uint64_t cycles_q64, const double* fir_taps_host, int fir_ntaps,
                                    const double* pre_taps_host, int pre_ntaps, const double* needle_host, int needle_len,
                                    double samp_rate, int64_t* peak_host, double* height_host, double* tsync_host,
                                    void* stream) {
    return dd_noaa_sync_windows_multi(iq, iq_kind, starts_host, nullptr, n_windows, win_len, cycles_q64, fir_taps_host, fir_ntaps,
                                      pre_taps_host, pre_ntaps, needle_host, needle_len, 1, samp_rate, peak_host, height_host, tsync_host, stream);
}

// The windows of several sync words in one call (getAccurateSync searches sync A around the crude A positions and sync B around
// the crude B positions, decode_noaa.py:828-835: two window lists, one chain, two needles of one length): needle_of_window_host[w]
// says which of the n_needles needles window w is correlated with (NULL: needle 0).  One upload, batches that mix the lists, one
// copy back, one synchronisation -- the second call's host work no longer sits between the two lists' kernels.
extern "C" int dd_noaa_sync_windows_multi(const void* iq, int iq_kind, const int64_t* starts_host, const int* needle_of_window_host,
                                          int n_windows, int64_t win_len, uint64_t cycles_q64, const double* fir_taps_host, int fir_ntaps,
                                          const double* pre_taps_host, int pre_ntaps, const double* needle_host, int needle_len, int n_needles,
                                          double samp_rate, int64_t* peak_host, double* height_host, double* tsync_host,
                                          void* stream) {
    DD_REQUIRE(n_windows >= 0, "n_windows");
    if (n_windows == 0) return DD_OK;
    static const char* tenv = getenv("DD_SYNC_TRACE");               // tools: host-side time stamps inside the call, to stderr
    const bool trace = tenv && atoi(tenv);
    auto now_us = []() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tt0 = now_us();
    DD_REQUIRE(iq && starts_host && peak_host && height_host && tsync_host, "null buffer");
    DD_REQUIRE(iq_kind == 0 || iq_kind == 1, "iq_kind (0 complex64, 1 uint8 pairs)");
    DD_REQUIRE(fir_taps_host && fir_ntaps >= 1 && pre_ntaps >= 0 && (pre_taps_host || pre_ntaps == 0), "taps");
    DD_REQUIRE(needle_host && needle_len >= 1 && samp_rate > 0, "needle/samp_rate");
    DD_REQUIRE(n_needles >= 1 && n_needles <= DD_CS_MAXNEEDLES, "n_needles (1 or 2)");
    if (needle_of_window_host)
        for (int w = 0; w < n_windows; ++w) DD_REQUIRE(needle_of_window_host[w] >= 0 && needle_of_window_host[w] < n_needles, "needle_of_window");
    const int64_t L = win_len, L2 = win_len - 1;
    DD_REQUIRE(L2 >= 2 && needle_len <= L2 && L < ((int64_t)1 << 30), "window length");
    if (!((double)L2 < 0.45 * samp_rate)) {
        dd_set_error("dd_noaa_sync_windows: windows of %lld samples are not shorter than the 0.45 s peak distance; "
                     "use the per-window entry points", (long long)L);
        return DD_ERR_INVALID;
    }
    if (L <= 3 * fir_ntaps || (pre_ntaps && L2 <= 3 * pre_ntaps)) {
        dd_set_error("The length of the input vector x must be greater than padlen, which is %d.",
                     L <= 3 * fir_ntaps ? 3 * fir_ntaps : 3 * pre_ntaps);
        return DD_ERR_INVALID;
    }
    if (!dd_ff_tiled_ok(fir_ntaps, 8) || (pre_ntaps && !dd_ff_tiled_ok(pre_ntaps, 8))) {
        dd_set_error("dd_noaa_sync_windows: filter too long for the tiled zero-phase kernel");
        return DD_ERR_INVALID;
    }
    DDRuns2 R2;                                                       // piecewise-constant needles -> runs
    if (!dd_runs_build(needle_host, needle_len, n_needles, &R2)) {
        dd_set_error("dd_noaa_sync_windows: the needle has more than %d constant runs", DD_XCORR_MAX_RUNS);
        return DD_ERR_INVALID;
    }

    hipStream_t s = dd_stream(stream);
    const float2* tbl = dd_nco_table();
    if (!tbl) {
        dd_set_error("NCO table initialisation failed (no GPU?)");
        return DD_ERR_NODEVICE;
    }
    // (the DD_SYNC_* switches below are read on every call on purpose: the test suite and tools/ change routes inside one process)
    const char* fr_env = getenv("DD_SYNC_FRONT");                     // tools / tests: "kernel" = the front end as a launch of its own
    const bool front_fused = !(fr_env && !strcmp(fr_env, "kernel"));
    int bmax = 64;
    if (const char* e = getenv("DD_SYNC_BATCH")) bmax = atoi(e) > 0 ? atoi(e) : bmax;
    const int B = n_windows < bmax ? n_windows : bmax;
    const int64_t N1 = L + 6 * (int64_t)fir_ntaps, N2 = L2 + 6 * (int64_t)pre_ntaps;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    // layout (per batch of B windows)
    const size_t o_starts = 0;
    const size_t o_group = o_starts + al(sizeof(int64_t) * n_windows);
    const size_t o_taps1 = o_group + al(sizeof(int) * n_windows);
    const size_t o_taps2 = o_taps1 + al(sizeof(double) * fir_ntaps);
    const size_t o_tab = o_taps2 + al(sizeof(double) * (pre_ntaps ? pre_ntaps : 1));
    const size_t o_res = o_tab + al(sizeof(double2) * 3 * (size_t)(pre_ntaps ? pre_ntaps : 1));
    const size_t o_X = o_res + al(24 * (size_t)n_windows);
    const size_t o_Y1 = o_X + al(sizeof(float2) * B * L);                 // X: c64 [B][L]; later the filtered IQ again
    const size_t o_W = o_Y1 + al(sizeof(float2) * B * N1);                // Y1: c64 [B][N1]
    int64_t M = 1;
    while (M < 2 * L2 + 2) M <<= 1;                                       // cyclic convolution length of the envelope stage
    const int64_t nb = M / 2 + 1;
    const char* hm = getenv("DD_SYNC_HILBERT");
    const bool hilbert_fft = hm && !strcmp(hm, "fft");                    // A/B switches: the library's length-N transforms ("fft"),
    const bool hilbert_own = !hilbert_fft && hc_length_ok(M) && !(hm && !strcmp(hm, "lib"));   // its padded real transforms ("lib"); dd_hconv_kernels.h
    const size_t o_SP = o_W + al(sizeof(double) * (B + (B & 1)) * M);     // (two windows share one complex [M] image in dd_hconv_kernels.h)                 // W/XR: f64 [B][M] (or c128 [B][L2]); later P, Q: f64 [B][L2+1] each
    const size_t o_YR = o_SP + al(sizeof(double2) * B * nb);              // SP: c128 [B][M/2+1]
    const size_t o_ENV = o_YR + al(sizeof(double) * B * M);               // YR: f64 [B][M]
    const size_t o_F1 = o_ENV + al(sizeof(double) * B * L2);              // ENV f64 [B][L2]
    const size_t o_H = o_F1 + al(sizeof(double) * B * N2);                // F1: f64 [B][N2]; later the scan tile sums and per-tile peak records
    const size_t total = o_H + al(sizeof(double) * B * L2);               // H: f64 [B][L2]
    char* base = nullptr;
    std::lock_guard<std::mutex> lk(g_sync_mu);
    int rc = sync_scratch(total + 4096, &base);
    if (rc != DD_OK) return rc;
    DDSyncOnExit sync_guard(s);                       // (an early error return below leaves nothing in flight)
    int64_t* d_starts = (int64_t*)(base + o_starts);
    const int* d_group = needle_of_window_host ? (const int*)(base + o_group) : nullptr;
    double* d_taps1 = (double*)(base + o_taps1);
    double* d_taps2 = (double*)(base + o_taps2);
    int64_t* d_peak = (int64_t*)(base + o_res);
    double* d_height = (double*)(base + o_res + 8 * (size_t)n_windows);
    double* d_tsync = (double*)(base + o_res + 16 * (size_t)n_windows);
    float2* X = (float2*)(base + o_X);
    float2* Y1 = (float2*)(base + o_Y1);
    double2* W = (double2*)(base + o_W);
    double2* SP = (double2*)(base + o_SP);
    double* YR = (double*)(base + o_YR);
    const double2* HH = nullptr;
    if (!hilbert_fft) {
        rc = hilbert_spectrum(L2, M, false, &HH, s);
        if (rc != DD_OK) return rc;
    }
    double* ENV = (double*)(base + o_ENV);
    double* F1 = (double*)(base + o_F1);
    double* H = (double*)(base + o_H);
    // window starts, both tap sets and the cosine table go up as ONE copy (they are neighbours in the layout)
    std::vector<char> up(o_res, 0);
    memcpy(up.data() + o_starts, starts_host, sizeof(int64_t) * n_windows);
    if (needle_of_window_host) memcpy(up.data() + o_group, needle_of_window_host, sizeof(int) * n_windows);
    memcpy(up.data() + o_taps1, fir_taps_host, sizeof(double) * fir_ntaps);
    if (pre_ntaps) memcpy(up.data() + o_taps2, pre_taps_host, sizeof(double) * pre_ntaps);
    // the envelope's pre-filter is hamming(492) (decode_noaa.py:677): a two-term cosine series -- prefix-sum form
    // (dd_filtfilt_kernels.h)
    DDCosFit fit2;
    const bool cos2 = pre_ntaps && dd_cos_fit_cached(pre_taps_host, pre_ntaps, &fit2) && dd_fc_ok(pre_ntaps, fit2.Q);
    double2* d_tab = (double2*)(base + o_tab);
    if (cos2) {
        // (the table of one tap set is kept on the host between calls; the copy's pageable source is staged before the call returns)
        static std::mutex tab_mu;
        static std::vector<double2> tabh;
        static int tab_K = 0, tab_Q = 0;
        std::lock_guard<std::mutex> tl(tab_mu);
        if (tab_K != pre_ntaps || tab_Q != fit2.Q) { dd_cos_table(pre_ntaps, fit2.Q, tabh); tab_K = pre_ntaps; tab_Q = fit2.Q; }
        memcpy(up.data() + o_tab, tabh.data(), sizeof(double2) * tabh.size());
    }
    const double tt_up0 = now_us() - tt0;
    DD_HIP_CHECK(hipMemcpyAsync(base, up.data(), o_res, hipMemcpyHostToDevice, s));          // (pageable source: staged before the call returns)
    const double tt_up1 = now_us() - tt0;
    for (int w0 = 0; w0 < n_windows; w0 += B) {
        const int b = n_windows - w0 < B ? n_windows - w0 : B;
        const dim3 gL4(grid1((L + 3) / 4), b);
        if (front_fused) {
            // X <- filtfilt(oscillator x raw IQ): pass 1 computes the samples where it stages them
            const DDFrontSrc F = {iq, d_starts + w0, cycles_q64, tbl, iq_kind};
            dd_filtfilt_front_launch(F, Y1, X, L, L, fir_ntaps, d_taps1, b, s);
        } else {
            if (iq_kind == 1) hipLaunchKernelGGL(k_sync_front<true>, gL4, dim3(256), 0, s, iq, d_starts + w0, L, cycles_q64, tbl, X);
            else hipLaunchKernelGGL(k_sync_front<false>, gL4, dim3(256), 0, s, iq, d_starts + w0, L, cycles_q64, tbl, X);
            dd_filtfilt_launch<float2>(X, L, Y1, X, L, L, fir_ntaps, d_taps1, b, s);        // X <- filtfilt(X): pass 2 reads only Y1
        }
        rc = sync_envelope_stage(hilbert_fft ? 2 : (hilbert_own ? 0 : 1), X, L, b, M, HH, W, SP, YR, ENV, s);
        if (rc != DD_OK) return rc;
        const double* hay = ENV;
        if (pre_ntaps) {
            rc = sync_prefilter_stage(ENV, L2, b, pre_ntaps, cos2 ? &fit2 : nullptr, d_tab, d_taps2, F1, H, s);
            if (rc != DD_OK) return rc;
            hay = H;
        }
        // prefix sums into the (now free) FFT buffer; tile sums and per-tile peak records into the pre-filter's (now free) work buffer
        sync_tail_stage(hay, ENV, L2, b, needle_len, R2, d_group ? d_group + w0 : nullptr, (double*)W, F1, d_peak + w0, d_height + w0, d_tsync + w0, s);
        DD_LAUNCH_CHECK();
    }
    char* down = nullptr;                                                                        // the three result arrays, one copy (pinned)
    rc = sync_pinned(24 * (size_t)n_windows, &down);
    if (rc != DD_OK) return rc;
    const double tt_enq = now_us() - tt0;
    DD_HIP_CHECK(hipMemcpyAsync(down, base + o_res, 24 * (size_t)n_windows, hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    sync_guard.done();
    { const int sr = dd_seam_poll_all(); if (sr != DD_OK) return sr; }
    if (trace) fprintf(stderr, "sync windows host us (%d windows): upload starts %.0f, upload enqueued %.0f, batches enqueued %.0f, synchronised %.0f\n",
                       n_windows, tt_up0, tt_up1, tt_enq, now_us() - tt0);
    memcpy(peak_host, down, 8 * (size_t)n_windows);
    memcpy(height_host, down + 8 * (size_t)n_windows, 8 * (size_t)n_windows);
    memcpy(tsync_host, down + 16 * (size_t)n_windows, 8 * (size_t)n_windows);
    return DD_OK;
}
