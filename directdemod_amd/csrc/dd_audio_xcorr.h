// X1 / X2: decode_noaa.__correlate and __correlateAndFindPeaks (decode_noaa.py:659-767): dd_xcorr_norm_f64, dd_find_peaks_f64, and what
// the accurate windows (dd_audio_sync.h) and the crude tail (dd_audio_crude.h) share with them: the prefix-sum scan, the needle's run
// table and the run-length correlation, the peak pick's selection and candidate kernels and its grouping on the host.
// One of the six parts of dd_audio.hip (one translation unit: the parts share the plan cache, the float64 transform and the scratch
// buffers of dd_audio.hip and are included there, each using only the parts before it).  Internal; not a stand-alone header.
// ---------------------------------------------------------------- X1: normalised correlation
// cor = correlate(h, needle, 'same'); sums = convolve(h*h, ones(m), 'same');
// out = cor / sqrt(sums * sum(needle^2))  (decode_noaa.py:671-673).  Both windows are
// h[k-(m-1) .. k], k = i + (m-1)/2, so one pass computes both (float64, direct form).
__global__ void __launch_bounds__(256) k_xcorr_norm(const double* __restrict__ h, int64_t n, const double* __restrict__ v, int m,
                                                    double vv, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t k = i + (m - 1) / 2;
    const int64_t a0 = k - (m - 1);
    double c = 0.0, e = 0.0;
    int t0 = a0 < 0 ? (int)(-a0) : 0;
    int t1 = (a0 + m > n) ? (int)(n - a0) : m;
    for (int t = t0; t < t1; ++t) {
        const double x = h[a0 + t];
        c = fma(v[t], x, c);
        e = fma(x, x, e);
    }
    out[i] = c / sqrt(e * vv);
}

// Run-length form.  The sync needles are np.repeat(bits, rep) * 233 + 11) / 255 (decode_noaa.py:690-694):
// 40 bits held for rep samples each, i.e. a dozen constant runs over 560 (crude) or 19 680 (accurate)
// samples.  Over a run the correlation is value * (window sum of h), so with prefix sums P of h and Q of
// h^2 an output costs two lookups per run and two for the energy instead of m multiply-adds: the accurate
// window went from 2.1 ms (2.3e9 MAC) to tens of microseconds.  float64 prefix sums over <= 1e6 values
// of O(1): the window differences carry ~1e-13 relative error -- the size of the difference between the
// direct sum and SciPy's FFT method, and well inside the 1e-9 of the stage.
#define DD_XCORR_MAX_RUNS 64
struct DDRuns {
    int nr;
    int start[DD_XCORR_MAX_RUNS + 1];
    double val[DD_XCORR_MAX_RUNS];
};
#define DD_CS_MAXNEEDLES 2               // needles (sync words) one call correlates
struct DDRuns2 { DDRuns r[DD_CS_MAXNEEDLES]; double vv[DD_CS_MAXNEEDLES]; };
// The run tables and sum(needle^2) of 1 or 2 needles of m samples each (needles_host[needle][m]); the unused slots repeat needle 0.
// false: a needle has more than DD_XCORR_MAX_RUNS runs (every caller has its own answer to that)
static bool dd_runs_build(const double* needles_host, int m, int n_needles, DDRuns2* R2) {
    for (int d = 0; d < n_needles; ++d) {
        const double* nh = needles_host + (size_t)d * m;
        DDRuns& R = R2->r[d];
        R.nr = 0;
        double vv = 0.0;
        for (int t = 0; t < m; ++t) {
            if (t == 0 || nh[t] != nh[t - 1]) {
                if (R.nr == DD_XCORR_MAX_RUNS) return false;
                R.start[R.nr] = t;
                R.val[R.nr] = nh[t];
                ++R.nr;
            }
            vv += nh[t] * nh[t];
        }
        R.start[R.nr] = m;
        R2->vv[d] = vv;
    }
    for (int d = n_needles; d < DD_CS_MAXNEEDLES; ++d) { R2->r[d] = R2->r[0]; R2->vv[d] = R2->vv[0]; }
    return true;
}

// ---- prefix sums of h and h^2 (a batch of windows in the accurate-sync chain, one signal elsewhere)
#define DD_SCAN_TILE 2048
// P[b][i] = sum h[b][0..i), Q likewise of h^2, in two launches over tiles of 2048 samples: tile sums, then each
// tile adds the sums of the tiles before it (ascending) to its own scan -- every tile of every window in parallel
// (a lane scans 8 consecutive samples, but the tile is fetched -- and the prefix sums are written -- with lanes on consecutive
// addresses, through an LDS image skewed by one element per 8: read lane by lane, 64-byte runs at a 64-byte stride, these
// kernels moved 2 TB/s)
#define DD_SCAN_LDS (DD_SCAN_TILE + DD_SCAN_TILE / 8)
__device__ __forceinline__ void dd_scan_tile_load(const double* __restrict__ h, int64_t n, int64_t tile0, int t, double* __restrict__ lds,
                                                  double (&p)[8], double (&q)[8]) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int e = t + 256 * r;
        lds[e + (e >> 3)] = (tile0 + e < n) ? h[tile0 + e] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double v = lds[9 * t + j];
        p[j] = j ? p[j - 1] + v : v;
        q[j] = j ? q[j - 1] + v * v : v * v;
    }
}
// out[tile0 + 1 + e] = v[e] for the tile's 2048 values held 8 per lane (lane t: e = 8 t .. 8 t + 7), stored coalesced
__device__ __forceinline__ void dd_scan_tile_store(double* __restrict__ out, int64_t n, int64_t tile0, int t, double* __restrict__ lds, const double (&v)[8]) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) lds[9 * t + j] = v[j];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int e = t + 256 * r;
        if (tile0 + e < n) out[tile0 + e + 1] = lds[e + (e >> 3)];
    }
}
__global__ void __launch_bounds__(256) k_scan_part(const double* __restrict__ h, int64_t n, int tiles, double2* __restrict__ part) {
    __shared__ double sp[4], sq[4];
    __shared__ double lds[DD_SCAN_LDS];
    h += (int64_t)blockIdx.y * n;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    double p[8], q[8];
    dd_scan_tile_load(h, n, (int64_t)blockIdx.x * DD_SCAN_TILE, t, lds, p, q);
    double tp = p[7], tq = q[7];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { tp += __shfl_down(tp, d); tq += __shfl_down(tq, d); }
    if (lane == 0) { sp[wv] = tp; sq[wv] = tq; }
    __syncthreads();
    if (t == 0) part[(int64_t)blockIdx.y * tiles + blockIdx.x] = make_double2(((sp[0] + sp[1]) + sp[2]) + sp[3], ((sq[0] + sq[1]) + sq[2]) + sq[3]);
}
__global__ void __launch_bounds__(256) k_scan_final(const double* __restrict__ h, int64_t n, int tiles, const double2* __restrict__ part,
                                                    double* __restrict__ P, double* __restrict__ Q) {
    __shared__ double sp[4], sq[4];
    h += (int64_t)blockIdx.y * n;
    P += (int64_t)blockIdx.y * (n + 1);
    Q += (int64_t)blockIdx.y * (n + 1);
    part += (int64_t)blockIdx.y * tiles;
    __shared__ double lds[DD_SCAN_LDS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t tile0 = (int64_t)blockIdx.x * DD_SCAN_TILE;
    double p[8], q[8];
    dd_scan_tile_load(h, n, tile0, t, lds, p, q);
    // sums of the tiles before this one: every lane takes the tiles t, t + 256, ..., the workgroup adds them up (one lane
    // walking all of them was 77 us of the accurate windows' 1.1 ms per batch)
    __shared__ double bp[4], bq[4];
    double cp = 0.0, cq = 0.0;
    for (int k = t; k < (int)blockIdx.x; k += 256) { const double2 v = part[k]; cp += v.x; cq += v.y; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { cp += __shfl_down(cp, d); cq += __shfl_down(cq, d); }
    if (lane == 0) { bp[wv] = cp; bq[wv] = cq; }
    double tp = p[7], tq = q[7];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double a = __shfl_up(tp, d), c = __shfl_up(tq, d);
        if (lane >= d) { tp += a; tq += c; }
    }
    if (lane == 63) { sp[wv] = tp; sq[wv] = tq; }
    double ep = __shfl_up(tp, 1), eq = __shfl_up(tq, 1);
    if (lane == 0) { ep = 0.0; eq = 0.0; }
    __syncthreads();
    cp = ((bp[0] + bp[1]) + bp[2]) + bp[3];
    cq = ((bq[0] + bq[1]) + bq[2]) + bq[3];
    for (int w = 0; w < wv; ++w) { cp += sp[w]; cq += sq[w]; }
    ep += cp;
    eq += cq;
    if (blockIdx.x == 0 && t == 0) { P[0] = 0.0; Q[0] = 0.0; }
#pragma unroll
    for (int j = 0; j < 8; ++j) { p[j] += ep; q[j] += eq; }
    dd_scan_tile_store(P, n, tile0, t, lds, p);
    dd_scan_tile_store(Q, n, tile0, t, lds, q);
}
// The crude tail's three-launch form: exclusive scan of the tile sums (one workgroup), so that the final pass adds one number per tile
// instead of walking all the tiles before it (1765 of them for a minute of audio)
__global__ void __launch_bounds__(256) k_scan_mid(double2* __restrict__ part, int tiles) {
    __shared__ double sp[4], sq[4];
    __shared__ double cp, cq;
    if (threadIdx.x == 0) { cp = 0.0; cq = 0.0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int b = 0; b < tiles; b += 256) {
        const int i = b + threadIdx.x;
        const double2 v = i < tiles ? part[i] : make_double2(0.0, 0.0);
        double ip = v.x, iq = v.y;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double a = __shfl_up(ip, d), c = __shfl_up(iq, d);
            if (lane >= d) { ip += a; iq += c; }
        }
        if (lane == 63) { sp[wv] = ip; sq[wv] = iq; }
        __syncthreads();
        double op = cp, oq = cq;
        for (int w = 0; w < wv; ++w) { op += sp[w]; oq += sq[w]; }
        if (i < tiles) part[i] = make_double2(op + ip - v.x, oq + iq - v.y);
        __syncthreads();
        if (threadIdx.x == 255) { cp = op + ip; cq = oq + iq; }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) k_scan_final_x(const double* __restrict__ h, int64_t n, const double2* __restrict__ partx,
                                                      double* __restrict__ P, double* __restrict__ Q) {
    __shared__ double sp[4], sq[4];
    __shared__ double lds[DD_SCAN_LDS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t tile0 = (int64_t)blockIdx.x * DD_SCAN_TILE;
    double p[8], q[8];
    dd_scan_tile_load(h, n, tile0, t, lds, p, q);
    const double2 base = partx[blockIdx.x];
    double cp = base.x, cq = base.y;
    double tp = p[7], tq = q[7];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double a = __shfl_up(tp, d), c = __shfl_up(tq, d);
        if (lane >= d) { tp += a; tq += c; }
    }
    if (lane == 63) { sp[wv] = tp; sq[wv] = tq; }
    double ep = __shfl_up(tp, 1), eq = __shfl_up(tq, 1);
    if (lane == 0) { ep = 0.0; eq = 0.0; }
    __syncthreads();
    for (int w = 0; w < wv; ++w) { cp += sp[w]; cq += sq[w]; }
    ep += cp;
    eq += cq;
    if (blockIdx.x == 0 && t == 0) { P[0] = 0.0; Q[0] = 0.0; }
#pragma unroll
    for (int j = 0; j < 8; ++j) { p[j] += ep; q[j] += eq; }
    dd_scan_tile_store(P, n, tile0, t, lds, p);
    dd_scan_tile_store(Q, n, tile0, t, lds, q);
}

// ---- the run-length correlation, stored: up to two needles of equal length at once (blockIdx.y = needle; out[needle][n]).  Per output:
// c = sum over the runs of value * (P[end of run] - P[start of run]) by fma in run order, e = Q[a0 + m] - Q[a0], both with the
// window h[a0 .. a0 + m - 1], a0 = i + (m - 1) / 2 - (m - 1), clamped to [0, n]; an all-zero window gives 0 / 0 like the direct form.
// The 256 outputs of a workgroup read P at a0 + start[r], r = 0 .. nr: 256 + m + 1 consecutive prefix sums, each wanted by
// ~nr outputs.  They are staged in LDS once (when they fit: 817 doubles for the crude needles) -- straight from L2 the kernel
// ran at the L2's bandwidth, 108 us for 2 x 3.6 M outputs.
// A lane owns outputs t, t + 256, t + 512, t + 768 of a 1024-output tile: four independent chains per run boundary (one
// output per lane was a chain of ~15 dependent LDS reads per wave: 93 us for 2 x 3.6 M outputs, latency bound).
#define DD_XC_LDS_MAX 4096
#define DD_XCN_TILE 1024
// (round 4: the run table comes out of LDS instead of one scalar load from the kernel arguments per run and the loop is
// unrolled by four -- the loop used to wait for that load, then for its four reads, run after run; the energy look-ups of
// the four outputs are issued together.  Same operations in the same order per output.)
template <bool STAGED>
__global__ void __launch_bounds__(256) k_xcorr_runs_n(const double* __restrict__ P, const double* __restrict__ Q, int64_t n, int m,
                                                      const DDRuns2 R2, double* __restrict__ out) {
    __shared__ double sP[STAGED ? DD_XC_LDS_MAX : 1];
    __shared__ double sval[DD_XCORR_MAX_RUNS];
    __shared__ int sst[DD_XCORR_MAX_RUNS + 4];
    const DDRuns& R = R2.r[blockIdx.y];
    const int nr = R.nr;
    const int64_t i0 = (int64_t)blockIdx.x * DD_XCN_TILE;
    const int64_t base = i0 + (m - 1) / 2 - (m - 1);             // window of output i: P[base + (i - i0) + start[r]]
    auto at = [&](const double* S, int64_t x) { return S[x < 0 ? 0 : (x > n ? n : x)]; };
    if (threadIdx.x < DD_XCORR_MAX_RUNS) {
        const int r = threadIdx.x;
        sst[r] = r < nr ? R.start[r + 1] : 0;                     // sst[r] = end of run r
        sval[r] = r < nr ? R.val[r] : 0.0;
    }
    if (STAGED)
        for (int k = threadIdx.x; k < DD_XCN_TILE + m + 1; k += 256) sP[k] = at(P, base + k);
    // energy window ends of this lane's four outputs (independent of the loop below: in flight across it)
    double qa[4], qb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t a0 = base + threadIdx.x + 256 * u;
        qa[u] = at(Q, a0);
        qb[u] = at(Q, a0 + m);
    }
    __syncthreads();
    auto look = [&](int u, int st) -> double {
        return STAGED ? sP[threadIdx.x + 256 * u + st] : at(P, base + threadIdx.x + 256 * u + st);
    };
    double c[4] = {0.0, 0.0, 0.0, 0.0}, lo[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) lo[u] = look(u, 0);
    int r = 0;
    for (; r + 4 <= nr; r += 4) {
        int st[4];
        double v[4], hi[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { st[k] = sst[r + k]; v[k] = sval[r + k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int u = 0; u < 4; ++u) hi[k][u] = look(u, st[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int u = 0; u < 4; ++u) { c[u] = fma(v[k], hi[k][u] - lo[u], c[u]); lo[u] = hi[k][u]; }
    }
    for (; r < nr; ++r) {
        const int st = sst[r];
        const double v = sval[r];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const double hi = look(u, st); c[u] = fma(v, hi - lo[u], c[u]); lo[u] = hi; }
    }
    const double qn = 1e-13 * Q[n], vv = R2.vv[blockIdx.y];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + threadIdx.x + 256 * u;
        double e = qb[u] - qa[u];
        double cc = c[u];
        if (!(e > qn)) { cc = 0.0; e = 0.0; }
        if (i < n) out[(int64_t)blockIdx.y * n + i] = cc / sqrt(e * vv);
    }
}

// cor[needle][n] from the prefix sums; the look-ups are staged in LDS when a tile's share of P fits
static void xcorr_runs_launch(const double* P, const double* Q, int64_t n, int m, const DDRuns2& R2, int n_needles, double* cor, hipStream_t s) {
    const dim3 grid((unsigned)((n + DD_XCN_TILE - 1) / DD_XCN_TILE), n_needles);
    if (DD_XCN_TILE + m + 1 <= DD_XC_LDS_MAX)
        hipLaunchKernelGGL(k_xcorr_runs_n<true>, grid, dim3(256), 0, s, P, Q, n, m, R2, cor);
    else
        hipLaunchKernelGGL(k_xcorr_runs_n<false>, grid, dim3(256), 0, s, P, Q, n, m, R2, cor);
}

static int xcorr_runs(const double* h, int64_t n, int m, const DDRuns2& R2, double* out, hipStream_t s) {
    // P[i] = sum h[0..i), Q[i] = sum h^2[0..i): the two-launch tile scan of the batched chain, batch of one
    const int tiles = (int)((n + DD_SCAN_TILE - 1) / DD_SCAN_TILE);
    std::lock_guard<std::mutex> lk(g_sync_mu);
    char* base = nullptr;
    const size_t pq_bytes = (sizeof(double) * (2 * (n + 1)) + 255) & ~(size_t)255;
    int rc = sync_scratch(pq_bytes + sizeof(double2) * (size_t)tiles, &base);
    if (rc != DD_OK) return rc;
    double* P = (double*)base;
    double* Q = P + (n + 1);
    double2* part = (double2*)(base + pq_bytes);
    hipLaunchKernelGGL(k_scan_part, dim3(tiles, 1), dim3(256), 0, s, h, n, tiles, part);
    hipLaunchKernelGGL(k_scan_final, dim3(tiles, 1), dim3(256), 0, s, h, n, tiles, part, P, Q);
    xcorr_runs_launch(P, Q, n, m, R2, 1, out, s);
    hipError_t le = hipGetLastError();
    hipError_t se = hipStreamSynchronize(s);
    DD_HIP_CHECK(le); DD_HIP_CHECK(se);
    return DD_OK;
}

extern "C" int dd_xcorr_norm_f64(const double* h, int64_t n, const double* needle_host, int m, double* out, void* stream) {
    DD_REQUIRE(n >= 1 && m >= 1 && m <= n, "n/m");
    DD_REQUIRE(h && needle_host && out, "null buffer");
    hipStream_t s = dd_stream(stream);
    // piecewise-constant needle with few runs -> prefix-sum form
    DDRuns2 R2;
    if (n < (int64_t)1 << 31 && dd_runs_build(needle_host, m, 1, &R2) && m >= 16 * R2.r[0].nr) return xcorr_runs(h, n, m, R2, out, s);
    DDScratchLock scr;                      // held until this entry point has enqueued everything
    int rcs = scr.get(sizeof(double) * (size_t)m, s);
    char* base = scr.ptr;
    if (rcs != DD_OK) return rcs;
    double* v = reinterpret_cast<double*>(base);
    DD_HIP_CHECK(hipMemcpyAsync(v, needle_host, sizeof(double) * m, hipMemcpyHostToDevice, s));
    double vv = 0.0;
    for (int t = 0; t < m; ++t) vv += needle_host[t] * needle_host[t];
    hipLaunchKernelGGL(k_xcorr_norm, dim3(grid1(n)), dim3(256), 0, s, h, n, v, m, vv, out);
    hipError_t le = hipGetLastError();
    hipError_t e = hipStreamSynchronize(s);                 // the needle is the caller's host memory
    DD_HIP_CHECK(le);
    DD_HIP_CHECK(e);
    return DD_OK;
}

// ---------------------------------------------------------------- X2: peak pick (decode_noaa.py:713-751)
// The reference takes the means of the K largest and K smallest correlation values with np.argpartition (:717-723; K is
// two per second of signal) and then every index whose value exceeds a threshold between them (:726).  No sort of the
// whole array is needed for that: a radix SELECT finds the K-th largest and K-th smallest value exactly -- eight
// passes over the data, one byte of the order-preserving 64-bit key per pass, histograms in LDS (interleaved copies,
// so that the many samples of one bin do not serialise on one address); every workgroup re-derives the bins picked so far
// from the earlier passes' global histograms, so no pick kernel sits between the passes -- and the values beyond them
// (fewer than K each) are appended to a small buffer, to be sorted and summed in ascending order.  Candidates: per-wave
// counts, then a second pass that writes the indices in ascending order.  One set of kernels for dd_find_peaks_f64 (one needle,
// threshold on the host, any K) and dd_noaa_crude_tail (both needles per launch, threshold on the device: dd_audio_crude.h).
// They count in 32 bits: n < 2^31.
__device__ __forceinline__ unsigned long long dd_key_f64(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);          // ascending in x, total order (-0 < +0, NaNs at the ends)
}
#define DD_CS_WG 512                  // workgroups per needle and selection launch
#define DD_CS_COPIES 8                // interleaved LDS histograms per selection
struct DDCrudeSel {
    unsigned int hist[8][2][256];     // per pass: [K-th largest | K-th smallest]
    unsigned int n_beyond[2];         // values appended above / below
    unsigned int n_cand;              // candidates appended
    unsigned int pad;
    unsigned int beyond_cnt[2];       // bookkeeping: how many values lie strictly beyond the final keys
    unsigned long long key[2];
    double thr, sum_hi, sum_lo;
};

// one wave: the bin that holds rank `r` counted from the top (TOP) or the bottom of a 256-bin histogram, and how many values
// lie in the bins beyond it.  Lane l owns bins 4 l .. 4 l + 3.
template <bool TOP>
__device__ __forceinline__ void dd_pick_bin(const unsigned int* gh, unsigned int r, int lane, int* bin, unsigned int* beyond) {
    unsigned int c[4], tot = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = gh[4 * lane + j]; tot += c[j]; }
    unsigned int incl = tot;                          // TOP: sum over lanes >= l; else lanes <= l
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int u = TOP ? __shfl_down(incl, d) : __shfl_up(incl, d);
        if (TOP ? (lane + d < 64) : (lane >= d)) incl += u;
    }
    unsigned int before = incl - tot;                 // values in the lanes beyond this one
    int found = -1;
    unsigned int fb = 0;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int j = TOP ? 3 - jj : jj;
        if (found < 0 && before + c[j] >= r) { found = 4 * lane + j; fb = before; }
        before += c[j];
    }
    // the first lane from the far end that finds it is the one; broadcast
    const unsigned long long m = __ballot(found >= 0);
    const int src = m ? (TOP ? (63 - __builtin_clzll(m)) : __builtin_ctzll(m)) : 0;
    *bin = __shfl(found, src);
    *beyond = __shfl(fb, src);
    if (!m) { *bin = TOP ? 0 : 255; *beyond = 0; }
}
// The selections' state after passes 0 .. upto-1, recomputed from the global histograms of those passes (complete: they were
// filled by earlier launches) by waves 0 (K-th largest) and 1 (K-th smallest) of every workgroup, and handed to all lanes.
struct DDCsState { unsigned long long prefix[2]; unsigned int remaining[2], beyond[2]; };
__device__ __forceinline__ DDCsState dd_cs_state(const DDCrudeSel* S, int upto, int K, DDCsState* lds_tmp) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (wv < 2) {
        unsigned long long prefix = 0ull;
        unsigned int remaining = (unsigned int)K, beyond = 0u;
        for (int p = 0; p < upto; ++p) {
            int bin;
            unsigned int by;
            if (wv == 0) dd_pick_bin<true>(S->hist[p][0], remaining, lane, &bin, &by);
            else dd_pick_bin<false>(S->hist[p][1], remaining, lane, &bin, &by);
            prefix = (prefix << 8) | (unsigned long long)bin;
            remaining -= by;
            beyond += by;
        }
        if (lane == 0) { lds_tmp->prefix[wv] = prefix; lds_tmp->remaining[wv] = remaining; lds_tmp->beyond[wv] = beyond; }
    }
    __syncthreads();
    const DDCsState st = *lds_tmp;
    __syncthreads();
    return st;
}

// pass `pass` of the radix select (one byte of the key): histogram of the values whose higher bytes equal the prefix so far.
// grid (G, needles); the launch boundary is the barrier between passes.
__global__ void __launch_bounds__(256) k_cs_hist(const double* __restrict__ cor_all, int64_t n, int K, int pass, DDCrudeSel* __restrict__ sel_all) {
    __shared__ unsigned int h[2][DD_CS_COPIES][256];
    __shared__ DDCsState tmp;
    const int nd = blockIdx.y, g = blockIdx.x, G = gridDim.x, t = threadIdx.x;
    const double* cor = cor_all + (int64_t)nd * n;
    DDCrudeSel* S = sel_all + nd;
    for (int i = t; i < 2 * DD_CS_COPIES * 256; i += 256) (&h[0][0][0])[i] = 0;
    const DDCsState st = dd_cs_state(S, pass, K, &tmp);          // (its barriers also cover the clearing above)
    const int64_t i_lo = n * g / G, i_hi = n * (g + 1) / G;
    const int shift = 56 - 8 * pass;
    const int copy = t & (DD_CS_COPIES - 1);
    for (int64_t i = i_lo + t; i < i_hi; i += 1024) {             // four loads in flight per lane
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (i + 256 * u < i_hi) ? cor[i + 256 * u] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i + 256 * u >= i_hi) break;
            const unsigned long long k = dd_key_f64(v[u]);
            const unsigned long long hi = pass ? (k >> (shift + 8)) : 0;
            const unsigned int d = (unsigned int)(k >> shift) & 255u;
            if (hi == st.prefix[0]) atomicAdd(&h[0][copy][d], 1u);
            if (hi == st.prefix[1]) atomicAdd(&h[1][copy][d], 1u);
        }
    }
    __syncthreads();
    for (int i = t; i < 512; i += 256) {
        unsigned int c = 0;
#pragma unroll
        for (int k = 0; k < DD_CS_COPIES; ++k) c += h[i >> 8][k][i & 255];
        if (c) atomicAdd(&S->hist[pass][i >> 8][i & 255], c);
    }
}
// the values strictly beyond the two final keys (fewer than K each), any order: beyond_all[needle][above | below][stride], of which
// the first `cap` of each are written
__global__ void __launch_bounds__(256) k_cs_collect(const double* __restrict__ cor_all, int64_t n, int K, DDCrudeSel* __restrict__ sel_all, double* __restrict__ beyond_all,
                                                    unsigned int cap, unsigned int stride) {
    __shared__ DDCsState tmp;
    const int nd = blockIdx.y, g = blockIdx.x, G = gridDim.x, t = threadIdx.x;
    const double* cor = cor_all + (int64_t)nd * n;
    DDCrudeSel* S = sel_all + nd;
    double* above = beyond_all + (size_t)nd * 2 * stride;
    double* below = above + stride;
    const DDCsState st = dd_cs_state(S, 8, K, &tmp);
    const int64_t i_lo = n * g / G, i_hi = n * (g + 1) / G;
    for (int64_t i = i_lo + t; i < i_hi; i += 256) {
        const double v = cor[i];
        const unsigned long long k = dd_key_f64(v);
        if (k > st.prefix[0]) { const unsigned int o = atomicAdd(&S->n_beyond[0], 1u); if (o < cap) above[o] = v; }
        if (k < st.prefix[1]) { const unsigned int o = atomicAdd(&S->n_beyond[1], 1u); if (o < cap) below[o] = v; }
    }
}
// one workgroup per needle: the two final keys and the counts beyond them, for a host that computes the threshold itself
__global__ void __launch_bounds__(128) k_cs_keys(int K, DDCrudeSel* __restrict__ sel_all) {
    __shared__ DDCsState tmp;
    DDCrudeSel* S = sel_all + blockIdx.x;
    const DDCsState st = dd_cs_state(S, 8, K, &tmp);
    if (threadIdx.x == 0) {
        S->key[0] = st.prefix[0]; S->key[1] = st.prefix[1];
        S->beyond_cnt[0] = st.beyond[0]; S->beyond_cnt[1] = st.beyond[1];
    }
}
// candidates cor > threshold (:726) with their heights, IN INDEX ORDER (the grouping of :729-746 walks them in that order; appended
// by atomics they came out shuffled and the host sorted 5 000 + 17 000 of them for the 60 s recording: 0.45 ms of a 1.0 ms call).
// Two launches: every wave counts the candidates of its contiguous stretch, then -- its offset = the counts of the waves before
// it -- writes them where they belong (ballot + prefix count, no barrier).  The first DD_CS_HEAD of a needle go into the block
// the host fetches in its one copy (behind the counters), later ones into the overflow arrays
#define DD_CS_HEAD 24576
#define DD_CS_WAVES (DD_CS_WG * 4)
struct DDCand { int64_t idx; double val; };
__device__ __forceinline__ void dd_cs_stretch(int64_t n, int wave, int64_t* lo, int64_t* hi) {
    *lo = n * wave / DD_CS_WAVES;
    *hi = n * (wave + 1) / DD_CS_WAVES;
}
__global__ void __launch_bounds__(256) k_cs_cand_count(const double* __restrict__ cor_all, int64_t n, DDCrudeSel* __restrict__ sel_all,
                                                       unsigned int* __restrict__ cnt_all) {
    const int nd = blockIdx.y, lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const double* cor = cor_all + (int64_t)nd * n;
    DDCrudeSel* S = sel_all + nd;
    const double thr = S->thr;
    int64_t lo, hi;
    dd_cs_stretch(n, wave, &lo, &hi);
    unsigned int c = 0;
    for (int64_t i = lo + lane; i < hi; i += 64) c += cor[i] > thr ? 1u : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d);
    if (lane == 0) {
        cnt_all[(size_t)nd * DD_CS_WAVES + wave] = c;
        if (c) atomicAdd(&S->n_cand, c);
    }
}
__global__ void __launch_bounds__(256) k_cs_cand_write(const double* __restrict__ cor_all, int64_t n, const DDCrudeSel* __restrict__ sel_all,
                                                       const unsigned int* __restrict__ cnt_all, DDCand* __restrict__ head_all,
                                                       int64_t* __restrict__ cidx_all, double* __restrict__ cval_all, unsigned int cap) {
    const int nd = blockIdx.y, lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const double* cor = cor_all + (int64_t)nd * n;
    const unsigned int* cnt = cnt_all + (size_t)nd * DD_CS_WAVES;
    DDCand* head = head_all + (size_t)nd * DD_CS_HEAD;
    int64_t* cidx = cidx_all + (size_t)nd * cap;
    double* cval = cval_all + (size_t)nd * cap;
    const double thr = sel_all[nd].thr;
    if (cnt[wave] == 0) return;                                    // (wave uniform)
    unsigned int off = 0;
    for (int w = lane; w < wave; w += 64) off += cnt[w];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) off += __shfl_xor(off, d);
    int64_t lo, hi;
    dd_cs_stretch(n, wave, &lo, &hi);
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        const double v = i < hi ? cor[i] : 0.0;
        const bool take = i < hi && v > thr;
        const unsigned long long mask = __ballot(take);
        if (take) {
            const unsigned int o = off + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
            if (o < DD_CS_HEAD) head[o] = DDCand{i, v};
            else if (o < cap) { cidx[o] = i; cval[o] = v; }
        }
        off += (unsigned int)__popcll(mask);
    }
}

// One needle's `count` candidates (in index order: k_cs_cand_write) -> its peaks.  head: the first min(count, DD_CS_HEAD) candidates,
// on the host; the rest is fetched from the overflow arrays d_cidx / d_cval (device, indexed by candidate number).
static int peaks_from_candidates(const char* who, unsigned int count, const DDCand* head, const int64_t* d_cidx, const double* d_cval,
                                 double samp_rate, int needle_len, int64_t* peaks_host, int max_peaks, int* n_peaks, hipStream_t s) {
    const unsigned int first_n = count < DD_CS_HEAD ? count : DD_CS_HEAD, more = count - first_n;
    std::vector<int64_t> ci(more);
    std::vector<double> cv(more);
    if (more) {
        DD_HIP_CHECK(hipMemcpyAsync(ci.data(), d_cidx + first_n, sizeof(int64_t) * more, hipMemcpyDeviceToHost, s));
        DD_HIP_CHECK(hipMemcpyAsync(cv.data(), d_cval + first_n, sizeof(double) * more, hipMemcpyDeviceToHost, s));
        DD_HIP_CHECK(hipStreamSynchronize(s));
    }
    // group by >= 0.45 s from the running maximum, first maximum wins (:729-746)
    const double min_dist = 0.45 * samp_rate;                             // NOAA_MINPEAKDIST
    std::vector<int64_t> peaks;
    bool have = false;
    double cur_max = 0.0;
    int64_t cur_idx = 0;
    for (unsigned int q = 0; q < count; ++q) {
        const int64_t idx = q < first_n ? head[q].idx : ci[q - first_n];
        const double val = q < first_n ? head[q].val : cv[q - first_n];
        if (have && (double)(idx - cur_idx) >= min_dist) { peaks.push_back(cur_idx); have = false; }
        if (!have || cur_max < val) { cur_max = val; cur_idx = idx; have = true; }
    }
    if (have) peaks.push_back(cur_idx);
    // the reference appends currentMaxIndex even when there was no candidate (None): an
    // empty candidate list cannot happen (the maximum itself exceeds the threshold)
    const int shift = needle_len / 2;                                     // int(len(sync)/2) (:749)
    for (auto& p : peaks) p -= shift;
    std::sort(peaks.begin(), peaks.end());
    if ((int)peaks.size() > max_peaks) {
        dd_set_error("%s: %d peaks found, buffer holds %d", who, (int)peaks.size(), max_peaks);
        return DD_ERR_INVALID;
    }
    for (size_t i = 0; i < peaks.size(); ++i) peaks_host[i] = peaks[i];
    *n_peaks = (int)peaks.size();
    return DD_OK;
}

extern "C" int dd_find_peaks_f64(const double* cor, int64_t n, double samp_rate, int needle_len,
                                 int64_t* peaks_host, int max_peaks, int* n_peaks, void* stream) {
    DD_REQUIRE(cor && n >= 1 && samp_rate > 0 && peaks_host && n_peaks && max_peaks >= 1, "arguments");
    DD_REQUIRE(n < ((int64_t)1 << 31), "n (the peak pick counts in 32 bits)");
    hipStream_t s = dd_stream(stream);
    const int K = (int)(2 * ((double)n / samp_rate)) + 2;                 // expectedPeaks (:714)
    DD_REQUIRE(K <= n, "signal shorter than the expected peak count");
    // ---- all intermediates from the scratch arena: [selection | above K | below K | wave counts | head | overflow idx n | overflow val n]
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_bey = al(sizeof(DDCrudeSel)), o_cnt = o_bey + al(sizeof(double) * 2 * K), o_head = o_cnt + al(sizeof(unsigned int) * DD_CS_WAVES);
    const size_t o_ci = o_head + al(sizeof(DDCand) * DD_CS_HEAD), o_cv = o_ci + al(sizeof(int64_t) * n);
    std::lock_guard<std::mutex> lk(g_sync_mu);
    char* base = nullptr;
    int rc = sync_scratch(o_cv + al(sizeof(double) * n), &base);
    if (rc != DD_OK) return rc;
    DDCrudeSel* sel = (DDCrudeSel*)base;
    double* d_bey = (double*)(base + o_bey);
    unsigned int* d_cnt = (unsigned int*)(base + o_cnt);
    DDCand* d_head = (DDCand*)(base + o_head);
    int64_t* d_ci = (int64_t*)(base + o_ci);
    double* d_cv = (double*)(base + o_cv);
    // ---- mean of the K largest and K smallest values (argpartition, :717-723): radix select, the 2 K values sorted and summed here
    // (any K; the crude tail's k_cs_threshold does the same on the device for K <= DD_CS_KMAX)
    DD_HIP_CHECK(hipMemsetAsync(sel, 0, sizeof(DDCrudeSel), s));
    for (int pass = 0; pass < 8; ++pass) hipLaunchKernelGGL(k_cs_hist, dim3(DD_CS_WG, 1), dim3(256), 0, s, cor, n, K, pass, sel);
    hipLaunchKernelGGL(k_cs_collect, dim3(DD_CS_WG, 1), dim3(256), 0, s, cor, n, K, sel, d_bey, (unsigned int)K, (unsigned int)K);
    hipLaunchKernelGGL(k_cs_keys, dim3(1), dim3(128), 0, s, K, sel);
    DD_LAUNCH_CHECK();
    DDCrudeSel h1;                                                        // (only what lies behind the histograms is fetched)
    const size_t o_tail = offsetof(DDCrudeSel, n_beyond);
    std::vector<double> bey(2 * (size_t)K);
    DD_HIP_CHECK(hipMemcpyAsync((char*)&h1 + o_tail, base + o_tail, sizeof(h1) - o_tail, hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipMemcpyAsync(bey.data(), d_bey, sizeof(double) * 2 * K, hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    auto unkey = [](unsigned long long k) {
        const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
        double d;
        memcpy(&d, &u, sizeof(d));
        return d;
    };
    DD_REQUIRE(h1.n_beyond[0] == h1.beyond_cnt[0] && h1.n_beyond[1] == h1.beyond_cnt[1] && h1.n_beyond[0] < (unsigned int)K && h1.n_beyond[1] < (unsigned int)K,
               "dd_find_peaks_f64: selection bookkeeping (internal)");
    double sums[2];
    for (int w = 0; w < 2; ++w) {
        double* v = bey.data() + (size_t)w * K;
        for (unsigned int i = h1.n_beyond[w]; i < (unsigned int)K; ++i) v[i] = unkey(h1.key[w]);      // the K-th itself and its ties
        std::sort(v, v + K);
        sums[w] = 0.0;
        for (int i = 0; i < K; ++i) sums[w] += v[i];                      // ascending, like the sums over the sorted array they replace
    }
    double avgpk = sums[0] / K;
    avgpk -= 0.25 * (avgpk - sums[1] / K);                                // NOAA_PEAKHEIGHTWIGGLE (:723)
    // ---- candidates cor > threshold, ascending index (:726), with their heights
    DD_HIP_CHECK(hipMemcpyAsync(&sel->thr, &avgpk, sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_cs_cand_count, dim3(DD_CS_WG, 1), dim3(256), 0, s, cor, n, sel, d_cnt);
    hipLaunchKernelGGL(k_cs_cand_write, dim3(DD_CS_WG, 1), dim3(256), 0, s, cor, n, (const DDCrudeSel*)sel, (const unsigned int*)d_cnt, d_head, d_ci, d_cv, (unsigned int)n);
    DD_LAUNCH_CHECK();
    unsigned int count = 0;
    DD_HIP_CHECK(hipMemcpyAsync(&count, &sel->n_cand, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<DDCand> head(count < DD_CS_HEAD ? count : DD_CS_HEAD);
    if (!head.empty()) {
        DD_HIP_CHECK(hipMemcpyAsync(head.data(), d_head, sizeof(DDCand) * head.size(), hipMemcpyDeviceToHost, s));
        DD_HIP_CHECK(hipStreamSynchronize(s));
    }
    return peaks_from_candidates("dd_find_peaks_f64", count, head.data(), d_ci, d_cv, samp_rate, needle_len, peaks_host, max_peaks, n_peaks, s);
}
