// getCrudeSync's audio-rate tail in one host call (decode_noaa.py:769-806): dd_noaa_crude_tail -- the orchestration, and what only
// the fused peak pick has: the threshold on the device (k_cs_threshold) and the header of its one copy back (k_cs_head).  The
// envelope is the block walk of dd_audio_envelope.h (envelope_plan / envelope_walk: the walk dd_am_envelope_f64 runs, every route of
// it); the scan, the correlation and the peak pick's other kernels are the shared ones of dd_audio_xcorr.h.
// One of the six parts of dd_audio.hip (one translation unit: the parts share the plan cache, the float64 transform and the scratch
// buffers of dd_audio.hip and are included there, each using only the parts before it).  Internal; not a stand-alone header.
// ---------------------------------------------------------------- getCrudeSync's audio-rate tail in ONE host call
// decode_noaa.py:781-790: envelope of the FM audio in 240 000-sample blocks (__getAM :631-657 -> demod_am.py:29), then for sync A
// and sync B the normalised correlation (:659-675) and the peak pick (:713-751).  Stage by stage through the entry points
// above that was ~70 launches, a dozen host round trips and -- measured at 60 s of recording -- 2.0 of the 2.2 ms of the crude
// sync (profiles/r03_side_benchmarks.txt); the samples themselves are 3.6 M doubles.  Here:
//   * the envelope block by block as ONE enqueue of the shared walk (own float64 transform where a block fits it, else the
//     library's real transform pair, batched over the full blocks);
//   * prefix sums of the envelope and its square ONCE, both needles correlated in one launch (blockIdx.y);
//   * the means of the K largest / K smallest correlation values, the threshold and the candidate list of BOTH needles in
//     eleven launches that never come back to the host: eight radix-select passes (one byte of the order-preserving key
//     each; every workgroup re-derives the bins picked so far from the earlier passes' global histograms, so no pick
//     kernel sits between them), the collection of the values beyond the K-th, their sort and ascending summation
//     (one workgroup per needle), the candidates by atomic append -- instead of 2 x 19 dependent launches and 2 x 2 host
//     round trips.  (Tried first: all of it as ONE persistent launch with grid-wide barriers.  It measured 0.56-0.76 ms:
//     ten barriers of 2 x 128..512 workgroups polling one word each cost more than the launch boundaries they replaced,
//     profiles/r04_noaa_stages.txt);
//   * one host synchronisation at the end (the grouping by 0.45 s of :729-746 runs on the host over a few thousand candidates).
// Results: the index lists are those of the staged route and of the reference (tests/golden/noaa_c4*.npz); the envelope agrees
// with scipy.signal.hilbert's complex-transform form to ~1e-15 relative.
#define DD_CS_KMAX 2048               // largest K (two per second of audio + 2) the in-kernel sort holds

__global__ void __launch_bounds__(256) k_cvt_f32_f64(const float* __restrict__ in, double* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}
// one workgroup per needle: the K largest (then the K smallest) sorted ascending and summed in that order (the sums over the
// sorted array that np.argpartition's slices stand for, :717-723), threshold
__global__ void __launch_bounds__(256) k_cs_threshold(int K, DDCrudeSel* __restrict__ sel_all, const double* __restrict__ beyond_all) {
    __shared__ double srt[DD_CS_KMAX];
    __shared__ DDCsState tmp;
    const int nd = blockIdx.x, t = threadIdx.x;
    DDCrudeSel* S = sel_all + nd;
    const double* above = beyond_all + (size_t)nd * 2 * DD_CS_KMAX;
    const double* below = above + DD_CS_KMAX;
    const DDCsState st = dd_cs_state(S, 8, K, &tmp);
    double sums[2] = {0.0, 0.0};
    for (int w = 0; w < 2; ++w) {
        const unsigned int nb = st.beyond[w];
        const unsigned long long kk = st.prefix[w];
        const unsigned long long u = (kk >> 63) ? (kk & 0x7fffffffffffffffull) : ~kk;
        const double kth = __longlong_as_double((long long)u);
        const double* src = w ? below : above;
        int np2 = 1;
        while (np2 < K) np2 <<= 1;
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        for (int i = t; i < np2; i += 256) srt[i] = i < (int)nb ? src[i] : (i < K ? kth : inf);
        __syncthreads();
        for (int k2 = 2; k2 <= np2; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = t; i < np2; i += 256) {
                    const int ixj = i ^ j;
                    if (ixj > i) {
                        const double a = srt[i], b = srt[ixj];
                        const bool up = (i & k2) == 0;
                        if (up ? (a > b) : (a < b)) { srt[i] = b; srt[ixj] = a; }
                    }
                }
                __syncthreads();
            }
        if (t == 0) {
            double acc = 0.0;
            for (int i = 0; i < K; ++i) acc += srt[i];
            sums[w] = acc;
            if (w == 0) S->sum_hi = acc; else S->sum_lo = acc;
        }
        __syncthreads();
    }
    if (t == 0) {
        double avgpk = sums[0] / K;
        avgpk -= 0.25 * (avgpk - sums[1] / K);                             // NOAA_PEAKHEIGHTWIGGLE (:723)
        S->thr = avgpk;
        S->key[0] = st.prefix[0]; S->key[1] = st.prefix[1];
        S->beyond_cnt[0] = st.beyond[0]; S->beyond_cnt[1] = st.beyond[1];
    }
}
// what the host needs of the selection records, in front of the candidates' head block (k_cs_cand_write) in the entry's one copy back
struct DDCrudeHead { unsigned int n_cand, n_beyond[2], beyond_cnt[2], pad[3]; };      // 32 bytes per needle, then DDCand[needles][DD_CS_HEAD]
__global__ void k_cs_head(const DDCrudeSel* __restrict__ sel, DDCrudeHead* __restrict__ hdr, int n_needles) {
    const int d = threadIdx.x;
    if (d >= n_needles) return;
    DDCrudeHead h = {sel[d].n_cand, {sel[d].n_beyond[0], sel[d].n_beyond[1]}, {sel[d].beyond_cnt[0], sel[d].beyond_cnt[1]}, {0, 0, 0}};
    hdr[d] = h;
}

extern "C" int dd_noaa_crude_tail(const void* audio, int audio_is_f32, int64_t n, double samp_rate, int64_t block,
                                  const double* needles_host, int m, int n_needles, double* env_out,
                                  int64_t* peaks_host, int max_peaks, int* n_peaks, void* stream) {
    DD_REQUIRE(audio && n >= 1 && samp_rate > 0 && block >= 1 && needles_host && m >= 1 && m <= n, "arguments");
    DD_REQUIRE(n_needles >= 1 && n_needles <= DD_CS_MAXNEEDLES && peaks_host && n_peaks && max_peaks >= 1, "arguments");
    hipStream_t s = dd_stream(stream);
    const int K = (int)(2 * ((double)n / samp_rate)) + 2;                 // expectedPeaks (:714)
    DD_REQUIRE(K <= n, "signal shorter than the expected peak count");
    if (K > DD_CS_KMAX || n >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED;          // (the caller takes the staged route)
    DDRuns2 R2;
    if (!dd_runs_build(needles_host, m, n_needles, &R2)) return DD_ERR_UNSUPPORTED;
    const DDEnvWalk walk = envelope_plan(n, block);                       // the envelope's blocks, routes and work areas (dd_audio_envelope.h)
    const int tiles = (int)((n + DD_SCAN_TILE - 1) / DD_SCAN_TILE);
    const unsigned int cap = 1u << 16;                                    // candidates per needle held on the device
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al(bytes); return o; };
    const size_t o_x = take(audio_is_f32 ? sizeof(double) * (size_t)n : 0);
    const size_t o_env = take(env_out ? 0 : sizeof(double) * (size_t)n);
    const size_t o_spec = take(sizeof(double2) * walk.spec_elems), o_y = take(sizeof(double) * walk.y_elems);
    const size_t o_T = take(sizeof(double2) * walk.T_elems);
    const size_t o_P = take(sizeof(double) * (size_t)(n + 1)), o_Q = take(sizeof(double) * (size_t)(n + 1));
    const size_t o_part = take(sizeof(double2) * (size_t)tiles);
    const size_t o_cor = take(sizeof(double) * (size_t)n * n_needles);
    const size_t o_sel = take(sizeof(DDCrudeSel) * n_needles);
    const size_t o_bey = take(sizeof(double) * 2 * DD_CS_KMAX * n_needles);
    const size_t o_ci = take(sizeof(int64_t) * (size_t)cap * n_needles), o_cv = take(sizeof(double) * (size_t)cap * n_needles);
    const size_t head_bytes = sizeof(DDCrudeHead) * DD_CS_MAXNEEDLES + sizeof(DDCand) * (size_t)DD_CS_HEAD * n_needles;
    const size_t o_head = take(head_bytes);
    const size_t o_cnt = take(sizeof(unsigned int) * DD_CS_WAVES * n_needles);
    std::lock_guard<std::mutex> lk(g_sync_mu);
    char* base = nullptr;
    int rc = sync_scratch(off, &base);
    if (rc != DD_OK) return rc;
    DDSyncOnExit sync_guard(s);                       // (an early error return below leaves nothing in flight)
    const double* x = audio_is_f32 ? (const double*)(base + o_x) : (const double*)audio;
    double* env = env_out ? env_out : (double*)(base + o_env);
    double* P = (double*)(base + o_P);
    double* Q = (double*)(base + o_Q);
    double2* part = (double2*)(base + o_part);
    double* cor = (double*)(base + o_cor);
    DDCrudeSel* sel = (DDCrudeSel*)(base + o_sel);
    static const char* tenv = getenv("DD_CRUDE_TRACE");
    const bool trace = tenv && atoi(tenv);
    auto now_us = []() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tt0 = now_us();
    double tt[4] = {0, 0, 0, 0};
    if (audio_is_f32) hipLaunchKernelGGL(k_cvt_f32_f64, dim3(grid1(n)), dim3(256), 0, s, (const float*)audio, (double*)(base + o_x), n);
    rc = envelope_walk(walk, x, env, (double2*)(base + o_T), (double2*)(base + o_spec), (double*)(base + o_y), s);
    if (rc != DD_OK) return rc;
    tt[0] = now_us() - tt0;
    // ---- prefix sums once, both correlations in one launch; selection, threshold, candidates of both needles: twelve launches,
    // nothing comes back to the host in between.  (These eighteen launches of our own kernels were also replayed as ONE captured
    // graph launch -- 300 calls with identical results -- for no gain, 0.995 against 0.985 ms per call: DD_CRUDE_TRACE=1 shows the
    // host done enqueueing the whole call after 0.12 ms of the 0.53 ms the device needs.  What the call did lose was 0.45 ms on the
    // host AFTER the synchronisation, sorting candidates: k_cs_cand_write.  profiles/r04_noaa_timeline.txt)
    auto enqueue_tail = [&](hipStream_t s) -> int {
    hipLaunchKernelGGL(k_scan_part, dim3(tiles, 1), dim3(256), 0, s, env, n, tiles, part);
    hipLaunchKernelGGL(k_scan_mid, dim3(1), dim3(256), 0, s, part, tiles);
    hipLaunchKernelGGL(k_scan_final_x, dim3(tiles), dim3(256), 0, s, env, n, part, P, Q);
    xcorr_runs_launch(P, Q, n, m, R2, n_needles, cor, s);
    DD_HIP_CHECK(hipMemsetAsync(sel, 0, sizeof(DDCrudeSel) * n_needles, s));
    for (int pass = 0; pass < 8; ++pass) hipLaunchKernelGGL(k_cs_hist, dim3(DD_CS_WG, n_needles), dim3(256), 0, s, cor, n, K, pass, sel);
    hipLaunchKernelGGL(k_cs_collect, dim3(DD_CS_WG, n_needles), dim3(256), 0, s, cor, n, K, sel, (double*)(base + o_bey), (unsigned int)DD_CS_KMAX, (unsigned int)DD_CS_KMAX);
    hipLaunchKernelGGL(k_cs_threshold, dim3(n_needles), dim3(256), 0, s, K, sel, (const double*)(base + o_bey));
    DDCrudeHead* d_hdr = (DDCrudeHead*)(base + o_head);
    DDCand* d_head = (DDCand*)(base + o_head + sizeof(DDCrudeHead) * DD_CS_MAXNEEDLES);
    hipLaunchKernelGGL(k_cs_cand_count, dim3(DD_CS_WG, n_needles), dim3(256), 0, s, cor, n, sel, (unsigned int*)(base + o_cnt));
    hipLaunchKernelGGL(k_cs_cand_write, dim3(DD_CS_WG, n_needles), dim3(256), 0, s, cor, n, (const DDCrudeSel*)sel, (const unsigned int*)(base + o_cnt), d_head,
                       (int64_t*)(base + o_ci), (double*)(base + o_cv), cap);
    hipLaunchKernelGGL(k_cs_head, dim3(1), dim3(64), 0, s, sel, d_hdr, n_needles);
    DD_LAUNCH_CHECK();
    return DD_OK;
    };
    rc = enqueue_tail(s);
    if (rc != DD_OK) return rc;
    tt[1] = now_us() - tt0;
    char* pin = nullptr;
    rc = sync_pinned(head_bytes, &pin);
    if (rc != DD_OK) return rc;
    DD_HIP_CHECK(hipMemcpyAsync(pin, base + o_head, head_bytes, hipMemcpyDeviceToHost, s));
    tt[2] = now_us() - tt0;
    DD_HIP_CHECK(hipStreamSynchronize(s));
    sync_guard.done();
    { const int sr = dd_seam_poll_all(); if (sr != DD_OK) return sr; }        // (the audio may come from a chunk-list launch on this stream)
    tt[3] = now_us() - tt0;
    if (trace) fprintf(stderr, "crude tail host us: envelope enqueued %.0f, tail enqueued %.0f, copy enqueued %.0f, synchronised %.0f\n", tt[0], tt[1], tt[2], tt[3]);
    const DDCrudeHead* hs = (const DDCrudeHead*)pin;
    const DDCand* hc = (const DDCand*)(pin + sizeof(DDCrudeHead) * DD_CS_MAXNEEDLES);
    for (int d = 0; d < n_needles; ++d) {
        const DDCrudeHead& h1 = hs[d];
        DD_REQUIRE(h1.n_beyond[0] == h1.beyond_cnt[0] && h1.n_beyond[1] == h1.beyond_cnt[1] && h1.n_beyond[0] < (unsigned int)K && h1.n_beyond[1] < (unsigned int)K,
                   "dd_noaa_crude_tail: selection bookkeeping (internal)");
        const unsigned int count = h1.n_cand;
        if (count > cap) return DD_ERR_UNSUPPORTED;                       // (a threshold that lets > 65 536 values through: staged route)
        rc = peaks_from_candidates("dd_noaa_crude_tail", count, hc + (size_t)d * DD_CS_HEAD, (const int64_t*)(base + o_ci) + (size_t)d * cap,
                                   (const double*)(base + o_cv) + (size_t)d * cap, samp_rate, m, peaks_host + (size_t)d * max_peaks, max_peaks, &n_peaks[d], s);
        if (rc != DD_OK) return rc;
        if (trace) fprintf(stderr, "   needle %d: %u candidates, %d peaks, done at %.0f us\n", d, count, n_peaks[d], now_us() - tt0);
    }
    return DD_OK;
}
