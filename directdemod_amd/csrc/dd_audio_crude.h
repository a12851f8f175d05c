// getCrudeSync's audio-rate tail in one host call (decode_noaa.py:769-806): dd_noaa_crude_tail -- the orchestration, the library-route
// envelope helpers, and what only the fused peak pick has: the threshold on the device (k_cs_threshold) and the header of its one
// copy back (k_cs_head).  The block envelope, the scan, the correlation and the peak pick's other kernels are the shared ones of
// dd_audio_envelope.h and dd_audio_xcorr.h.
// One of the six parts of dd_audio.hip (one translation unit: the parts share the plan cache, the float64 transform and the scratch
// buffers of dd_audio.hip and are included there, each using only the parts before it).  Internal; not a stand-alone header.
// ---------------------------------------------------------------- getCrudeSync's audio-rate tail in ONE host call
// decode_noaa.py:781-790: envelope of the FM audio in 240 000-sample blocks (__getAM :631-657 -> demod_am.py:29), then for sync A
// and sync B the normalised correlation (:659-675) and the peak pick (:713-751).  Stage by stage through the entry points
// above that was ~70 launches, a dozen host round trips and -- measured at 60 s of recording -- 2.0 of the 2.2 ms of the crude
// sync (profiles/r03_side_benchmarks.txt); the samples themselves are 3.6 M doubles.  Here:
//   * envelope = hypot(x, H x) with H x from a real-to-complex / complex-to-real transform pair per block (bin k of the
//     spectrum times -j for 0 < k < N/2, zero at DC and Nyquist: the imaginary part of scipy.signal.hilbert's analytic
//     signal) -- half the transform work of the complex pair, batched over the full blocks;
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
// with the complex-transform form to ~1e-15 relative.
#define DD_CS_KMAX 2048               // largest K (two per second of audio + 2) the in-kernel sort holds

__global__ void __launch_bounds__(256) k_cvt_f32_f64(const float* __restrict__ in, double* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}
// spectrum of a real block -> spectrum of its Hilbert transform (blockIdx.y = block of the batch; nb = N/2 + 1 bins)
__global__ void __launch_bounds__(256) k_hilb_bins(double2* __restrict__ S, int64_t nb, int64_t N) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nb) return;
    double2* p = S + (int64_t)blockIdx.y * nb + k;
    const double2 v = *p;
    const bool zero = k == 0 || (2 * k == N);
    *p = zero ? make_double2(0.0, 0.0) : make_double2(v.y, -v.x);          // -j X[k]
}
__global__ void __launch_bounds__(256) k_env_hypot_flat(const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ env, int64_t n, double inv_n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) env[i] = hypot(x[i], y[i] * inv_n);
}
__global__ void __launch_bounds__(256) k_pad_f64(const double* __restrict__ x, int64_t n, double* __restrict__ XR, int64_t M) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < M) XR[j] = j < n ? x[j] : 0.0;
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
    // block list by the chunker rule (decode_noaa.py:644-653 via chunker.py:36-45)
    int64_t nfull = 0;
    while ((nfull + 1) * block < n) ++nfull;
    const int64_t rem = n - nfull * block;
    const int GB = 16;
    const int64_t gb = nfull < GB ? nfull : GB;
    const int64_t nbins_b = block / 2 + 1, nbins_r = rem / 2 + 1;
    const int tiles = (int)((n + DD_SCAN_TILE - 1) / DD_SCAN_TILE);
    const unsigned int cap = 1u << 16;                                    // candidates per needle held on the device
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al(bytes); return o; };
    const size_t o_x = take(audio_is_f32 ? sizeof(double) * (size_t)n : 0);
    const size_t o_env = take(env_out ? 0 : sizeof(double) * (size_t)n);
    // the ragged last block: a length with a large prime factor (14 100 = 2^2 3 5^2 47 for a minute of audio) makes the library
    // run Bluestein's algorithm -- twenty launches for 14 100 samples.  Its envelope then goes through the zero-padded cyclic
    // convolution with the Hilbert kernel that the accurate-sync windows use (hilbert_kernel_spectrum): four launches and two
    // power-of-two transforms.
    int64_t Mr = 0;
    if (rem >= 2 && largest_prime_factor(rem) > 17) { Mr = 1; while (Mr < 2 * rem + 2) Mr <<= 1; }
    const size_t spec_r = (size_t)(Mr ? Mr / 2 + 1 : nbins_r);
    const size_t spec_elems = (size_t)(gb * nbins_b) > spec_r ? (size_t)(gb * nbins_b) : spec_r;
    const size_t o_spec = take(sizeof(double2) * spec_elems);
    const size_t y_r = (size_t)(Mr ? 2 * Mr : rem);
    const size_t o_y = take(sizeof(double) * ((size_t)(gb * block) > y_r ? (size_t)(gb * block) : y_r));
    // Round 5: the blocks' envelopes through the own float64 transform (hc_block_envelope: the even / odd split of the Hilbert kernel puts a
    // 240 000-sample block on the cyclic length 2^18) -- no FFT-library plan on this path, whose creation was 0.9 s of a process's first call.
    // DD_AM_HILBERT=lib (tools / tests) keeps the library's transforms.
    static const char* amh_env = getenv("DD_AM_HILBERT");
    const bool own_ok = !(amh_env && !strcmp(amh_env, "lib"));
    bool split_b = false, split_r = false;
    const int64_t Mb_own = (own_ok && nfull > 0) ? hc_block_len(block, &split_b) : 0;
    const int64_t Mr_own = (own_ok && rem >= 2) ? hc_block_len(rem, &split_r) : 0;
    const int64_t T_elems = std::max<int64_t>(Mb_own && split_b ? gb * Mb_own : (Mb_own ? Mb_own : 0), Mr_own);
    const size_t o_T = take(sizeof(double2) * (size_t)T_elems);
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
    double2* spec = (double2*)(base + o_spec);
    double* y = (double*)(base + o_y);
    double* P = (double*)(base + o_P);
    double* Q = (double*)(base + o_Q);
    double2* part = (double2*)(base + o_part);
    double* cor = (double*)(base + o_cor);
    DDCrudeSel* sel = (DDCrudeSel*)(base + o_sel);
    static const char* tenv = getenv("DD_CRUDE_TRACE");
    const bool trace = tenv && atoi(tenv);
    auto now_us = []() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tt0 = now_us();
    double tt[6] = {0, 0, 0, 0, 0, 0};
    if (audio_is_f32) hipLaunchKernelGGL(k_cvt_f32_f64, dim3(grid1(n)), dim3(256), 0, s, (const float*)audio, (double*)(base + o_x), n);
    // ---- envelope
    auto env_blocks = [&](int64_t first, int64_t N, int batch) -> int {
        hipfftHandle pf, pb;
        int r = get_plan(&pf, HIPFFT_D2Z, N, batch, s);
        if (r == DD_OK) r = get_plan(&pb, HIPFFT_Z2D, N, batch, s);
        if (r != DD_OK) return r;
        const int64_t nb = N / 2 + 1;
        DD_FFT_CHECK(hipfftExecD2Z(pf, (hipfftDoubleReal*)(x + first), (hipfftDoubleComplex*)spec));
        hipLaunchKernelGGL(k_hilb_bins, dim3(grid1(nb), batch), dim3(256), 0, s, spec, nb, N);
        DD_FFT_CHECK(hipfftExecZ2D(pb, (hipfftDoubleComplex*)spec, (hipfftDoubleReal*)y));
        hipLaunchKernelGGL(k_env_hypot_flat, dim3(grid1(N * batch)), dim3(256), 0, s, x + first, y, env + first, N * batch, 1.0 / (double)N);
        return DD_OK;
    };
    double2* Tw = (double2*)(base + o_T);
    if (Mb_own) {
        // (plain form: one block per call; split form: a batch of blocks, one complex image each)
        const int per = split_b ? (int)gb : 1;
        for (int64_t b0 = 0; b0 < nfull && rc == DD_OK; b0 += per)
            rc = hc_block_envelope(x + b0 * block, env + b0 * block, block, (int)(nfull - b0 < per ? nfull - b0 : per), split_b, Mb_own, Tw, s);
    } else {
        for (int64_t b0 = 0; b0 < nfull && rc == DD_OK; b0 += GB) rc = env_blocks(b0 * block, block, (int)(nfull - b0 < GB ? nfull - b0 : GB));
    }
    tt[0] = now_us() - tt0;
    if (rc == DD_OK && Mr_own) {
        rc = hc_block_envelope(x + nfull * block, env + nfull * block, rem, 1, split_r, Mr_own, Tw, s);
    } else if (rc == DD_OK && Mr) {
        const double2* HH = nullptr;
        rc = hilbert_kernel_spectrum(rem, Mr, &HH, s);
        hipfftHandle pf, pb;
        if (rc == DD_OK) rc = get_plan(&pf, HIPFFT_D2Z, Mr, 1, s);
        if (rc == DD_OK) rc = get_plan(&pb, HIPFFT_Z2D, Mr, 1, s);
        if (rc == DD_OK) {
            double* XR = y, *YR = y + Mr;
            const int64_t nb = Mr / 2 + 1;
            hipLaunchKernelGGL(k_pad_f64, dim3(grid1(Mr)), dim3(256), 0, s, x + nfull * block, rem, XR, Mr);
            DD_FFT_CHECK(hipfftExecD2Z(pf, XR, (hipfftDoubleComplex*)spec));
            hipLaunchKernelGGL(k_spec_mul, dim3(grid1(nb), 1), dim3(256), 0, s, spec, HH, nb);
            DD_FFT_CHECK(hipfftExecZ2D(pb, (hipfftDoubleComplex*)spec, YR));
            hipLaunchKernelGGL(k_env_hypot, dim3(grid1(rem), 1), dim3(256), 0, s, XR, YR, Mr, rem, env + nfull * block);
        }
    } else if (rc == DD_OK) {
        rc = env_blocks(nfull * block, rem, 1);
    }
    if (rc != DD_OK) return rc;
    tt[1] = now_us() - tt0;
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
    tt[2] = now_us() - tt0;
    char* pin = nullptr;
    rc = sync_pinned(head_bytes, &pin);
    if (rc != DD_OK) return rc;
    DD_HIP_CHECK(hipMemcpyAsync(pin, base + o_head, head_bytes, hipMemcpyDeviceToHost, s));
    tt[3] = now_us() - tt0;
    DD_HIP_CHECK(hipStreamSynchronize(s));
    sync_guard.done();
    { const int sr = dd_seam_poll_all(); if (sr != DD_OK) return sr; }        // (the audio may come from a chunk-list launch on this stream)
    tt[4] = now_us() - tt0;
    if (trace) fprintf(stderr, "crude tail host us: blocks enqueued %.0f, remainder %.0f, tail enqueued %.0f, copy enqueued %.0f, synchronised %.0f\n", tt[0], tt[1], tt[2], tt[3], tt[4]);
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
