// Funcube telemetry frames (beyond the reference; DESIGN.md section 4.17 defines every stage bit for bit, funcube_fec.py restates it
// in NumPy), included by dd_afsk.hip after dd_fec.h, dd_lrpt_rs.h and dd_funcube.h.  All arithmetic is integer.
//
//   k_fc_diff     -- ten-symbol bit sums of the int8 soft symbols and the differential metric D of two sums ten symbols apart
//   k_fc_sync     -- the 65-bit sync vector, spread over a frame at stride 800, against D at every position: (position,
//                    correlation, score) of every score >= min_score is a candidate
//   k_fc_viterbi  -- one wave per frame: the de-interleaving gather, the terminated K = 7 trellis with lane = state (dd_fec.h),
//                    descrambling, and the re-encode count
//   k_fc_rs       -- one wave per codeword of the (160,128) code, two per frame: the word behind 95 zero bytes, decoded by
//                    dd_rs_wave; a root among the 95 rejects the word
//
// The format's constants (public descriptions of the AO-40 FEC block; not checked against a recording) are all here.
#pragma once

#define DD_FCF_SPB 10                  // symbols per channel bit
#define DD_FCF_SYNC 65                 // sync bits; sync bit k is channel bit 80 k
#define DD_FCF_ROWS 80                 // slot s is channel bit 80 (s % 65) + s / 65
#define DD_FCF_CHANNEL 5200            // channel bits per frame
#define DD_FCF_CODE 5132               // code bits, at slots 65 .. 5196
#define DD_FCF_STEPS 2566              // trellis steps: 2560 data bits and 6 tail zeros
#define DD_FCF_BLOCK 320               // the scrambled block's bytes: two interleaved codewords
#define DD_FCF_FRAME 256               // telemetry bytes
#define DD_FCF_RS_DATA 128
#define DD_FCF_RS_PAD 95               // RS(255,223) shortened by 95 leading zero bytes to (160,128)
#define DD_FCF_SYNC_START 0x7F         // the sync vector's 7-bit register, output bit 6 ...
#define DD_FCF_SYNC_TAPS 0x48          // ... and feedback parity(sr & 0x48)
#define DD_FCF_START (-(1 << 24))      // the start metric of the states other than 0
#define DD_FCF_SPAN ((int64_t)DD_FCF_SPB * (DD_FCF_CHANNEL - 1) + 1)        // entries of D a frame spans
#define DD_FCF_STEPS_PAD ((DD_FCF_STEPS + 63) / 64 * 64)

struct DDFcFormat {
    int8_t sync[DD_FCF_SYNC];         // 2 V[k] - 1
};

static constexpr DDFcFormat dd_fc_make_format() {
    DDFcFormat f{};
    int sr = DD_FCF_SYNC_START;
    for (int k = 0; k < DD_FCF_SYNC; ++k) {
        f.sync[k] = (int8_t)(2 * ((sr >> 6) & 1) - 1);
        int t = sr & DD_FCF_SYNC_TAPS, par = 0;
        for (; t; t >>= 1) par ^= t & 1;
        sr = ((sr << 1) | par) & 0x7F;
    }
    return f;
}

__constant__ DDFcFormat dd_fc_format = dd_fc_make_format();

// D[i] for i = 256 blockIdx.x + threadIdx.x < n - 19: the workgroup's 256 + 19 soft symbols (0 past the end) and their 256 + 10 sums
__global__ void __launch_bounds__(256) k_fc_diff(const char2* __restrict__ soft, int64_t n, int8_t* __restrict__ D) {
    __shared__ int r[256 + 2 * DD_FCF_SPB - 1];
    __shared__ int S[256 + DD_FCF_SPB];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 256;
    for (int i = tid; i < 256 + 2 * DD_FCF_SPB - 1; i += 256) r[i] = i0 + i < n ? (int)(signed char)soft[i0 + i].x : 0;
    __syncthreads();
    for (int i = tid; i < 256 + DD_FCF_SPB; i += 256) {
        int s = 0;
        for (int j = 0; j < DD_FCF_SPB; ++j) s += r[i + j];
        S[i] = s;
    }
    __syncthreads();
    if (i0 + tid + 2 * DD_FCF_SPB - 1 >= n) return;
    const int a = S[tid + DD_FCF_SPB], b = S[tid];
    const int ma = a < 0 ? -a : a, mb = b < 0 ? -b : b;              // int32: 10 * -128 survives
    int mag = (ma < mb ? ma : mb) / DD_FCF_SPB;
    mag = mag > 127 ? 127 : mag;
    const int v = ((a < 0) != (b < 0)) ? mag : -mag;                  // a phase flip is channel bit 1
    D[i0 + tid] = (int8_t)((a == 0 || b == 0) ? 0 : v);
}

// one position per thread: 65 reads at stride 800, consecutive threads on consecutive bytes
__global__ void __launch_bounds__(256) k_fc_sync(const int8_t* __restrict__ D, int64_t npos, int min_score, int64_t cap,
                                                  int64_t* __restrict__ cand, unsigned long long* __restrict__ count) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npos) return;
    const int8_t* src = D + p;
    int C = 0, pos = 0, neg = 0;
#pragma unroll 13
    for (int k = 0; k < DD_FCF_SYNC; ++k) {
        const int d = src[(int64_t)(DD_FCF_ROWS * DD_FCF_SPB) * k];
        const int v = dd_fc_format.sync[k];
        C += v * d;
        pos += (d > 0) == (v > 0);
        neg += (d < 0) == (v > 0);
    }
    const int score = C < 0 ? neg : pos;
    if (score < min_score) return;
    if (int64_t* t = dd_cand_slot(cap, cand, count)) {
        t[0] = p;
        t[1] = C;
        t[2] = score;
    }
}

// Frame blockIdx.x = (p, inv), one wave.  xs[j] = D[p + 10 pos(j)], kept as received and negated in int32 where inv (-(-128) = 128
// survives).  Then dd_fec.h's trellis over all 2566 steps, the decision words of 64 steps going to LDS together.  State 0 starts at 0
// and the others at -(1 << 24); traceback starts from state 0.  Metrics stay within 2566 * 256 of their start: int32.  The
// workgroup is one wave and no lane leaves early: every barrier is met by all 64 lanes.
__global__ void __launch_bounds__(64) k_fc_viterbi(const int8_t* __restrict__ D, const int64_t* __restrict__ frames,
                                                    uint8_t* __restrict__ blocks, int* __restrict__ corrected) {
    __shared__ unsigned long long dec[DD_FCF_STEPS_PAD];
    __shared__ int8_t xs[2 * DD_FCF_STEPS_PAD];
    __shared__ uint8_t ob[DD_FCF_STEPS_PAD];
    const int lane = threadIdx.x;
    const int64_t f = blockIdx.x;
    const int8_t* src = D + frames[2 * f];
    const int sgn = frames[2 * f + 1] ? -1 : 1;
    for (int j = lane; j < 2 * DD_FCF_STEPS_PAD; j += 64) {
        int8_t v = 0;
        if (j < DD_FCF_CODE) {
            const int s = DD_FCF_SYNC + j;
            v = src[DD_FCF_SPB * (DD_FCF_ROWS * (s % DD_FCF_SYNC) + s / DD_FCF_SYNC)];
        }
        xs[j] = v;
    }
    __syncthreads();
    const int T = DD_FCF_STEPS;
    int s1[2], s2[2];
    dd_k7_signs(lane, s1, s2);
    int m = lane == 0 ? 0 : DD_FCF_START;
    for (int c = 0; c < T; c += 64) {
        const int a = sgn * xs[2 * (c + lane)], b = sgn * xs[2 * (c + lane) + 1];      // 0 past the last step
        dec[c + lane] = dd_k7_acs(a, b, T - c < 64 ? T - c : 64, lane, s1, s2, m);
    }
    __syncthreads();
    int st = 0;                                                       // the trellis is terminated
    for (int c = ((T - 1) >> 6) << 6; c >= 0; c -= 64)                // every step is inside the window: step j of the group to ob[c + j]
        st = dd_k7_traceback(dec[c + lane], T - c < 64 ? T - c : 64, -c, 64, st, lane, ob);
    __syncthreads();
    for (int i = lane; i < DD_FCF_BLOCK; i += 64) {
        uint32_t byte = 0;
        for (int q = 0; q < 8; ++q) byte = (byte << 1) | ob[8 * i + q];
        blocks[f * DD_FCF_BLOCK + i] = (uint8_t)(byte ^ dd_pn.b[i % 255]);
    }
    // step t: r = the decoded bits t-6 .. t, bit t in r's bit 6, zeros before the first (the encoder starts in state 0)
    int mine = 0;
    for (int t = lane; t < T; t += 64) {
        int r = 0;
        for (int j = 0; j < 7; ++j) {
            const int u = t - 6 + j;
            r |= (u >= 0 ? (int)ob[u] : 0) << j;
        }
        mine += dd_k7_mismatch(r, sgn * xs[2 * t], sgn * xs[2 * t + 1]);
    }
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if (lane == 0) corrected[f] = mine;
}

// Frame blockIdx.x, codeword w = the wave: row[1 + i] = byte i of the (255,223) word, 0 for i < 95 and block[w + 2 (i - 95)] after.
// A root among the 95 would put a non-zero byte where the shortened code has none.  dd_rs_wave's rule holds below the staging barrier.
__global__ void __launch_bounds__(128) k_fc_rs(const uint8_t* __restrict__ blocks, uint8_t* __restrict__ frames, int* __restrict__ errors) {
    __shared__ uint8_t ex[512];
    __shared__ uint8_t lg[256];
    __shared__ uint8_t cw[2][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t f = blockIdx.x;
    for (int i = tid; i < 512; i += 128) ex[i] = dd_rs_tables.ex[i];
    for (int i = tid; i < 256; i += 128) lg[i] = dd_rs_tables.lg[i];
    for (int i = tid; i < 2 * (1 + DD_FCF_RS_PAD); i += 128) cw[i / (1 + DD_FCF_RS_PAD)][i % (1 + DD_FCF_RS_PAD)] = 0;
    for (int i = tid; i < DD_FCF_BLOCK; i += 128) cw[i & 1][1 + DD_FCF_RS_PAD + (i >> 1)] = blocks[f * DD_FCF_BLOCK + i];
    __syncthreads();

    uint8_t* row = cw[w];
    int pos[4], got[4], out[4];
    for (int q = 0; q < 4; ++q) {
        pos[q] = lane + 64 * q;
        got[q] = pos[q] < DD_RS_N ? row[1 + pos[q]] : 0;
        out[q] = got[q];
    }
    const int nerr = dd_rs_wave<DD_RS_T, DD_RS_BETA, DD_RS_ROOT0>(ex, lg, row, lane, pos, got, out, DD_FCF_RS_PAD);
    uint8_t* dst = frames + f * DD_FCF_FRAME + w;
    for (int q = 0; q < 4; ++q) {
        const int k = pos[q] - DD_FCF_RS_PAD;
        if (k >= 0 && k < DD_FCF_RS_DATA) dst[2 * k] = (uint8_t)out[q];
    }
    if (lane == 0) errors[2 * f + w] = nerr;
}

extern "C" int dd_fc_diff(const int8_t* soft, int64_t nsym, int8_t* D, void* stream) {
    DD_REQUIRE(nsym >= 0 && nsym / 256 < 0x7fffffff, "dd_fc_diff: sizes");
    if (nsym < 2 * DD_FCF_SPB) return DD_OK;
    DD_REQUIRE(soft != nullptr && D != nullptr, "dd_fc_diff: null buffer");
    const int64_t m = nsym - (2 * DD_FCF_SPB - 1);
    hipLaunchKernelGGL(k_fc_diff, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, dd_stream(stream), (const char2*)soft, nsym, D);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_fc_sync_search(const int8_t* D, int64_t m, int min_score, int64_t cap, int64_t* cand, unsigned long long* count,
                                 void* stream) {
    DD_REQUIRE(m >= 0 && m / 256 < 0x7fffffff && cap >= 0 && count != nullptr, "dd_fc_sync_search: sizes");
    DD_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned long long), dd_stream(stream)));
    if (m < DD_FCF_SPAN) return DD_OK;
    DD_REQUIRE(D != nullptr && (cap == 0 || cand != nullptr), "dd_fc_sync_search: null buffer");
    const int64_t npos = m - (DD_FCF_SPAN - 1);
    hipLaunchKernelGGL(k_fc_sync, dim3((unsigned)((npos + 255) / 256)), dim3(256), 0, dd_stream(stream), D, npos, min_score, cap, cand,
                       count);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_fc_viterbi(const int8_t* D, int64_t m, const int64_t* frames_host, int64_t nframes, uint8_t* blocks,
                             int32_t* corrected, void* stream) {
    DD_REQUIRE(m >= 0 && nframes >= 0 && nframes <= 0x7fffffff, "dd_fc_viterbi: sizes");
    if (nframes == 0) return DD_OK;
    DD_REQUIRE(D != nullptr && frames_host != nullptr && blocks != nullptr && corrected != nullptr, "dd_fc_viterbi: null buffer");
    for (int64_t i = 0; i < nframes; ++i) {
        const int64_t p = frames_host[2 * i], inv = frames_host[2 * i + 1];
        DD_REQUIRE(inv == 0 || inv == 1, "dd_fc_viterbi: polarity outside 0..1");
        DD_REQUIRE(p >= 0 && p <= m - DD_FCF_SPAN, "dd_fc_viterbi: frame outside D");
    }
    return dd_with_spans(frames_host, nframes, "dd_fc_viterbi", stream, [&](const int64_t* d) {
        hipLaunchKernelGGL(k_fc_viterbi, dim3((unsigned)nframes), dim3(64), 0, dd_stream(stream), D, d, blocks, corrected);
    });
}

extern "C" int dd_fc_rs(const uint8_t* blocks, int64_t nframes, uint8_t* frames, int32_t* errors, void* stream) {
    DD_REQUIRE(nframes >= 0 && nframes <= 0x7fffffff, "dd_fc_rs: sizes");
    if (nframes == 0) return DD_OK;
    DD_REQUIRE(blocks != nullptr && frames != nullptr && errors != nullptr, "dd_fc_rs: null buffer");
    hipLaunchKernelGGL(k_fc_rs, dim3((unsigned)nframes), dim3(128), 0, dd_stream(stream), blocks, frames, errors);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
