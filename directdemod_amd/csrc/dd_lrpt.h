// Meteor-M2 LRPT channel decoding (beyond the reference; DESIGN.md section 4.14 defines every stage bit for bit, lrpt.py restates
// it in NumPy), included by dd_afsk.hip after dd_meteor.h and dd_fec.h.  All arithmetic is integer.
//
//   k_lrpt_soft     -- lim(re / 2), lim(im / 2) of each corrected symbol as an int8 pair
//   k_lrpt_asm_t    -- an encoded sync marker's 52 scored bits against the hard bits at every symbol, under the eight phase /
//                      IQ-swap hypotheses; (position, hypothesis, score) of every score >= min_score is a candidate
//   k_lrpt_viterbi  -- rate 1/2, K = 7 soft-decision decode: one wave per block of 512 trellis steps, through dd_fec.h's trellis
//   k_lrpt_finish   -- per frame: marker bits in error, bytes 4..1023 XOR the CCSDS pseudo-noise sequence, and how many hard input
//                      bits differ from the re-encoded decoded bits; <true> for a differential (NRZ-M) stream
#pragma once

#define DD_LRPT_FRAME 8192            // trellis steps (= symbols = decoded bits) per channel frame
#define DD_LRPT_BODY 1020             // bytes after the 4-byte marker
#define DD_LRPT_BLOCK 512             // trellis steps decoded per wave
#define DD_LRPT_WARM 128              // steps of add-compare-select before a block (warm-up) and after it (tail)
#define DD_LRPT_STEPS (DD_LRPT_BLOCK + 2 * DD_LRPT_WARM)
#define DD_LRPT_ASM 0x1ACFFC1Du
// encode(marker) from state 0, first code bit in bit 63, split into the (c1, c2) = (I, Q) halves of its 32 symbols, first symbol in
// bit 31; the first six symbols (12 code bits) depend on the previous frame's tail and are never scored
#define DD_LRPT_ASM_CODE 0x035D49C24FF2686Bull
#define DD_LRPT_SCORED 0x03FFFFFFu

// the soft pair under hypothesis h: h & 3 selects (a, b), (-b, a), (-a, -b), (b, -a); h & 4 then exchanges the two.  int32: 128 survives
__device__ __forceinline__ void dd_lrpt_hyp(int a, int b, int h, int& oa, int& ob) {
    const int r = h & 3;
    const int x = r == 0 ? a : (r == 1 ? -b : (r == 2 ? -a : b));
    const int y = r == 0 ? b : (r == 1 ? a : (r == 2 ? -b : -a));
    oa = (h & 4) ? y : x;
    ob = (h & 4) ? x : y;
}

__global__ void __launch_bounds__(256) k_lrpt_soft(const double2* __restrict__ sym, int64_t nsym, char2* __restrict__ soft) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nsym) return;
    const double2 v = sym[k];
    soft[k] = make_char2((signed char)dd_met_lim(v.x / 2.0), (signed char)dd_met_lim(v.y / 2.0));
}

// sg[i], i < n = the soft pair of symbol p0 + i as four sign bits: a > 0, b > 0, a < 0, b < 0 (0 past the last symbol).  The whole
// workgroup of 256 calls it; the caller's barrier follows.
__device__ __forceinline__ void dd_lrpt_stage_signs(const char2* __restrict__ soft, int64_t nsym, int64_t p0, int n, uint8_t* sg) {
    for (int i = threadIdx.x; i < n; i += 256) {
        uint8_t v = 0;
        if (p0 + i < nsym) {
            const char2 s = soft[p0 + i];
            v = (uint8_t)((s.x > 0) | ((s.y > 0) << 1) | ((s.x < 0) << 2) | ((s.y < 0) << 3));
        }
        sg[i] = v;
    }
}

// m[q] = sign bit q of the n <= 32 symbols from sg[0], the first in bit n - 1
__device__ __forceinline__ void dd_lrpt_sign_masks(const uint8_t* sg, int n, uint32_t (&m)[4]) {
    for (int q = 0; q < 4; ++q) m[q] = 0;
    for (int k = 0; k < n; ++k) {
        const uint32_t v = sg[k];
        for (int q = 0; q < 4; ++q) m[q] = (m[q] << 1) | ((v >> q) & 1);
    }
}

// the hard bits under hypothesis h, as dd_lrpt_hyp turns the pair: those of (a, b), (-b, a), (-a, -b), (b, -a) are (a > 0, b > 0),
// (b < 0, a > 0), (a < 0, b < 0), (b > 0, a < 0)
__device__ __forceinline__ void dd_lrpt_hyp_hard(const uint32_t (&m)[4], int h, uint32_t& hi, uint32_t& hq) {
    const int r = h & 3;
    const uint32_t x = r == 0 ? m[0] : (r == 1 ? m[3] : (r == 2 ? m[2] : m[1]));
    const uint32_t y = r == 0 ? m[1] : (r == 1 ? m[0] : (r == 2 ? m[3] : m[2]));
    hi = (h & 4) ? y : x;
    hq = (h & 4) ? x : y;
}

// one position per thread, the workgroup's 256 + 31 symbols staged; ei, eq = the (c1, c2) halves of the code word's 32 symbols,
// first symbol in bit 31
__global__ void __launch_bounds__(256) k_lrpt_asm_t(const char2* __restrict__ soft, int64_t nsym, uint32_t ei, uint32_t eq, int min_score,
                                                     int64_t cap, int64_t* __restrict__ cand, unsigned long long* __restrict__ count) {
    __shared__ uint8_t sg[256 + 31];
    const int64_t p0 = (int64_t)blockIdx.x * 256;
    dd_lrpt_stage_signs(soft, nsym, p0, 256 + 31, sg);
    __syncthreads();
    const int64_t p = p0 + threadIdx.x;
    if (p + 32 > nsym) return;
    uint32_t m[4];
    dd_lrpt_sign_masks(sg + threadIdx.x, 32, m);
    for (int h = 0; h < 8; ++h) {
        uint32_t hi, hq;
        dd_lrpt_hyp_hard(m, h, hi, hq);
        const int score = __popc(~(hi ^ ei) & DD_LRPT_SCORED) + __popc(~(hq ^ eq) & DD_LRPT_SCORED);
        if (score < min_score) continue;
        if (int64_t* t = dd_cand_slot(cap, cand, count)) {
            t[0] = p;
            t[1] = h;
            t[2] = score;
        }
    }
}

// Block blockIdx.x of span blockIdx.y: add-compare-select over the steps lo = max(0, k - 128) .. hi = min(nsym, e + 128) of the
// block's steps [k, e), all metrics 0 at lo.  The decision words of 64 steps sit one per lane (dd_k7_acs) until they go to LDS
// together.  Traceback from the largest final metric (lowest state among equals) reads them back the same way, 64 steps per LDS
// read, and the 512 bits of [k, e) leave packed MSB first.  Metrics stay below 768 * 256: int32.
__global__ void __launch_bounds__(64) k_lrpt_viterbi(const char2* __restrict__ soft, int64_t nsym, const int64_t* __restrict__ spans,
                                                      int64_t nbits, uint8_t* __restrict__ bits) {
    __shared__ unsigned long long dec[DD_LRPT_STEPS];
    __shared__ uint8_t ob[DD_LRPT_BLOCK];
    const int lane = threadIdx.x;
    const int64_t p = spans[2 * blockIdx.y];
    const int h = (int)spans[2 * blockIdx.y + 1];
    const int64_t k = p + (int64_t)blockIdx.x * DD_LRPT_BLOCK, e = k + DD_LRPT_BLOCK;
    const int64_t lo = k - DD_LRPT_WARM < 0 ? 0 : k - DD_LRPT_WARM;
    const int64_t hi = e + DD_LRPT_WARM > nsym ? nsym : e + DD_LRPT_WARM;
    const int T = (int)(hi - lo), warm = (int)(k - lo);              // T <= 768, warm <= 128
    int s1[2], s2[2];
    dd_k7_signs(lane, s1, s2);
    int m = 0;
    for (int c = 0; c < T; c += 64) {
        int a = 0, b = 0;
        if (c + lane < T) {
            const char2 s = soft[lo + c + lane];
            dd_lrpt_hyp(s.x, s.y, h, a, b);
        }
        const unsigned long long w = dd_k7_acs(a, b, T - c < 64 ? T - c : 64, lane, s1, s2, m);
        if (c + lane < T) dec[c + lane] = w;
    }
    // the best final state: largest metric, lowest index among equals
    int bm = m, bs = lane;
    for (int off = 32; off >= 1; off >>= 1) {
        const int om = __shfl_xor(bm, off, 64), os = __shfl_xor(bs, off, 64);
        if (om > bm || (om == bm && os < bs)) { bm = om; bs = os; }
    }
    __syncthreads();
    int st = __builtin_amdgcn_readfirstlane(bs);
    for (int c = ((T - 1) >> 6) << 6; c >= 0; c -= 64) {
        const unsigned long long w = c + lane < T ? dec[c + lane] : 0ull;
        st = dd_k7_traceback(w, T - c < 64 ? T - c : 64, warm - c, warm + DD_LRPT_BLOCK - c, st, lane, ob);
        if (c < warm) break;
    }
    __syncthreads();
    uint32_t byte = 0;
    for (int q = 0; q < 8; ++q) byte = (byte << 1) | ob[8 * lane + q];
    bits[(int64_t)blockIdx.y * (nbits / 8) + (int64_t)blockIdx.x * (DD_LRPT_BLOCK / 8) + lane] = (uint8_t)byte;
}

// One workgroup per frame: fr = the frame's 1024 Viterbi bytes v, decoded from symbol p under h.  The frame's bytes fb are v itself
// or, for a differential stream (NRZM, section 4.18), d[i] = v[i] ^ v[i-1] with bit 0 of the frame set to 0: its neighbour lies in
// another decode span, so the marker is then compared over bits 1..31.  The re-encode count is taken from v, everything else from fb.
template <bool NRZM>
__global__ void __launch_bounds__(256) k_lrpt_finish(const uint8_t* __restrict__ bits, const char2* __restrict__ soft,
                                                      const int64_t* __restrict__ spans, uint8_t* __restrict__ bodies,
                                                      int* __restrict__ info) {
    __shared__ uint8_t fr[DD_LRPT_FRAME / 8];
    __shared__ int diff;
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x;
    const int64_t p = spans[2 * f];
    const int h = (int)spans[2 * f + 1];
    for (int i = tid; i < DD_LRPT_FRAME / 8; i += 256) fr[i] = bits[f * (DD_LRPT_FRAME / 8) + i];
    if (tid == 0) diff = 0;
    __syncthreads();
    const uint8_t* fb = fr;
    if constexpr (NRZM) {
        __shared__ uint8_t dd[DD_LRPT_FRAME / 8];
        for (int i = tid; i < DD_LRPT_FRAME / 8; i += 256) {
            const uint32_t v = fr[i];
            const uint32_t before = i ? (uint32_t)(fr[i - 1] & 1) << 7 : (v & 0x80u);      // v[8i - 1]; for i = 0 the bit itself: d[0] = 0
            dd[i] = (uint8_t)(v ^ ((v >> 1) | before));
        }
        fb = dd;
    }
    // step t: r = the decoded bits t-6 .. t, bit t in r's bit 6 (the encoder state from the decoded bits themselves)
    int mine = 0;
    for (int t = 6 + tid; t < DD_LRPT_FRAME; t += 256) {
        int r = 0;
        for (int j = 0; j < 7; ++j) {
            const int u = t - 6 + j;
            r |= ((fr[u >> 3] >> (7 - (u & 7))) & 1) << j;
        }
        const char2 s = soft[p + t];
        int a, b;
        dd_lrpt_hyp(s.x, s.y, h, a, b);
        mine += dd_k7_mismatch(r, a, b);
    }
    atomicAdd(&diff, mine);
    __syncthreads();
    for (int i = tid; i < DD_LRPT_BODY; i += 256) bodies[f * DD_LRPT_BODY + i] = fb[4 + i] ^ dd_pn.b[i % 255];
    if (tid == 0) {
        const uint32_t head = ((uint32_t)fb[0] << 24) | ((uint32_t)fb[1] << 16) | ((uint32_t)fb[2] << 8) | fb[3];
        info[3 * f] = __popc((head ^ DD_LRPT_ASM) & (NRZM ? 0x7FFFFFFFu : 0xFFFFFFFFu));
        info[3 * f + 1] = diff;
        info[3 * f + 2] = (fb[5] ^ dd_pn.b[1]) & 0x3F;            // the virtual channel id: the body's second byte, low six bits
    }
}

// spans_host = nspans (p, h) pairs: 0 <= h < 8 and [p, p + nbits) inside the symbols
static int dd_lrpt_check_spans(const int64_t* spans_host, int64_t nspans, int64_t nbits, int64_t nsym, const char* who) {
    for (int64_t i = 0; i < nspans; ++i) {
        const int64_t p = spans_host[2 * i], h = spans_host[2 * i + 1];
        DD_SYM_REQUIRE(h >= 0 && h < 8, who, "hypothesis outside 0..7");
        DD_SYM_REQUIRE(p >= 0 && p <= nsym - nbits, who, "span outside the symbols");
    }
    return DD_OK;
}

extern "C" int dd_lrpt_soft(const void* sym, int64_t nsym, int8_t* soft, void* stream) {
    DD_REQUIRE(nsym >= 0, "dd_lrpt_soft: sizes");
    if (nsym == 0) return DD_OK;
    DD_REQUIRE(sym != nullptr && soft != nullptr, "dd_lrpt_soft: null buffer");
    hipLaunchKernelGGL(k_lrpt_soft, dim3((unsigned)((nsym + 255) / 256)), dim3(256), 0, dd_stream(stream), (const double2*)sym, nsym,
                       (char2*)soft);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

// dd_lrpt_asm_search and dd_lrpt_asm_search_t: encoded = 32 symbols of code bits, first code bit in bit 63
static int dd_lrpt_asm_run(const char* who, const int8_t* soft, int64_t nsym, unsigned long long encoded, int min_score, int64_t cap,
                           int64_t* cand, unsigned long long* count, void* stream) {
    DD_SYM_REQUIRE(nsym >= 0 && cap >= 0 && count != nullptr, who, "sizes");
    DD_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned long long), dd_stream(stream)));
    if (nsym < 32) return DD_OK;
    DD_SYM_REQUIRE(soft != nullptr && (cap == 0 || cand != nullptr), who, "null buffer");
    uint32_t ei = 0, eq = 0;
    for (int k = 0; k < 32; ++k) {
        ei = (ei << 1) | (uint32_t)((encoded >> (63 - 2 * k)) & 1);
        eq = (eq << 1) | (uint32_t)((encoded >> (62 - 2 * k)) & 1);
    }
    hipLaunchKernelGGL(k_lrpt_asm_t, dim3((unsigned)((nsym - 31 + 255) / 256)), dim3(256), 0, dd_stream(stream), (const char2*)soft, nsym,
                       ei, eq, min_score, cap, cand, count);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_lrpt_asm_search(const int8_t* soft, int64_t nsym, int min_score, int64_t cap, int64_t* cand,
                                  unsigned long long* count, void* stream) {
    return dd_lrpt_asm_run("dd_lrpt_asm_search", soft, nsym, DD_LRPT_ASM_CODE, min_score, cap, cand, count, stream);
}

extern "C" int dd_lrpt_viterbi(const int8_t* soft, int64_t nsym, const int64_t* spans_host, int64_t nspans, int64_t nbits,
                               uint8_t* bits_packed, void* stream) {
    DD_REQUIRE(nsym >= 0 && nspans >= 0 && nspans <= 65535, "dd_lrpt_viterbi: sizes");
    DD_REQUIRE(nbits > 0 && nbits % DD_LRPT_BLOCK == 0 && nbits / DD_LRPT_BLOCK <= 0x7fffffff, "dd_lrpt_viterbi: nbits must be a multiple of 512");
    if (nspans == 0) return DD_OK;
    DD_REQUIRE(soft != nullptr && spans_host != nullptr && bits_packed != nullptr, "dd_lrpt_viterbi: null buffer");
    const int rc = dd_lrpt_check_spans(spans_host, nspans, nbits, nsym, "dd_lrpt_viterbi");
    if (rc != DD_OK) return rc;
    return dd_with_spans(spans_host, nspans, "dd_lrpt_viterbi", stream, [&](const int64_t* d) {
        hipLaunchKernelGGL(k_lrpt_viterbi, dim3((unsigned)(nbits / DD_LRPT_BLOCK), (unsigned)nspans), dim3(64), 0, dd_stream(stream),
                           (const char2*)soft, nsym, d, nbits, bits_packed);
    });
}

// dd_lrpt_finish and dd_lrpt_finish_nrzm
static int dd_lrpt_finish_run(const char* who, bool nrzm, const uint8_t* bits_packed, const int8_t* soft, int64_t nsym,
                              const int64_t* spans_host, int64_t nspans, uint8_t* bodies, int32_t* info, void* stream) {
    DD_SYM_REQUIRE(nsym >= 0 && nspans >= 0 && nspans <= 0x7fffffff, who, "sizes");
    if (nspans == 0) return DD_OK;
    DD_SYM_REQUIRE(bits_packed != nullptr && soft != nullptr && spans_host != nullptr && bodies != nullptr && info != nullptr, who,
                   "null buffer");
    const int rc = dd_lrpt_check_spans(spans_host, nspans, DD_LRPT_FRAME, nsym, who);
    if (rc != DD_OK) return rc;
    return dd_with_spans(spans_host, nspans, who, stream, [&](const int64_t* d) {
        hipLaunchKernelGGL(nrzm ? k_lrpt_finish<true> : k_lrpt_finish<false>, dim3((unsigned)nspans), dim3(256), 0, dd_stream(stream),
                           bits_packed, (const char2*)soft, d, bodies, info);
    });
}

extern "C" int dd_lrpt_finish(const uint8_t* bits_packed, const int8_t* soft, int64_t nsym, const int64_t* spans_host, int64_t nspans,
                              uint8_t* bodies, int32_t* info, void* stream) {
    return dd_lrpt_finish_run("dd_lrpt_finish", false, bits_packed, soft, nsym, spans_host, nspans, bodies, info, stream);
}
