// Meteor-M2 LRPT channel decoding (beyond the reference; DESIGN.md section 4.14 defines every stage bit for bit, lrpt.py restates
// it in NumPy), included by dd_afsk.hip after dd_meteor.h.  All arithmetic is integer.
//
//   k_lrpt_soft     -- lim(re / 2), lim(im / 2) of each corrected symbol as an int8 pair
//   k_lrpt_asm      -- the encoded sync marker's 52 scored bits against the hard bits at every symbol, under the eight phase /
//                      IQ-swap hypotheses; (position, hypothesis, score) of every score >= min_score is a candidate
//   k_lrpt_viterbi  -- rate 1/2, K = 7 soft-decision decode: one wave per block of 512 trellis steps, lane = state
//   k_lrpt_finish   -- per frame: marker bits in error, bytes 4..1023 XOR the CCSDS pseudo-noise sequence, and how many hard input
//                      bits differ from the re-encoded decoded bits
#pragma once

#define DD_LRPT_FRAME 8192            // trellis steps (= symbols = decoded bits) per channel frame
#define DD_LRPT_BODY 1020             // bytes after the 4-byte marker
#define DD_LRPT_BLOCK 512             // trellis steps decoded per wave
#define DD_LRPT_WARM 128              // steps of add-compare-select before a block (warm-up) and after it (tail)
#define DD_LRPT_STEPS (DD_LRPT_BLOCK + 2 * DD_LRPT_WARM)
#define DD_LRPT_G1 0x79
#define DD_LRPT_G2 0x5B
#define DD_LRPT_ASM 0x1ACFFC1Du
// encode(marker) from state 0, first code bit in bit 63, split into the (c1, c2) = (I, Q) halves of its 32 symbols, first symbol in
// bit 31; the first six symbols (12 code bits) depend on the previous frame's tail and are never scored
#define DD_LRPT_ASM_CODE 0x035D49C24FF2686Bull
#define DD_LRPT_SCORED 0x03FFFFFFu

struct DDLrptPn {
    uint8_t b[255];                   // the pseudo-noise sequence's first 255 bytes (its period: 255 bits)
};

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

// one position per thread; the workgroup's 256 + 31 symbols are staged as four sign bits each: a > 0, b > 0, a < 0, b < 0
__global__ void __launch_bounds__(256) k_lrpt_asm(const char2* __restrict__ soft, int64_t nsym, int min_score, int64_t cap,
                                                   int64_t* __restrict__ cand, unsigned long long* __restrict__ count) {
    __shared__ uint8_t sg[256 + 31];
    const int64_t p0 = (int64_t)blockIdx.x * 256;
    for (int i = threadIdx.x; i < 256 + 31; i += 256) {
        uint8_t v = 0;
        if (p0 + i < nsym) {
            const char2 s = soft[p0 + i];
            v = (uint8_t)((s.x > 0) | ((s.y > 0) << 1) | ((s.x < 0) << 2) | ((s.y < 0) << 3));
        }
        sg[i] = v;
    }
    __syncthreads();
    const int64_t p = p0 + threadIdx.x;
    if (p + 32 > nsym) return;
    uint32_t m[4] = {0, 0, 0, 0};             // per sign bit: the 32 symbols from p, the first in bit 31
    for (int k = 0; k < 32; ++k) {
        const uint32_t v = sg[threadIdx.x + k];
        for (int q = 0; q < 4; ++q) m[q] = (m[q] << 1) | ((v >> q) & 1);
    }
    uint32_t ei = 0, eq = 0;
    for (int k = 0; k < 32; ++k) {
        ei = (ei << 1) | (uint32_t)((DD_LRPT_ASM_CODE >> (63 - 2 * k)) & 1);
        eq = (eq << 1) | (uint32_t)((DD_LRPT_ASM_CODE >> (62 - 2 * k)) & 1);
    }
    for (int h = 0; h < 8; ++h) {
        // hard bits of (a, b), (-b, a), (-a, -b), (b, -a): (a > 0, b > 0), (b < 0, a > 0), (a < 0, b < 0), (b > 0, a < 0)
        const int r = h & 3;
        const uint32_t x = r == 0 ? m[0] : (r == 1 ? m[3] : (r == 2 ? m[2] : m[1]));
        const uint32_t y = r == 0 ? m[1] : (r == 1 ? m[0] : (r == 2 ? m[3] : m[2]));
        const uint32_t hi = (h & 4) ? y : x, hq = (h & 4) ? x : y;
        const int score = __popc(~(hi ^ ei) & DD_LRPT_SCORED) + __popc(~(hq ^ eq) & DD_LRPT_SCORED);
        if (score >= min_score) {
            const unsigned long long c = atomicAdd(count, 1ull);
            if ((int64_t)c < cap) {
                cand[3 * c] = p;
                cand[3 * c + 1] = h;
                cand[3 * c + 2] = score;
            }
        }
    }
}

// Block blockIdx.x of span blockIdx.y: add-compare-select over the steps lo = max(0, k - 128) .. hi = min(nsym, e + 128) of the
// block's steps [k, e), all metrics 0 at lo; lane ns is state ns, its predecessors ((ns & 31) << 1) | x come by cross-lane reads,
// x = 1 survives only when strictly larger.  The 64 decisions of a step are one ballot word; the words of 64 steps sit one per
// lane until they go to LDS together.  Traceback from the largest final metric (lowest state among equals) reads them back the
// same way, 64 steps per LDS read, and the 512 bits of [k, e) leave packed MSB first.  Metrics stay below 768 * 256: int32.
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
    const int pred0 = (lane & 31) << 1;
    int s1[2], s2[2];                                                 // 2 c - 1 of the branches from the two predecessors
    for (int x = 0; x < 2; ++x) {
        const int r = ((lane >> 5) << 6) | pred0 | x;
        s1[x] = 2 * (__popc(r & DD_LRPT_G1) & 1) - 1;
        s2[x] = 2 * (__popc(r & DD_LRPT_G2) & 1) - 1;
    }
    int m = 0;
    for (int c = 0; c < T; c += 64) {
        int a = 0, b = 0;
        if (c + lane < T) {
            const char2 s = soft[lo + c + lane];
            dd_lrpt_hyp(s.x, s.y, h, a, b);
        }
        unsigned long long w = 0;
        const int nj = T - c < 64 ? T - c : 64;
        for (int j = 0; j < nj; ++j) {
            const int aj = __builtin_amdgcn_readlane(a, j), bj = __builtin_amdgcn_readlane(b, j);
            const int c0 = __shfl(m, pred0, 64) + s1[0] * aj + s2[0] * bj;
            const int c1 = __shfl(m, pred0 | 1, 64) + s1[1] * aj + s2[1] * bj;
            const bool d = c1 > c0;
            const unsigned long long word = __ballot(d);
            m = d ? c1 : c0;
            if (lane == j) w = word;
        }
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
        const int wl = (int)(uint32_t)w, wh = (int)(uint32_t)(w >> 32);
        const int nj = T - c < 64 ? T - c : 64;
        for (int j = nj - 1; j >= 0; --j) {
            const int t = c + j;
            if (t < warm) break;
            const uint32_t half = (uint32_t)(st < 32 ? __builtin_amdgcn_readlane(wl, j) : __builtin_amdgcn_readlane(wh, j));
            if (t < warm + DD_LRPT_BLOCK && lane == 0) ob[t - warm] = (uint8_t)(st >> 5);
            st = ((st & 31) << 1) | (int)((half >> (st & 31)) & 1);
        }
        if (c < warm) break;
    }
    __syncthreads();
    uint32_t byte = 0;
    for (int q = 0; q < 8; ++q) byte = (byte << 1) | ob[8 * lane + q];
    bits[(int64_t)blockIdx.y * (nbits / 8) + (int64_t)blockIdx.x * (DD_LRPT_BLOCK / 8) + lane] = (uint8_t)byte;
}

// one workgroup per frame: bits = the frame's 1024 decoded bytes, decoded from symbol p under h
__global__ void __launch_bounds__(256) k_lrpt_finish(const uint8_t* __restrict__ bits, const char2* __restrict__ soft,
                                                      const int64_t* __restrict__ spans, const DDLrptPn pn, uint8_t* __restrict__ bodies,
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
    for (int i = tid; i < DD_LRPT_BODY; i += 256) bodies[f * DD_LRPT_BODY + i] = fr[4 + i] ^ pn.b[i % 255];
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
        mine += ((__popc(r & DD_LRPT_G1) & 1) != (a > 0)) + ((__popc(r & DD_LRPT_G2) & 1) != (b > 0));
    }
    atomicAdd(&diff, mine);
    __syncthreads();
    if (tid == 0) {
        const uint32_t head = ((uint32_t)fr[0] << 24) | ((uint32_t)fr[1] << 16) | ((uint32_t)fr[2] << 8) | fr[3];
        info[3 * f] = __popc(head ^ DD_LRPT_ASM);
        info[3 * f + 1] = diff;
        info[3 * f + 2] = (fr[5] ^ pn.b[1]) & 0x3F;               // the virtual channel id: the body's second byte, low six bits
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

// the (p, h) pairs go up to a device array of the call, launch(that array) enqueues the kernel, the stream is drained before it is freed
template <class Launch>
static int dd_lrpt_with_spans(const int64_t* spans_host, int64_t nspans, const char* who, void* stream, Launch launch) {
    DDDevBuf<int64_t> d;
    DD_HIP_CHECK(d.alloc((size_t)nspans * 2));
    int rc = DD_OK;
    if (hipMemcpyAsync(d, spans_host, d.bytes(), hipMemcpyHostToDevice, dd_stream(stream)) != hipSuccess) rc = DD_ERR_HIP;
    if (rc == DD_OK) {
        launch(d.get());
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(dd_stream(stream)) != hipSuccess) rc = DD_ERR_HIP;
    }
    DD_SYM_REQUIRE(rc == DD_OK, who, "launch failed");
    return DD_OK;
}

// the pseudo-noise sequence's period as bytes (host): register all ones, output r[0], feedback r[0] ^ r[3] ^ r[5] ^ r[7]
static DDLrptPn dd_lrpt_pn() {
    DDLrptPn pn;
    uint8_t r[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    memset(pn.b, 0, sizeof(pn.b));
    for (int i = 0; i < 255 * 8; ++i) {
        pn.b[i >> 3] |= (uint8_t)(r[0] << (7 - (i & 7)));
        const uint8_t fb = r[0] ^ r[3] ^ r[5] ^ r[7];
        for (int q = 0; q < 7; ++q) r[q] = r[q + 1];
        r[7] = fb;
    }
    return pn;
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

extern "C" int dd_lrpt_asm_search(const int8_t* soft, int64_t nsym, int min_score, int64_t cap, int64_t* cand,
                                  unsigned long long* count, void* stream) {
    DD_REQUIRE(nsym >= 0 && cap >= 0 && count != nullptr, "dd_lrpt_asm_search: sizes");
    DD_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(unsigned long long), dd_stream(stream)));
    if (nsym < 32) return DD_OK;
    DD_REQUIRE(soft != nullptr && (cap == 0 || cand != nullptr), "dd_lrpt_asm_search: null buffer");
    hipLaunchKernelGGL(k_lrpt_asm, dim3((unsigned)((nsym - 31 + 255) / 256)), dim3(256), 0, dd_stream(stream), (const char2*)soft, nsym,
                       min_score, cap, cand, count);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_lrpt_viterbi(const int8_t* soft, int64_t nsym, const int64_t* spans_host, int64_t nspans, int64_t nbits,
                               uint8_t* bits_packed, void* stream) {
    DD_REQUIRE(nsym >= 0 && nspans >= 0 && nspans <= 65535, "dd_lrpt_viterbi: sizes");
    DD_REQUIRE(nbits > 0 && nbits % DD_LRPT_BLOCK == 0 && nbits / DD_LRPT_BLOCK <= 0x7fffffff, "dd_lrpt_viterbi: nbits must be a multiple of 512");
    if (nspans == 0) return DD_OK;
    DD_REQUIRE(soft != nullptr && spans_host != nullptr && bits_packed != nullptr, "dd_lrpt_viterbi: null buffer");
    const int rc = dd_lrpt_check_spans(spans_host, nspans, nbits, nsym, "dd_lrpt_viterbi");
    if (rc != DD_OK) return rc;
    return dd_lrpt_with_spans(spans_host, nspans, "dd_lrpt_viterbi", stream, [&](const int64_t* d) {
        hipLaunchKernelGGL(k_lrpt_viterbi, dim3((unsigned)(nbits / DD_LRPT_BLOCK), (unsigned)nspans), dim3(64), 0, dd_stream(stream),
                           (const char2*)soft, nsym, d, nbits, bits_packed);
    });
}

extern "C" int dd_lrpt_finish(const uint8_t* bits_packed, const int8_t* soft, int64_t nsym, const int64_t* spans_host, int64_t nspans,
                              uint8_t* bodies, int32_t* info, void* stream) {
    DD_REQUIRE(nsym >= 0 && nspans >= 0 && nspans <= 0x7fffffff, "dd_lrpt_finish: sizes");
    if (nspans == 0) return DD_OK;
    DD_REQUIRE(bits_packed != nullptr && soft != nullptr && spans_host != nullptr && bodies != nullptr && info != nullptr,
               "dd_lrpt_finish: null buffer");
    const int rc = dd_lrpt_check_spans(spans_host, nspans, DD_LRPT_FRAME, nsym, "dd_lrpt_finish");
    if (rc != DD_OK) return rc;
    const DDLrptPn pn = dd_lrpt_pn();
    return dd_lrpt_with_spans(spans_host, nspans, "dd_lrpt_finish", stream, [&](const int64_t* d) {
        hipLaunchKernelGGL(k_lrpt_finish, dim3((unsigned)nspans), dim3(256), 0, dd_stream(stream), bits_packed, (const char2*)soft, d, pn,
                           bodies, info);
    });
}
