// ACARS on VHF, 2400 baud MSK on 1200 / 2400 Hz over AM (beyond the reference; DESIGN.md section 4.25 defines every stage, acars.py
// restates each kernel in NumPy), included by dd_afsk.hip after dd_candidates.h, whose LDS prefix sum, tail, list kernel and driver it
// uses; the quantiser's scale and clip and the bit-end positions are its own.  The audio is the float64 AM envelope; everything
// behind the quantiser is integer, so sums in any order equal the restatement bit for bit.  The boundaries are float64 products and sums rounded one by one
// (the unit is built without contraction).
//
//   k_acars_sync      -- a workgroup stages the quantised audio of 256 starts and the reach of 32 bits in LDS and turns it into its
//                        exclusive prefix sum in place (dd_stage_prefix256; 32-bit wrap-around: |v| <= 2^27, so differences are
//                        exact); one thread per start decides the 32 bits of * SYN SYN SOH, each the sum of the w samples behind a
//                        bit's end less the w before it, three LDS reads per bit; a mask byte per sample, a count per workgroup
//   k_cand_list       -- (dd_candidates.h) the masks' pass bits as an ordered candidate list below the capacity
//   k_acars_block     -- one wave per listed start: 1920 bits by thirty ballots, each ballot word eight received characters; the end
//                        by a lane per character, the block check as a wave XOR of lone-bit registers, repair of one bit or of one
//                        bit in each of two characters guided by the characters' parity
#pragma once

#define DD_ACARS_TILE 256             // starts per workgroup (mirrored by acars.TILE)
#define DD_ACARS_W_MAX 32             // samples summed on either side of a bit's end at most
#define DD_ACARS_SLACK_MAX 5          // the template slid over a block's own pre-key is 6 or more places from itself and its inverse
#define DD_ACARS_CHARS 240            // characters demodulated behind SOH
#define DD_ACARS_BITS 1920
#define DD_ACARS_WORDS 30             // ballots: 64 bits, eight characters each
#define DD_ACARS_FIRST_END 12         // mode, address, ack, label and block id come before the first place ETX / ETB can take
#define DD_ACARS_TEMPLATE 0x54686880u // * SYN SYN SOH, each character lowest bit first, the first-sent bit in bit 31
#define DD_ACARS_SPAN 2372            // prefix entries of a tile at most: 258 + floor(32 * 64) + 2 * 32 = 2370
#define DD_ACARS_SCALE 4096.0
#define DD_ACARS_CLIP 2097152.0       // |q| <= 2^21: a u8 recording's envelope is below 2^20; beyond it and for a NaN q = 0
#define DD_ACARS_META 8

enum { DD_ACARS_OK = 0, DD_ACARS_OUTSIDE = 1, DD_ACARS_NO_END = 2, DD_ACARS_BAD_BCS = 3 };

struct DDAcarsGrid {
    double sps;                       // samples per bit
    int w, slack, fix;                // samples summed on either side; template places that may differ; bits a block may have repaired
    int span;                         // prefix entries of a tile: 258 + floor(32 sps) + 2 w
    int64_t nstart;                   // starts whose template ends inside the audio
};

struct DDAcarsTable {
    uint16_t z[DD_ACARS_BITS];        // the CRC register m zero bits after a lone one bit entered an empty register
};

constexpr DDAcarsTable dd_acars_make_table() {
    DDAcarsTable t{};
    unsigned v = 0x8408u;
    for (int m = 0; m < DD_ACARS_BITS; ++m) {
        t.z[m] = (uint16_t)v;
        v = (v & 1u) ? ((v >> 1) ^ 0x8408u) : (v >> 1);
    }
    return t;
}

__constant__ const DDAcarsTable dd_acars_table = dd_acars_make_table();

__device__ __forceinline__ int dd_acars_q(double x) {
    const double r = rint(x * DD_ACARS_SCALE);
    return (r >= -DD_ACARS_CLIP && r <= DD_ACARS_CLIP) ? (int)r : 0;
}

// the sample at which bit k of the start t ends
__device__ __forceinline__ int64_t dd_acars_end(int64_t t, int k, double sps) {
    return (int64_t)floor((double)t + ((double)k + 1.0) * sps);
}

__global__ void __launch_bounds__(DD_ACARS_TILE) k_acars_sync(const double* __restrict__ x, int64_t n, const DDAcarsGrid gd,
                                                              uint8_t* __restrict__ mask, int* __restrict__ bsum) {
    __shared__ uint32_t ps[DD_ACARS_SPAN];           // first q, then ps[j] = the sum of q over samples first .. first + j - 1 (mod 2^32)
    __shared__ int sh[256];
    __shared__ uint32_t tops[4];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * DD_ACARS_TILE;
    const int64_t first = base - gd.w;               // the tile's first sample; 0 outside the audio
    dd_stage_prefix256([&](int64_t i) { return dd_acars_q(x[i]); }, n, first, gd.span, ps, tops);
    const int64_t t = base + tid;
    uint32_t m = 0;
    if (t < gd.nstart) {
        uint32_t d = 0;                                                   // bit 31 - k = decision k: the first-sent bit in bit 31
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            // floor(sps) + w <= at <= 256 + floor(32 sps) + w (a rounding of the sum included): at - w >= 8, at + w <= span - 2
            const int at = (int)(dd_acars_end(t, k, gd.sps) - first);
            const int v = (int)(ps[at + gd.w] - 2u * ps[at] + ps[at - gd.w]);
            d |= v > 0 ? 0x80000000u >> k : 0u;
        }
        const int mis = __popc(d ^ DD_ACARS_TEMPLATE);
        m = mis <= gd.slack ? 1u : (32 - mis <= gd.slack ? 3u : 0u);
    }
    dd_cand_tail(mask, t, n, m, (int)(m & 1u), sh, bsum);
}

// the bytes of word j that lie at or before byte e, as a mask over the word's 64 bits
__device__ __forceinline__ unsigned long long dd_acars_upto(int j, int e) {
    const int nb = e + 1 - 8 * j;
    return nb >= 8 ? ~0ull : (nb <= 0 ? 0ull : (1ull << (8 * nb)) - 1ull);
}

// bytes[240 c]: the characters behind SOH in the polarity found, the first-sent bit in bit 0, repaired where the block is accepted;
// meta[8 c] = status, polarity, the template's wrong places, e (-1: no end), parity-flagged characters among 0 .. e, bits repaired,
// whether character e + 3 is DEL, the block check register over 0 .. e + 2 as received; score[c].  A start outside the audio gives
// DD_ACARS_OUTSIDE and zeros.
__global__ void __launch_bounds__(64) k_acars_block(const double* __restrict__ x, int64_t n, const DDAcarsGrid gd,
                                                    const int64_t* __restrict__ list, uint8_t* __restrict__ bytes,
                                                    int* __restrict__ meta, int64_t* __restrict__ score) {
    __shared__ unsigned long long rw[DD_ACARS_WORDS];                    // the received bits: bit 64 j + l is bit l of rw[j]
    __shared__ unsigned long long fw[DD_ACARS_WORDS];                    // bit 8 b of fw[j]: character 8 j + b has an even number of ones
    const int lane = threadIdx.x;
    const int64_t t = list[blockIdx.x];
    uint32_t* out = (uint32_t*)(bytes + (int64_t)blockIdx.x * DD_ACARS_CHARS);
    int* mt = meta + (int64_t)blockIdx.x * DD_ACARS_META;
    if (t < 0 || t >= n) {                                               // (uniform over the wave)
        if (lane < DD_ACARS_CHARS / 4) out[lane] = 0u;
        if (lane < DD_ACARS_META) mt[lane] = lane == 0 ? DD_ACARS_OUTSIDE : (lane == 3 ? -1 : 0);
        if (lane == 0) score[blockIdx.x] = 0;
        return;
    }
    const auto value = [&](int k) {
        const int64_t at = dd_acars_end(t, k, gd.sps);
        int s = 0;
        for (int j = 0; j < gd.w; ++j) {
            const int64_t a = at + j, b = at - 1 - j;
            if (a >= 0 && a < n) s += dd_acars_q(x[a]);
            if (b >= 0 && b < n) s -= dd_acars_q(x[b]);
        }
        return s;
    };
    // the template (lanes 0 .. 31): its wrong places, the polarity, the score
    const int v0 = lane < 32 ? value(lane) : 0;
    const uint32_t d = __brev((uint32_t)__ballot(lane < 32 && v0 > 0));
    const int far = __popc(d ^ DD_ACARS_TEMPLATE);
    const bool inv = far > 16;
    const int mis = inv ? 32 - far : far;
    int64_t sc = v0 < 0 ? -(int64_t)v0 : (int64_t)v0;
    for (int o = 32; o > 0; o >>= 1) sc += __shfl_xor(sc, o);
    // thirty ballots: a ballot word is eight received characters in order
    for (int j = 0; j < DD_ACARS_WORDS; ++j) {
        const unsigned long long up = __ballot(value(32 + 64 * j + lane) > 0);
        const unsigned long long r = inv ? ~up : up;
        unsigned long long f = r ^ (r >> 4);
        f ^= f >> 2;
        f ^= f >> 1;
        if (lane == 0) {
            rw[j] = r;
            fw[j] = ~f & 0x0101010101010101ull;
        }
    }
    __syncthreads();
    uint8_t* by = (uint8_t*)rw;
    // e: the least character from 12 on that holds ETX or ETB with the block check's two behind it inside the 240
    int e = -1;
    for (int r = 3; r >= 0; --r) {
        const int i = 64 * r + lane;
        const bool hit = i >= DD_ACARS_FIRST_END && i + 2 < DD_ACARS_CHARS && (by[i] == 0x83 || by[i] == 0x97);
        const unsigned long long hits = __ballot(hit);
        if (hits) e = 64 * r + __ffsll((long long)hits) - 1;
    }
    int status = DD_ACARS_NO_END, c = 0, fixed = 0, del = 0;
    uint32_t s = 0;
    if (e >= 0) {                                                        // (uniform over the wave)
        const int N = 8 * (e + 3);
        // the register over characters 0 .. e + 2: the XOR of the lone-bit registers of the one bits
        for (int j = 0; j < DD_ACARS_WORDS; ++j) {
            const int p = 64 * j + lane;
            if (p < N && ((rw[j] >> lane) & 1ull)) s ^= dd_acars_table.z[N - 1 - p];
        }
        for (int o = 32; o > 0; o >>= 1) s ^= __shfl_xor(s, o);
        // the parity-flagged characters among 0 .. e: how many, and the first two
        const unsigned long long mine = lane < DD_ACARS_WORDS ? fw[lane] & dd_acars_upto(lane, e) : 0ull;
        c = __popcll(mine);
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        unsigned long long has = __ballot(mine != 0ull);
        int f1 = 0, f2 = 0;
        if (c == 1 || c == 2) {
            const int j1 = __ffsll((long long)has) - 1;
            unsigned long long m1 = fw[j1] & dd_acars_upto(j1, e);
            f1 = 8 * j1 + ((__ffsll((long long)m1) - 1) >> 3);
            m1 &= m1 - 1ull;
            if (c == 2) {
                if (!m1) {
                    has &= has - 1ull;
                    const int j2 = __ffsll((long long)has) - 1;
                    f2 = 8 * j2 + ((__ffsll((long long)(fw[j2] & dd_acars_upto(j2, e))) - 1) >> 3);
                } else f2 = 8 * j1 + ((__ffsll((long long)m1) - 1) >> 3);
            }
        }
        status = DD_ACARS_BAD_BCS;
        int p1 = -1, p2 = -1;                                            // the bits to flip
        if (s == 0u) status = DD_ACARS_OK;
        else if (gd.fix >= 1 && c <= 1) {
            // one flagged character: lanes 0 .. 7 its bits; none: lanes 0 .. 15 the block check's
            const int p = (c ? 8 * f1 : 8 * (e + 1)) + lane;
            const unsigned long long hits = __ballot(lane < (c ? 8 : 16) && dd_acars_table.z[N - 1 - (p < N ? p : N - 1)] == s);
            if (hits) {                                                  // (the registers of distinct bits differ: one hit at most)
                p1 = p - lane + __ffsll((long long)hits) - 1;
                fixed = 1;
            }
        } else if (gd.fix >= 2 && c == 2) {
            // lane 8 i + j tests bit i of the first flagged character with bit j of the second
            const uint32_t za = dd_acars_table.z[N - 1 - (8 * f1 + (lane >> 3))], zb = dd_acars_table.z[N - 1 - (8 * f2 + (lane & 7))];
            const unsigned long long hits = __ballot((za ^ zb) == s);
            if (__popcll(hits) == 1) {
                const int l = __ffsll((long long)hits) - 1;
                p1 = 8 * f1 + (l >> 3);
                p2 = 8 * f2 + (l & 7);
                fixed = 2;
            }
        }
        if (fixed) status = DD_ACARS_OK;
        del = e + 3 < DD_ACARS_CHARS && by[e + 3] == 0x7F;
        __syncthreads();                                                 // (every lane has read the characters as received)
        if (lane == 0 && p1 >= 0) by[p1 >> 3] ^= (uint8_t)(1u << (p1 & 7));
        if (lane == 0 && p2 >= 0) by[p2 >> 3] ^= (uint8_t)(1u << (p2 & 7));
        __syncthreads();
    }
    if (lane < DD_ACARS_CHARS / 4) out[lane] = ((const uint32_t*)rw)[lane];
    if (lane == 0) {
        mt[0] = status;
        mt[1] = inv ? 1 : 0;
        mt[2] = mis;
        mt[3] = e;
        mt[4] = c;
        mt[5] = fixed;
        mt[6] = del;
        mt[7] = (int)s;
        score[blockIdx.x] = sc;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the C entries
// 0 when a size, the samples per bit, the window, the slack or the repair limit is not served, else 1 with the grid filled
static int dd_acars_grid(int64_t n, double sps, int w, int slack, int fix, DDAcarsGrid* gd) {
    if (n < 0 || n > 0x7FFFFFF0LL || !(sps >= 8.0 && sps <= 64.0) || w < 1 || w > DD_ACARS_W_MAX || slack < 0 ||
        slack > DD_ACARS_SLACK_MAX || fix < 0 || fix > 2)
        return 0;
    gd->sps = sps;
    gd->w = w;
    gd->slack = slack;
    gd->fix = fix;
    const int64_t reach = (int64_t)floor(32.0 * sps) + w;               // samples from a start to past its template's last
    gd->span = (int)(DD_ACARS_TILE + 2 + reach + w);
    gd->nstart = n >= reach ? n - reach + 1 : 0;
    return 1;
}

static auto dd_acars_sync_launch(const double* audio, int64_t n, const DDAcarsGrid& gd, hipStream_t s) {
    return [=](uint8_t* mask, int* bsum, int64_t nb) {
        hipLaunchKernelGGL(k_acars_sync, dim3((unsigned)nb), dim3(DD_ACARS_TILE), 0, s, audio, n, gd, mask, bsum);
    };
}

extern "C" int dd_acars_candidates(const double* audio, int64_t n, double sps, int w, int slack, int64_t* list, int64_t cap,
                                   int64_t* count_host, void* stream) {
    DDAcarsGrid gd = {};
    const bool served = cap >= 0 && dd_acars_grid(n, sps, w, slack, 0, &gd);
    hipStream_t s = dd_stream(stream);
    return dd_cand_entry("dd_acars_candidates", served,
                         "dd_acars_candidates: need 0 <= n < 2^31, 8 <= sps <= 64, 1 <= w <= 32, 0 <= slack <= 5 and cap >= 0", audio, n,
                         gd.nstart, 1, 1u, list, cap, count_host, s, dd_acars_sync_launch(audio, n, gd, s));
}

extern "C" int dd_acars_blocks(const double* audio, int64_t n, double sps, int w, int fix, const int64_t* list, int64_t m,
                               uint8_t* bytes, int32_t* meta, int64_t* score, void* stream) {
    DDAcarsGrid gd;
    DD_REQUIRE(m >= 0 && m <= 0x7FFFFFFFLL && dd_acars_grid(n, sps, w, 0, fix, &gd),
               "dd_acars_blocks: need 0 <= n < 2^31, 8 <= sps <= 64, 1 <= w <= 32, fix of 0, 1 or 2 and 0 <= m < 2^31");
    if (n == 0 || m == 0) return DD_OK;
    DD_REQUIRE(audio != nullptr && list != nullptr && bytes != nullptr && meta != nullptr && score != nullptr,
               "dd_acars_blocks: null buffer");
    hipLaunchKernelGGL(k_acars_block, dim3((unsigned)m), dim3(64), 0, dd_stream(stream), audio, n, gd, list, bytes, meta, score);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_debug_acars_masks(const double* audio, int64_t n, double sps, int w, int slack, uint8_t* mask, void* stream) {
    DDAcarsGrid gd = {};
    const bool served = dd_acars_grid(n, sps, w, slack, 0, &gd);
    hipStream_t s = dd_stream(stream);
    return dd_cand_masks_entry("dd_debug_acars_masks", served,
                               "dd_debug_acars_masks: need 0 <= n < 2^31, 8 <= sps <= 64, 1 <= w <= 32 and 0 <= slack <= 5", audio, n, gd.nstart,
                               mask, s, dd_acars_sync_launch(audio, n, gd, s));
}
