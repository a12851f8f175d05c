// POCSAG paging, 2-FSK at 512, 1200 or 2400 baud (beyond the reference; DESIGN.md section 4.24 defines every stage, pocsag.py restates
// each kernel in NumPy), included by dd_afsk.hip after dd_candidates.h, whose quantiser, positions, LDS prefix sum, tail, list kernel
// and driver it uses.  The audio is the FM discriminator's float64 output in radians per sample; everything behind the quantiser is
// integer, so sums in any order equal the restatement bit for bit.
//
//   k_pocsag_sync     -- a workgroup stages the quantised audio of 256 starts and the reach of 32 bits in LDS and turns it into its
//                        exclusive prefix sum in place (dd_stage_prefix256; 32-bit wrap-around: a window's sum is below 2^28, so differences are exact);
//                        one thread per start decides the 32 bits of the frame sync codeword against their own mean, two LDS reads
//                        per bit; a mask byte per sample, a count per workgroup
//   k_cand_list       -- (dd_candidates.h) the masks' pass bits as an ordered candidate list below the capacity
//   k_pocsag_batch    -- one wave per listed start: 544 bits by nine ballots, polarity from the sync codeword, BCH(31,21) + parity
//                        correction of up to two bits per codeword by a syndrome search across the lanes, two codewords per ballot
#pragma once

#define DD_POCSAG_TILE 256            // starts per workgroup (mirrored by pocsag.TILE)
#define DD_POCSAG_W_MAX 77            // samples summed per bit value at most: the odd number nearest 0.6 * 128
#define DD_POCSAG_SLACK_MAX 8         // the sync codeword slid into the preamble is 9 or more places from itself and its inverse
#define DD_POCSAG_WORDS 17            // codewords per batch, the sync codeword included
#define DD_POCSAG_BITS 544
#define DD_POCSAG_FSC 0x7CD215D8u     // the frame sync codeword, the first-sent bit in bit 31
#define DD_POCSAG_GEN 0x769u          // x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1 over bits 31 .. 1

enum { DD_POCSAG_OK = 0, DD_POCSAG_OUTSIDE = 1 };

struct DDPocsagGrid {
    double sps;                       // samples per bit
    int h, slack, fix;                // a bit value sums 2 h + 1 samples; sync places that may differ; errors a codeword may hold
    int span;                         // prefix entries of a tile: 257 + floor(31.5 sps) + 2 h + 1
    int64_t nstart;                   // starts whose sync codeword ends inside the audio
};

struct DDPocsagTable {
    uint16_t z[32];                   // z[p] = x^(p - 1) mod the generator: the syndrome of a lone error in bit p; z[0] = 0 (parity)
};

constexpr DDPocsagTable dd_pocsag_make_table() {
    DDPocsagTable t{};
    unsigned v = 1u;
    for (int p = 1; p < 32; ++p) {
        t.z[p] = (uint16_t)v;
        v <<= 1;
        if (v & 0x400u) v ^= DD_POCSAG_GEN;
    }
    return t;
}

__constant__ const DDPocsagTable dd_pocsag_table = dd_pocsag_make_table();

__global__ void __launch_bounds__(DD_POCSAG_TILE) k_pocsag_sync(const double* __restrict__ x, int64_t n, const DDPocsagGrid gd,
                                                                uint8_t* __restrict__ mask, int* __restrict__ bsum) {
    __shared__ uint32_t ps[DD_CAND_SPAN];            // first q, then ps[j] = the sum of q over samples first .. first + j - 1 (mod 2^32)
    __shared__ int sh[256];
    __shared__ uint32_t tops[4];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * DD_POCSAG_TILE;
    const int64_t first = base - gd.h;               // the tile's first sample; 0 outside the audio
    dd_stage_prefix256([&](int64_t i) { return dd_fm_q(x[i]); }, n, first, gd.span, ps, tops);
    const int64_t t = base + tid;
    uint32_t m = 0;
    if (t < gd.nstart) {
        int v[32];
        int64_t S = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            const int at = (int)(dd_bit_mid(t, k, gd.sps) - first);      // h <= at, at + h + 1 < span (a rounding of the sum included)
            v[k] = (int)(ps[at + gd.h + 1] - ps[at - gd.h]);
            S += v[k];
        }
        uint32_t d = 0;                                                   // bit 31 - k = decision k: the first-sent bit in bit 31
#pragma unroll
        for (int k = 0; k < 32; ++k) d |= (int64_t)32 * v[k] > S ? 0x80000000u >> k : 0u;
        const int mis = __popc(~d ^ DD_POCSAG_FSC);                      // a level above the mean is a 0
        m = mis <= gd.slack ? 1u : (32 - mis <= gd.slack ? 3u : 0u);
    }
    dd_cand_tail(mask, t, n, m, (int)(m & 1u), sh, bsum);
}

// words[17 c]: the batch's codewords in the polarity found, the first-sent bit in bit 31; codeword 0 as received, 1 .. 16 corrected
// where accepted and as received where not; errs[17 c]: errs[0] = the sync codeword's wrong places, else the bits repaired, 255 =
// uncorrectable; meta[4 c] = status, polarity, accepted codewords of the 16, errs[0]; score[c].  A start outside the audio gives
// DD_POCSAG_OUTSIDE and zeros.
__global__ void __launch_bounds__(64) k_pocsag_batch(const double* __restrict__ x, int64_t n, const DDPocsagGrid gd,
                                                     const int64_t* __restrict__ list, uint32_t* __restrict__ words,
                                                     uint8_t* __restrict__ errs, int* __restrict__ meta, int64_t* __restrict__ score) {
    const int lane = threadIdx.x;
    const int64_t t = list[blockIdx.x];
    uint32_t* wo = words + (int64_t)blockIdx.x * DD_POCSAG_WORDS;
    uint8_t* eo = errs + (int64_t)blockIdx.x * DD_POCSAG_WORDS;
    int* mt = meta + (int64_t)blockIdx.x * 4;
    if (t < 0 || t >= n) {                                               // (uniform over the wave)
        if (lane < DD_POCSAG_WORDS) {
            wo[lane] = 0u;
            eo[lane] = 0;
        }
        if (lane == 0) {
            mt[0] = DD_POCSAG_OUTSIDE;
            mt[1] = mt[2] = mt[3] = 0;
            score[blockIdx.x] = 0;
        }
        return;
    }
    const auto value = [&](int k) { return dd_window_sum(x, n, dd_bit_mid(t, k, gd.sps), gd.h); };
    // the sync codeword (lanes 0 .. 31): S, the polarity, the score
    const int v0 = value(lane);
    int64_t S = lane < 32 ? v0 : 0;
    for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
    unsigned long long up = __ballot((int64_t)32 * v0 > S);
    const int far = __popc(~__brev((uint32_t)up) ^ DD_POCSAG_FSC);
    const bool inv = far > 16;
    const int mis = inv ? 32 - far : far;
    const int64_t dv = (int64_t)32 * v0 - S;
    int64_t sc = lane < 32 ? (dv < 0 ? -dv : dv) : 0;
    for (int o = 32; o > 0; o >>= 1) sc += __shfl_xor(sc, o);
    // bit 64 j + lane of the batch is lane `lane` of ballot j: lane l of a half holds bit 31 - l of codeword 2 j + half
    const int p = 31 - (lane & 31);
    const uint32_t zl = dd_pocsag_table.z[p];
    int good = 0;
    for (int j = 0; j < 9; ++j) {
        const int b = 64 * j + lane;
        if (j > 0) up = __ballot(b < DD_POCSAG_BITS && (int64_t)32 * value(b) > S);
        const unsigned long long rx = inv ? up : ~up;                    // the received bits in the polarity found
        // the syndrome of each half: the XOR of the lone-bit remainders of its one bits
        uint32_t syn = ((rx >> lane) & 1ull) ? zl : 0u;
        for (int o = 16; o > 0; o >>= 1) syn ^= __shfl_xor(syn, o);
        const bool one = syn != 0u && zl == syn;
        bool two = false;                                                // is there another bit whose remainder completes mine to syn?
        if (syn != 0u && p > 0) {
            const uint32_t want = syn ^ zl;
            for (int q = 1; q < 32; ++q) two |= dd_pocsag_table.z[q] == want;
        }
        const unsigned long long oneb = __ballot(one), twob = __ballot(two);
        for (int half = 0; half < 2; ++half) {
            const int cw = 2 * j + half;
            if (cw >= DD_POCSAG_WORDS) break;
            const uint32_t got = __brev((uint32_t)(rx >> (32 * half)));
            if (cw == 0) {
                if (lane == 0) {
                    wo[0] = got;
                    eo[0] = (uint8_t)mis;
                }
                continue;
            }
            const uint32_t sy = (uint32_t)__shfl((int)syn, 32 * half);
            const uint32_t f1 = __brev((uint32_t)(oneb >> (32 * half))), f2 = __brev((uint32_t)(twob >> (32 * half)));
            uint32_t fixed = got;
            int ne = 0;
            bool ok = true;
            if (sy != 0u) {
                if (f1) {
                    fixed ^= f1;
                    ne = 1;
                } else if (__popc(f2) == 2) {
                    fixed ^= f2;
                    ne = 2;
                } else ok = false;
            }
            if (ok && (__popc(fixed) & 1)) {                             // the parity bit: one more error
                fixed ^= 1u;
                ++ne;
            }
            ok = ok && ne <= gd.fix;
            good += ok ? 1 : 0;
            if (lane == 0) {
                wo[cw] = ok ? fixed : got;
                eo[cw] = (uint8_t)(ok ? ne : 255);
            }
        }
    }
    if (lane == 0) {
        mt[0] = DD_POCSAG_OK;
        mt[1] = inv ? 1 : 0;
        mt[2] = good;
        mt[3] = mis;
        score[blockIdx.x] = sc;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the C entries
// 0 when a size, the samples per bit, the window, the slack or the error limit is not served, else 1 with the grid filled
static int dd_pocsag_grid(int64_t n, double sps, int w, int slack, int fix, DDPocsagGrid* gd) {
    if (n < 0 || n > 0x7FFFFFF0LL || !(sps >= 4.0 && sps <= 128.0) || w < 1 || w > DD_POCSAG_W_MAX || !(w & 1) || slack < 0 ||
        slack > DD_POCSAG_SLACK_MAX || fix < 0 || fix > 2)
        return 0;
    gd->sps = sps;
    gd->h = w / 2;
    gd->slack = slack;
    gd->fix = fix;
    const int64_t reach = (int64_t)floor(31.5 * sps) + gd->h + 1;       // samples from a start to past its sync codeword's last
    gd->span = (int)(DD_POCSAG_TILE + reach + gd->h + 1);
    gd->nstart = n >= reach ? n - reach + 1 : 0;
    return 1;
}

static auto dd_pocsag_sync_launch(const double* audio, int64_t n, const DDPocsagGrid& gd, hipStream_t s) {
    return [=](uint8_t* mask, int* bsum, int64_t nb) {
        hipLaunchKernelGGL(k_pocsag_sync, dim3((unsigned)nb), dim3(DD_POCSAG_TILE), 0, s, audio, n, gd, mask, bsum);
    };
}

extern "C" int dd_pocsag_candidates(const double* audio, int64_t n, double sps, int w, int slack, int64_t* list, int64_t cap,
                                    int64_t* count_host, void* stream) {
    DDPocsagGrid gd = {};
    const bool served = cap >= 0 && dd_pocsag_grid(n, sps, w, slack, 0, &gd);
    hipStream_t s = dd_stream(stream);
    return dd_cand_entry("dd_pocsag_candidates", served,
                         "dd_pocsag_candidates: need 0 <= n < 2^31, 4 <= sps <= 128, an odd w from 1 to 77, 0 <= slack <= 8 and cap >= 0", audio,
                         n, gd.nstart, 1, 1u, list, cap, count_host, s, dd_pocsag_sync_launch(audio, n, gd, s));
}

extern "C" int dd_pocsag_batches(const double* audio, int64_t n, double sps, int w, int fix, const int64_t* list, int64_t m,
                                 uint32_t* words, uint8_t* errs, int32_t* meta, int64_t* score, void* stream) {
    DDPocsagGrid gd;
    DD_REQUIRE(m >= 0 && m <= 0x7FFFFFFFLL && dd_pocsag_grid(n, sps, w, 0, fix, &gd),
               "dd_pocsag_batches: need 0 <= n < 2^31, 4 <= sps <= 128, an odd w from 1 to 77, fix of 0, 1 or 2 and 0 <= m < 2^31");
    if (n == 0 || m == 0) return DD_OK;
    DD_REQUIRE(audio != nullptr && list != nullptr && words != nullptr && errs != nullptr && meta != nullptr && score != nullptr,
               "dd_pocsag_batches: null buffer");
    hipLaunchKernelGGL(k_pocsag_batch, dim3((unsigned)m), dim3(64), 0, dd_stream(stream), audio, n, gd, list, words, errs, meta, score);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_debug_pocsag_masks(const double* audio, int64_t n, double sps, int w, int slack, uint8_t* mask, void* stream) {
    DDPocsagGrid gd = {};
    const bool served = dd_pocsag_grid(n, sps, w, slack, 0, &gd);
    hipStream_t s = dd_stream(stream);
    return dd_cand_masks_entry("dd_debug_pocsag_masks", served,
                               "dd_debug_pocsag_masks: need 0 <= n < 2^31, 4 <= sps <= 128, an odd w from 1 to 77 and 0 <= slack <= 8", audio, n,
                               gd.nstart, mask, s, dd_pocsag_sync_launch(audio, n, gd, s));
}
