// RDS on broadcast FM, 1187.5 bit/s differential biphase on a 57 kHz subcarrier of the multiplex (beyond the reference; DESIGN.md
// section 4.27 defines every stage, rds.py restates each kernel in NumPy), included by dd_afsk.hip after dd_candidates.h, whose LDS
// prefix sum, tail, list kernel and driver it uses; the quantiser and the positions are its own.  The multiplex is the FM
// discriminator's float64 output in radians per sample; everything behind the quantiser is integer, so sums in any order equal the
// restatement bit for bit.  Positions are float64 products and sums rounded one by one (the unit is built without contraction).
//
//   k_rds_baseband    -- a workgroup stages the quantised multiplex of 256 outputs in LDS beside the 1024-entry phasor table; a thread
//                        per output sums D products q * table[phase] in int64 and stores the sum >> 10 as an int32 pair
//   k_rds_sync        -- a workgroup stages the baseband of 256 starts and the reach of 105 bit boundaries in LDS and turns both
//                        components into exclusive prefix sums in place (dd_prefix256; 32-bit wrap-around: |z| < 2^30, so
//                        differences are exact); one thread per start takes the 105 half-bit differences, three LDS reads per
//                        component, decides 104 bits by the sign of Re(z[p_k] conj(z[p_k-1])) and runs them through the
//                        remainder register of four 26-bit blocks; a mask byte per start, a count per workgroup
//   k_cand_list       -- (dd_candidates.h) the masks' pass bits as an ordered candidate list below the capacity
//   k_rds_groups      -- one wave per listed start: 104 bits by two ballots, the four remainders as wave XORs of lone-bit
//                        remainders, burst repair searched a lane per position and pattern
//   k_rds_halfbit, k_rds_repair -- (diagnostics) the half-bit differences of every sample; the repair of loose 26-bit words
#pragma once

#define DD_RDS_TILE 256               // outputs, starts per workgroup (mirrored by rds.TILE)
#define DD_RDS_D_MAX 32               // multiplex samples summed per baseband sample at most
#define DD_RDS_SHIFT 10               // |q| <= 2^15, |table| <= 2^14, 32 products: |sum| <= 2^34, |b| <= 2^24
#define DD_RDS_H_MAX 16               // floor(sps / 2) at most: |z| <= 2 * 16 * 2^24 = 2^29, |Re(z z')| <= 2^59
#define DD_RDS_BITS 104
#define DD_RDS_SPAN 3624              // prefix entries of a tile at most: 256 + floor(103 * 32) + 2 + 16 + (32 + 16 + 1) + 1 = 3620
#define DD_RDS_GEN 0x5B9u             // x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
#define DD_RDS_SCALE (32768.0 / 3.14159265358979323846)
#define DD_RDS_CLIP 32768.0           // |q| <= 2^15: what a discriminator can give; beyond it and for a NaN q = 0
#define DD_RDS_METRIC_SHIFT 20
#define DD_RDS_METRIC_CAP 16777216    // per bit; the metric of a group is at most 104 * 2^24 < 2^31
#define DD_RDS_META 8

static_assert(DD_RDS_TILE + 103 * 32 + 2 + DD_RDS_H_MAX + (32 + DD_RDS_H_MAX + 1) + 1 <= DD_RDS_SPAN, "a tile's span at 32 samples per bit");
static_assert(2 * 4 * DD_RDS_SPAN + 4 * 256 + 16 <= 65536 && 4 * DD_RDS_TILE * (DD_RDS_D_MAX + 1) + 8 * 1024 <= 65536, "a workgroup's LDS");

enum { DD_RDS_OK = 0, DD_RDS_OUTSIDE = 1 };
enum { DD_RDS_A = 0, DD_RDS_B = 1, DD_RDS_C = 2, DD_RDS_CP = 3, DD_RDS_D = 4 };

struct DDRdsGrid {
    double sps;                       // baseband samples per bit
    int h, clean, fix;                // a half bit sums h samples; clean blocks a listed start needs; bits a burst may span
    int lead, span;                   // samples staged before a tile's first start; prefix entries of a tile
    int64_t m;                        // baseband samples
};

struct DDRdsTable {
    uint16_t x[32];                   // x[e] = x^e mod the generator: the remainder of a lone one in bit e of a block
};

constexpr DDRdsTable dd_rds_make_table() {
    DDRdsTable t{};
    unsigned v = 1u;
    for (int e = 0; e < 32; ++e) {
        t.x[e] = (uint16_t)v;
        v <<= 1;
        if (v & 0x400u) v ^= DD_RDS_GEN;
    }
    return t;
}

__constant__ const DDRdsTable dd_rds_table = dd_rds_make_table();
__constant__ const uint16_t dd_rds_offset[5] = {0x0FC, 0x198, 0x168, 0x350, 0x1B4};      // A, B, C, C', D

__device__ __forceinline__ int dd_rds_q(double x) {
    const double r = rint(x * DD_RDS_SCALE);
    return (r >= -DD_RDS_CLIP && r <= DD_RDS_CLIP) ? (int)r : 0;
}

// the boundary sample p_k of the start t: bit k lies between p_(k-1) and p_k
__device__ __forceinline__ int64_t dd_rds_pos(int64_t t, int k, double sps) {
    return (int64_t)floor(((double)t + (double)k * sps) + 0.5);
}

// the group of the start t lies inside the data: p_-1 >= 0 and p_103 <= m - h
__device__ __forceinline__ bool dd_rds_fits(int64_t t, const DDRdsGrid& gd) {
    return t >= 0 && t < gd.m && dd_rds_pos(t, -1, gd.sps) >= 0 && dd_rds_pos(t, DD_RDS_BITS - 1, gd.sps) <= gd.m - gd.h;
}

// b[2 o], b[2 o + 1] = (sum over i < D of q[o D + i] * table[phase(n0 + o D + i)]) >> 10, phase(n) = bits 31 .. 22 of n * step mod 2^32
__global__ void __launch_bounds__(DD_RDS_TILE) k_rds_baseband(const double* __restrict__ x, int64_t nout, int D, uint64_t n0, uint64_t step,
                                                              const int2* __restrict__ table, int2* __restrict__ b) {
    __shared__ int qs[DD_RDS_TILE * (DD_RDS_D_MAX + 1)];             // output o's samples from o * (D | 1) on: an odd stride, no bank shared
    __shared__ int2 tb[1024];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * DD_RDS_TILE;
    const int outs = nout - base < DD_RDS_TILE ? (int)(nout - base) : DD_RDS_TILE;
    const int row = D | 1;
    for (int j = tid; j < outs * D; j += DD_RDS_TILE) qs[j / D * row + j % D] = dd_rds_q(x[base * D + j]);
    for (int j = tid; j < 1024; j += DD_RDS_TILE) tb[j] = table[j];
    __syncthreads();
    if (tid >= outs) return;
    const uint64_t first = n0 + (uint64_t)(base + tid) * (uint64_t)D;
    int64_t re = 0, im = 0;
    for (int i = 0; i < D; ++i) {
        const int2 w = tb[(uint32_t)((first + (uint64_t)i) * step) >> 22];
        const int64_t q = qs[tid * row + i];
        re += q * w.x;
        im += q * w.y;
    }
    b[base + tid] = make_int2((int)(re >> DD_RDS_SHIFT), (int)(im >> DD_RDS_SHIFT));
}

// pr, pi[0 .. span) = the exclusive wrap-around prefix sums of the two components of b[first .. first + span), 0 outside the data
__device__ __forceinline__ void dd_rds_stage(const int2* __restrict__ b, int64_t m, int64_t first, int span, uint32_t* pr, uint32_t* pi,
                                             uint32_t* tops) {
    for (int j = threadIdx.x; j < span; j += DD_RDS_TILE) {                 // (one read serves both components: not dd_stage_prefix256)
        const int64_t i = first + j;
        const int2 v = (i >= 0 && i < m) ? b[i] : make_int2(0, 0);
        pr[j] = (uint32_t)v.x;
        pi[j] = (uint32_t)v.y;
    }
    __syncthreads();
    dd_prefix256(pr, span, tops);
    dd_prefix256(pi, span, tops);
}

// z[p] = the sum of b[p .. p + h - 1] less the sum of b[p - h .. p - 1] from the prefix sums, at = p - first; 0 below p = h
__device__ __forceinline__ int2 dd_rds_z(const uint32_t* pr, const uint32_t* pi, int at, int64_t p, int h) {
    if (p < h) return make_int2(0, 0);
    return make_int2((int)(pr[at + h] - 2u * pr[at] + pr[at - h]), (int)(pi[at + h] - 2u * pi[at] + pi[at - h]));
}

// mask[t] = score << 1 | (score >= clean), score = the blocks of the start t whose remainder is their offset word's: A, B, C or C', D
__global__ void __launch_bounds__(DD_RDS_TILE) k_rds_sync(const int2* __restrict__ b, const DDRdsGrid gd, uint8_t* __restrict__ mask,
                                                          int* __restrict__ bsum) {
    __shared__ uint32_t pr[DD_RDS_SPAN];
    __shared__ uint32_t pi[DD_RDS_SPAN];
    __shared__ int sh[256];
    __shared__ uint32_t tops[4];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * DD_RDS_TILE;
    const int64_t first = base - gd.lead;
    dd_rds_stage(b, gd.m, first, gd.span, pr, pi, tops);
    const int64_t t = base + tid;
    uint32_t score = 0;
    if (dd_rds_fits(t, gd)) {
        // h <= p - first and p + h - first < span for every boundary of a start that fits (a rounding of the sums included)
        int64_t p = dd_rds_pos(t, -1, gd.sps);
        int2 was = dd_rds_z(pr, pi, (int)(p - first), p, gd.h);
        for (int blk = 0; blk < 4; ++blk) {
            uint32_t r = 0;
            for (int i = 0; i < 26; ++i) {
                p = dd_rds_pos(t, 26 * blk + i, gd.sps);
                const int2 z = dd_rds_z(pr, pi, (int)(p - first), p, gd.h);
                const int64_t prod = (int64_t)z.x * was.x + (int64_t)z.y * was.y;
                r = (r << 1) | (prod < 0 ? 1u : 0u);
                if (r & 0x400u) r ^= DD_RDS_GEN;
                was = z;
            }
            const bool ok = blk == 2 ? (r == dd_rds_offset[DD_RDS_C] || r == dd_rds_offset[DD_RDS_CP])
                                     : r == dd_rds_offset[blk == 3 ? DD_RDS_D : blk];
            score += ok ? 1u : 0u;
        }
    }
    const uint32_t pass = score >= (uint32_t)gd.clean ? 1u : 0u;
    dd_cand_tail(mask, t, gd.m, score << 1 | pass, (int)pass, sh, bsum);
}

// z[2 p], z[2 p + 1] for every sample p (a diagnostic): 0 below h and beyond m - h
__global__ void __launch_bounds__(DD_RDS_TILE) k_rds_halfbit(const int2* __restrict__ b, int64_t m, int h, int2* __restrict__ z) {
    __shared__ uint32_t pr[DD_RDS_TILE + 2 * DD_RDS_H_MAX];
    __shared__ uint32_t pi[DD_RDS_TILE + 2 * DD_RDS_H_MAX];
    __shared__ uint32_t tops[4];
    const int64_t base = (int64_t)blockIdx.x * DD_RDS_TILE;
    dd_rds_stage(b, m, base - h, DD_RDS_TILE + 2 * h, pr, pi, tops);
    const int64_t p = base + threadIdx.x;
    if (p < m) z[p] = p <= m - h ? dd_rds_z(pr, pi, (int)threadIdx.x + h, p, h) : make_int2(0, 0);
}

__device__ __forceinline__ uint32_t dd_rds_wave_xor(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// The block w whose remainder differs from its offset word by syn: 0 when syn is 0; else the one burst of at most `fix` bits inside
// the 26 whose remainder is syn is taken out of w and its ones are counted; -1 when there is none.  Lane c of round r tries pattern
// 2 (c / 26) + 1 (the odd numbers below 32: a burst begins and ends in a wrong bit) shifted up c mod 26 places; the 367 bursts that
// fit have 367 distinct remainders, so at most one lane hits.  Uniform over the wave.
__device__ __forceinline__ int dd_rds_repair(uint32_t& w, uint32_t syn, int fix, int lane) {
    if (syn == 0u) return 0;
    for (int r = 0; r < 7; ++r) {
        const int c = 64 * r + lane, up = c % 26;
        const uint32_t pat = 2u * (uint32_t)(c / 26) + 1u;
        const int len = 32 - __clz((int)pat);
        uint32_t rem = 0;
        for (int q = 0; q < 5; ++q) rem ^= (pat >> q) & 1u ? dd_rds_table.x[(up + q) & 31] : 0u;
        const unsigned long long hits = __ballot(pat < 32u && len <= fix && up + len <= 26 && rem == syn);
        if (hits) {
            const uint32_t e = (uint32_t)__shfl((int)(pat << up), __ffsll((long long)hits) - 1);
            w ^= e;
            return __popc(e);
        }
    }
    return -1;
}

// words[4 c ..]: the four information words, repaired where a status says so and as received where it is -1; meta[8 c ..] = the four
// statuses (0 clean, n bits repaired, -1 not decodable), the third block's offset word (0 C, 1 C'), the merge metric, DD_RDS_OK or
// DD_RDS_OUTSIDE, the blocks decoded.  A start whose group does not fit the data gives DD_RDS_OUTSIDE, zeros and statuses of -1.
__global__ void __launch_bounds__(64) k_rds_groups(const int2* __restrict__ b, const DDRdsGrid gd, const int64_t* __restrict__ list,
                                                   uint16_t* __restrict__ words, int* __restrict__ meta) {
    const int lane = threadIdx.x;
    const int64_t t = list[blockIdx.x];
    uint16_t* wo = words + (int64_t)blockIdx.x * 4;
    int* mt = meta + (int64_t)blockIdx.x * DD_RDS_META;
    if (!dd_rds_fits(t, gd)) {                                           // (uniform over the wave)
        if (lane < 4) wo[lane] = 0;
        if (lane < DD_RDS_META) mt[lane] = lane < 4 ? -1 : (lane == 6 ? DD_RDS_OUTSIDE : 0);
        return;
    }
    const auto zat = [&](int k) {                                        // h <= p <= m - h for every boundary but a p_-1 below h
        const int64_t p = dd_rds_pos(t, k, gd.sps);
        int zr = 0, zi = 0;
        if (p >= gd.h)
            for (int j = 0; j < gd.h; ++j) {
                const int2 a = b[p + j], c = b[p - 1 - j];
                zr += a.x - c.x;
                zi += a.y - c.y;
            }
        return make_int2(zr, zi);
    };
    // bit 64 j + lane of the group is lane `lane` of ballot j
    unsigned long long bal[2];
    uint32_t s[4] = {0u, 0u, 0u, 0u};
    int metric = 0;
    for (int j = 0; j < 2; ++j) {
        const int k = 64 * j + lane;
        const bool valid = k < DD_RDS_BITS;
        int64_t prod = 0;
        if (valid) {
            const int2 z = zat(k), was = zat(k - 1);
            prod = (int64_t)z.x * was.x + (int64_t)z.y * was.y;
        }
        bal[j] = __ballot(prod < 0);
        const int64_t mag = (prod < 0 ? -prod : prod) >> DD_RDS_METRIC_SHIFT;
        metric += (int)(mag < DD_RDS_METRIC_CAP ? mag : DD_RDS_METRIC_CAP);
        const uint32_t mine = prod < 0 ? dd_rds_table.x[25 - k % 26] : 0u;
        for (int blk = 0; blk < 4; ++blk) s[blk] ^= dd_rds_wave_xor(valid && k / 26 == blk ? mine : 0u);
    }
    for (int o = 32; o > 0; o >>= 1) metric += __shfl_xor(metric, o);
    uint32_t w[4];
    for (int blk = 0; blk < 4; ++blk) {
        uint32_t v = 0;
        for (int i = 0; i < 26; ++i) {
            const int k = 26 * blk + i;
            v = v << 1 | (uint32_t)((bal[k >> 6] >> (k & 63)) & 1ull);
        }
        w[blk] = v;
    }
    int st[4];
    st[0] = dd_rds_repair(w[0], s[0] ^ dd_rds_offset[DD_RDS_A], gd.fix, lane);
    st[1] = dd_rds_repair(w[1], s[1] ^ dd_rds_offset[DD_RDS_B], gd.fix, lane);
    // version B (bit 11 of the second information word) sends C' in the third block
    const int third = st[1] >= 0 ? (int)(w[1] >> 21 & 1u) : (s[2] == dd_rds_offset[DD_RDS_CP] ? 1 : 0);
    st[2] = dd_rds_repair(w[2], s[2] ^ dd_rds_offset[third ? DD_RDS_CP : DD_RDS_C], gd.fix, lane);
    st[3] = dd_rds_repair(w[3], s[3] ^ dd_rds_offset[DD_RDS_D], gd.fix, lane);
    if (lane == 0) {
        int good = 0;
        for (int blk = 0; blk < 4; ++blk) {
            wo[blk] = (uint16_t)(w[blk] >> 10);
            mt[blk] = st[blk];
            good += st[blk] >= 0 ? 1 : 0;
        }
        mt[4] = third;
        mt[5] = metric;
        mt[6] = DD_RDS_OK;
        mt[7] = good;
    }
}

// word c of 26 bits against offset word offs[c] (0 .. 4): fixed[c] = the block repaired or as received, status[c] as k_rds_groups gives it
__global__ void __launch_bounds__(64) k_rds_repair(const uint32_t* __restrict__ words, const int* __restrict__ offs, int fix,
                                                   uint32_t* __restrict__ fixed, int* __restrict__ status) {
    const int lane = threadIdx.x;
    uint32_t w = words[blockIdx.x] & 0x3FFFFFFu;
    const uint32_t s = dd_rds_wave_xor(lane < 26 && (w >> lane & 1u) ? dd_rds_table.x[lane] : 0u);
    const int o = offs[blockIdx.x];
    const int st = dd_rds_repair(w, s ^ dd_rds_offset[o < 0 ? 0 : (o > 4 ? 4 : o)], fix, lane);
    if (lane == 0) {
        fixed[blockIdx.x] = w;
        status[blockIdx.x] = st;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the C entries
// 0 when a size, the samples per bit, the clean count or the burst length is not served, else 1 with the grid filled
static int dd_rds_grid(int64_t m, double sps, int clean, int fix, DDRdsGrid* gd) {
    if (m < 0 || m > 0x7FFFFFF0LL || !(sps >= 12.0 && sps <= 32.0) || clean < 2 || clean > 4 || fix < 0 || fix > 5) return 0;
    gd->sps = sps;
    gd->h = (int)floor(sps / 2.0);
    gd->clean = clean;
    gd->fix = fix;
    gd->lead = (int)ceil(sps) + gd->h + 1;
    gd->span = DD_RDS_TILE + (int)floor(103.0 * sps) + 2 + gd->h + gd->lead + 1;
    gd->m = m;
    return 1;
}

extern "C" int dd_rds_baseband(const double* mpx, int64_t n, int D, uint64_t n0, uint64_t step, const int32_t* table, int32_t* b,
                               void* stream) {
    DD_REQUIRE(n >= 0 && D >= 1 && D <= DD_RDS_D_MAX && n / D <= 0x7FFFFFF0LL, "dd_rds_baseband: need n >= 0, 1 <= D <= 32 and n / D < 2^31");
    const int64_t nout = n / D;
    if (nout == 0) return DD_OK;
    DD_REQUIRE(mpx != nullptr && table != nullptr && b != nullptr, "dd_rds_baseband: null buffer");
    const int64_t nb = (nout + DD_RDS_TILE - 1) / DD_RDS_TILE;
    hipLaunchKernelGGL(k_rds_baseband, dim3((unsigned)nb), dim3(DD_RDS_TILE), 0, dd_stream(stream), mpx, nout, D, n0, step,
                       (const int2*)table, (int2*)b);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

static auto dd_rds_sync_launch(const int32_t* b, const DDRdsGrid& gd, hipStream_t s) {
    return [=](uint8_t* mask, int* bsum, int64_t nb) {
        hipLaunchKernelGGL(k_rds_sync, dim3((unsigned)nb), dim3(DD_RDS_TILE), 0, s, (const int2*)b, gd, mask, bsum);
    };
}

extern "C" int dd_rds_candidates(const int32_t* b, int64_t m, double sps, int clean, int64_t* list, int64_t cap, int64_t* count_host,
                                 void* stream) {
    DDRdsGrid gd = {};
    const bool served = cap >= 0 && dd_rds_grid(m, sps, clean, 0, &gd);
    hipStream_t s = dd_stream(stream);
    return dd_cand_entry("dd_rds_candidates", served, "dd_rds_candidates: need 0 <= m < 2^31, 12 <= sps <= 32, 2 <= clean <= 4 and cap >= 0", b,
                         m, m, 1, 1u, list, cap, count_host, s, dd_rds_sync_launch(b, gd, s));
}

extern "C" int dd_rds_groups(const int32_t* b, int64_t m, double sps, int fix, const int64_t* list, int64_t count, uint16_t* words,
                             int32_t* meta, void* stream) {
    DDRdsGrid gd;
    DD_REQUIRE(count >= 0 && count <= 0x7FFFFFFFLL && dd_rds_grid(m, sps, 2, fix, &gd),
               "dd_rds_groups: need 0 <= m < 2^31, 12 <= sps <= 32, 0 <= fix <= 5 and 0 <= count < 2^31");
    if (count == 0) return DD_OK;
    DD_REQUIRE((b != nullptr || m == 0) && list != nullptr && words != nullptr && meta != nullptr, "dd_rds_groups: null buffer");
    hipLaunchKernelGGL(k_rds_groups, dim3((unsigned)count), dim3(64), 0, dd_stream(stream), (const int2*)b, gd, list, words, meta);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_debug_rds_masks(const int32_t* b, int64_t m, double sps, int clean, uint8_t* mask, void* stream) {
    DDRdsGrid gd = {};
    const bool served = dd_rds_grid(m, sps, clean, 0, &gd);
    hipStream_t s = dd_stream(stream);
    return dd_cand_masks_entry("dd_debug_rds_masks", served, "dd_debug_rds_masks: need 0 <= m < 2^31, 12 <= sps <= 32 and 2 <= clean <= 4", b, m, m,
                               mask, s, dd_rds_sync_launch(b, gd, s));
}

extern "C" int dd_debug_rds_halfbit(const int32_t* b, int64_t m, double sps, int32_t* z, void* stream) {
    DDRdsGrid gd;
    DD_REQUIRE(dd_rds_grid(m, sps, 2, 0, &gd), "dd_debug_rds_halfbit: need 0 <= m < 2^31 and 12 <= sps <= 32");
    if (m == 0) return DD_OK;
    DD_REQUIRE(b != nullptr && z != nullptr, "dd_debug_rds_halfbit: null buffer");
    const int64_t nb = (m + DD_RDS_TILE - 1) / DD_RDS_TILE;
    hipLaunchKernelGGL(k_rds_halfbit, dim3((unsigned)nb), dim3(DD_RDS_TILE), 0, dd_stream(stream), (const int2*)b, m, gd.h, (int2*)z);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_debug_rds_repair(const uint32_t* words, const int32_t* offs, int64_t count, int fix, uint32_t* fixed, int32_t* status,
                                   void* stream) {
    DD_REQUIRE(count >= 0 && count <= 0x7FFFFFFFLL && fix >= 0 && fix <= 5, "dd_debug_rds_repair: need 0 <= count < 2^31 and 0 <= fix <= 5");
    if (count == 0) return DD_OK;
    DD_REQUIRE(words != nullptr && offs != nullptr && fixed != nullptr && status != nullptr, "dd_debug_rds_repair: null buffer");
    hipLaunchKernelGGL(k_rds_repair, dim3((unsigned)count), dim3(64), 0, dd_stream(stream), words, offs, fix, fixed, status);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
