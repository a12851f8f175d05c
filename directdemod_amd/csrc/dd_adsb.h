// 1090 MHz Mode S / ADS-B squitters (beyond the reference; DESIGN.md section 4.22 defines every stage, adsb.py restates each kernel in
// NumPy), included by dd_afsk.hip after dd_candidates.h, whose tail, list kernel and driver it uses.  All integer: positions in units of g = gcd(U / Q, R)
// with u = U / g units per sample, xq = U / (Q g) per candidate step and r = R / g per chip; a chip energy is the sum of
// overlap * power over the samples the chip touches, below 2^43, so sums in any order equal the restatement bit for bit.
//
//   k_adsb_preamble   -- a workgroup stages the power of 256 samples of starts and the preamble's reach in LDS, one thread per
//                        sample walks its Q candidates' 15 chips, a mask byte per sample and a count per workgroup come out
//   k_cand_list       -- (dd_candidates.h) the masks' set bits, all Q of a byte, as an ordered candidate list below the capacity
//   k_adsb_demod      -- one wave per listed candidate: 112 bit decisions by ballot, remainder, score, one-bit repair
//   k_adsb_chips      -- diagnostic: one wave per listed candidate, all 240 chip energies
#pragma once

#define DD_ADSB_U 2000000LL           // chips per second
#define DD_ADSB_TILE 256              // samples' worth of starts per workgroup (mirrored by adsb.TILE)
#define DD_ADSB_REACH 162             // samples past a tile's last start that a 16-chip preamble touches: 16 * 10 at 20 MS/s, and 2
#define DD_ADSB_CHIPS 240
#define DD_ADSB_GENERATOR 0x1FFF409u

struct DDAdsbGrid {
    uint32_t u, xq, r;                // units per sample, per candidate step, per chip
    int Q;
    int64_t ncand;                    // candidates of the recording
};

struct DDAdsbTable {
    uint32_t t[112];                  // the remainder of a lone bit at each position of a 112-bit word
};

__device__ __forceinline__ uint32_t dd_adsb_power(const uint8_t* __restrict__ iq, int64_t j) {
    const uchar2 v = ((const uchar2*)iq)[j];
    const int a = 2 * (int)v.x - 255, b = 2 * (int)v.y - 255;
    return (uint32_t)(a * a + b * b);
}

// The energy of the chip that starts f units into sample j, 0 <= f < u; (j, f) leaves as the next chip's start.
// P(j) gives the power of sample j; only samples the chip covers with a positive weight are read.
template <typename P>
__device__ __forceinline__ uint64_t dd_adsb_chip(P power, int64_t& j, uint32_t& f, uint32_t u, uint32_t r) {
    uint64_t e = 0;
    uint32_t left = r;
    while (left > 0) {
        const uint32_t w = min(u - f, left);
        e += (uint64_t)w * power(j);
        left -= w;
        f += w;
        if (f == u) {
            f = 0;
            ++j;
        }
    }
    return e;
}

__global__ void __launch_bounds__(DD_ADSB_TILE) k_adsb_preamble(const uint8_t* __restrict__ iq, int64_t n, const DDAdsbGrid gd,
                                                                uint8_t* __restrict__ mask, int* __restrict__ bsum) {
    __shared__ uint32_t ps[DD_ADSB_TILE + DD_ADSB_REACH];            // ps[j] = power of sample base + j, 0 past the recording
    __shared__ int sh[256];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * DD_ADSB_TILE;
    for (int j = tid; j < DD_ADSB_TILE + DD_ADSB_REACH; j += DD_ADSB_TILE) ps[j] = base + j < n ? dd_adsb_power(iq, base + j) : 0u;
    __syncthreads();
    const int64_t k0 = (base + tid) * gd.Q;                          // this thread's candidates start inside sample base + tid
    uint32_t m = 0;
    for (int i = 0; i < gd.Q && k0 + i < gd.ncand; ++i) {
        int64_t j = tid;
        uint32_t f = (uint32_t)i * gd.xq;
        uint64_t e[15];
#pragma unroll
        for (int c = 0; c < 15; ++c) e[c] = dd_adsb_chip([&](int64_t at) { return ps[at]; }, j, f, gd.u, gd.r);
        const uint64_t s = e[0] + e[2] + e[7] + e[9];
        const bool ok = e[0] > e[1] && e[2] > e[1] && e[2] > e[3] && e[7] > e[6] && e[7] > e[8] && e[9] > e[8] && e[9] > e[10] &&
                        6 * e[4] < s && 6 * e[5] < s && 6 * e[11] < s && 6 * e[12] < s && 6 * e[13] < s && 6 * e[14] < s;
        m |= ok ? 1u << i : 0u;
    }
    dd_cand_tail(mask, base + tid, n, m, __popc(m), sh, bsum);
}

// where candidate k's chip c starts: sample j and f units into it (k xq = (k / Q) u + (k mod Q) xq)
__device__ __forceinline__ void dd_adsb_seek(const DDAdsbGrid& gd, int64_t k, int c, int64_t& j, uint32_t& f) {
    const int64_t off = (k % gd.Q) * (int64_t)gd.xq + (int64_t)c * gd.r;
    j = k / gd.Q + off / gd.u;
    f = (uint32_t)(off % gd.u);
}

// meta[4 c] = L, DF, rem, fixed; frames[14 c]: the word with the repaired bit flipped, zero beyond L.  A k outside the
// recording's candidates gives zeros and fixed = -1.
__global__ void __launch_bounds__(64) k_adsb_demod(const uint8_t* __restrict__ iq, const DDAdsbGrid gd, const DDAdsbTable tb,
                                                   const int64_t* __restrict__ list, uint8_t* __restrict__ frames,
                                                   int* __restrict__ meta, int64_t* __restrict__ score) {
    const int lane = threadIdx.x;
    const int64_t k = list[blockIdx.x];
    const bool inside = k >= 0 && k < gd.ncand;                      // (uniform over the wave)
    const auto power = [&](int64_t at) { return dd_adsb_power(iq, at); };
    bool bit[2] = {false, false};
    int64_t dif[2] = {0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {                                    // this lane's bits: lane and lane + 64
        const int b = lane + 64 * h;
        if (inside && b < 112) {
            int64_t j;
            uint32_t f;
            dd_adsb_seek(gd, k, 16 + 2 * b, j, f);
            const uint64_t hi = dd_adsb_chip(power, j, f, gd.u, gd.r);
            const uint64_t lo = dd_adsb_chip(power, j, f, gd.u, gd.r);
            bit[h] = hi > lo;
            dif[h] = hi > lo ? (int64_t)(hi - lo) : (int64_t)(lo - hi);
        }
    }
    unsigned long long w0 = __ballot(bit[0]), w1 = __ballot(bit[1]); // bit b of the word is bit b of w0, bit b - 64 of w1
    const int df = (int)(((w0 & 1) << 4) | ((w0 & 2) << 2) | (w0 & 4) | ((w0 & 8) >> 2) | ((w0 & 16) >> 4));
    const int L = inside ? (df >= 16 ? 112 : 56) : 0;
    if (L < 112) {
        w1 = 0;
        w0 &= L == 56 ? (1ull << 56) - 1 : 0ull;
    }
    const int shift = 112 - L;                                       // a 56-bit word uses the table's tail
    uint32_t rem = 0;
    int64_t sc = 0;
    if (lane < L) {
        rem = ((w0 >> lane) & 1) ? tb.t[lane + shift] : 0u;
        sc = dif[0];
    }
    if (lane + 64 < L) {
        rem ^= ((w1 >> lane) & 1) ? tb.t[lane + 64] : 0u;
        sc += dif[1];
    }
    for (int o = 32; o > 0; o >>= 1) {
        rem ^= __shfl_xor(rem, o);
        sc += __shfl_xor(sc, o);
    }
    int fixed = -1;
    if (L == 112 && (df == 17 || df == 18) && rem != 0) {            // the syndrome of one wrong bit is that bit's table entry
        const unsigned long long m0 = __ballot(lane >= 5 && rem == tb.t[lane]);
        const unsigned long long m1 = __ballot(lane < 48 && rem == tb.t[lane + 64]);
        if (__popcll(m0) + __popcll(m1) == 1) {
            fixed = m0 ? __ffsll((long long)m0) - 1 : 64 + __ffsll((long long)m1) - 1;
            w0 ^= m0;
            w1 ^= m1;
        }
    }
    if (lane < 14) {
        const unsigned long long w = lane < 8 ? w0 >> (8 * lane) : w1 >> (8 * (lane - 8));
        uint32_t v = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) v |= (uint32_t)((w >> t) & 1) << (7 - t);
        frames[(int64_t)blockIdx.x * 14 + lane] = (uint8_t)v;
    }
    if (lane == 0) {
        int* mt = meta + (int64_t)blockIdx.x * 4;
        mt[0] = L;
        mt[1] = inside ? df : 0;
        mt[2] = (int)rem;
        mt[3] = fixed;
        score[blockIdx.x] = sc;
    }
}

__global__ void __launch_bounds__(64) k_adsb_chips(const uint8_t* __restrict__ iq, const DDAdsbGrid gd, const int64_t* __restrict__ list,
                                                   int64_t* __restrict__ E) {
    const int64_t k = list[blockIdx.x];
    const bool inside = k >= 0 && k < gd.ncand;
    for (int c = threadIdx.x; c < DD_ADSB_CHIPS; c += 64) {
        uint64_t e = 0;
        if (inside) {
            int64_t j;
            uint32_t f;
            dd_adsb_seek(gd, k, c, j, f);
            e = dd_adsb_chip([&](int64_t at) { return dd_adsb_power(iq, at); }, j, f, gd.u, gd.r);
        }
        E[(int64_t)blockIdx.x * DD_ADSB_CHIPS + c] = (int64_t)e;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the C entries
static int64_t dd_adsb_gcd(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// 0 when the rate, the phase count or a size is not served, else 1 with the grid filled
static int dd_adsb_grid(int64_t n, int64_t rate, int Q, DDAdsbGrid* gd) {
    if (n < 0 || n > 0x7FFFFFF0LL / 8 || rate < 2000000 || rate > 20000000 || !(Q == 1 || Q == 2 || Q == 4 || Q == 8)) return 0;
    const int64_t g = dd_adsb_gcd(DD_ADSB_U / Q, rate);
    gd->u = (uint32_t)(DD_ADSB_U / g);
    gd->xq = (uint32_t)(DD_ADSB_U / Q / g);
    gd->r = (uint32_t)(rate / g);
    gd->Q = Q;
    const int64_t room = n * DD_ADSB_U - DD_ADSB_CHIPS * rate;
    gd->ncand = room < 0 ? 0 : room / (DD_ADSB_U / Q) + 1;
    return 1;
}

static const DDAdsbTable& dd_adsb_table() {
    static const DDAdsbTable tb = [] {
        DDAdsbTable t;
        uint32_t v = 1;
        for (int i = 111; i >= 0; --i) {
            t.t[i] = v;
            v <<= 1;
            if (v & (1u << 24)) v ^= DD_ADSB_GENERATOR;
        }
        return t;
    }();
    return tb;
}

extern "C" int dd_adsb_candidates(const void* iq, int64_t n, int64_t rate, int phases, int64_t* list, int64_t cap, int64_t* count_host,
                                  void* stream) {
    DDAdsbGrid gd = {};
    const bool served = cap >= 0 && dd_adsb_grid(n, rate, phases, &gd);
    hipStream_t s = dd_stream(stream);
    const int64_t starts = served ? (gd.ncand + phases - 1) / phases : 0;   // samples that hold a candidate's start
    return dd_cand_entry("dd_adsb_candidates", served,
                         "dd_adsb_candidates: need 0 <= n < 2^28, 2 000 000 <= rate <= 20 000 000, phases of 1, 2, 4, 8 and cap >= 0", iq, n,
                         starts, phases, 0xFFu, list, cap, count_host, s, [=](uint8_t* mask, int* bsum, int64_t nb) {
                             hipLaunchKernelGGL(k_adsb_preamble, dim3((unsigned)nb), dim3(DD_ADSB_TILE), 0, s, (const uint8_t*)iq, n, gd, mask,
                                                bsum);
                         });
}

extern "C" int dd_adsb_demod(const void* iq, int64_t n, int64_t rate, int phases, const int64_t* list, int64_t m, uint8_t* frames,
                             int32_t* meta, int64_t* score, void* stream) {
    DDAdsbGrid gd;
    DD_REQUIRE(m >= 0 && m <= 0x7FFFFFFFLL && dd_adsb_grid(n, rate, phases, &gd),
               "dd_adsb_demod: need 0 <= n < 2^28, 2 000 000 <= rate <= 20 000 000, phases of 1, 2, 4, 8 and 0 <= m < 2^31");
    if (n == 0 || m == 0) return DD_OK;
    DD_REQUIRE(iq != nullptr && list != nullptr && frames != nullptr && meta != nullptr && score != nullptr, "dd_adsb_demod: null buffer");
    hipLaunchKernelGGL(k_adsb_demod, dim3((unsigned)m), dim3(64), 0, dd_stream(stream), (const uint8_t*)iq, gd, dd_adsb_table(), list, frames,
                       meta, score);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_debug_adsb_chips(const void* iq, int64_t n, int64_t rate, int phases, const int64_t* list, int64_t m, int64_t* energies,
                                   void* stream) {
    DDAdsbGrid gd;
    DD_REQUIRE(m >= 0 && m <= 0x7FFFFFFFLL && dd_adsb_grid(n, rate, phases, &gd),
               "dd_debug_adsb_chips: need 0 <= n < 2^28, 2 000 000 <= rate <= 20 000 000, phases of 1, 2, 4, 8 and 0 <= m < 2^31");
    if (n == 0 || m == 0) return DD_OK;
    DD_REQUIRE(iq != nullptr && list != nullptr && energies != nullptr, "dd_debug_adsb_chips: null buffer");
    hipLaunchKernelGGL(k_adsb_chips, dim3((unsigned)m), dim3(64), 0, dd_stream(stream), (const uint8_t*)iq, gd, list, energies);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
