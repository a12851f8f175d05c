// AIS, 9600 baud GMSK bursts carrying HDLC frames (beyond the reference; DESIGN.md section 4.23 defines every stage, ais.py restates
// each kernel in NumPy), included by dd_afsk.hip after dd_candidates.h, whose tail, list kernel and driver it uses.  The audio is
// the FM discriminator's float64 output in radians per sample.  One multiply and one rint make an integer of each sample (dd_fm_q);
// everything behind that is integer, so sums in any order equal the restatement bit for bit.  The positions are float64 products and sums rounded one
// by one (the unit is built without contraction), as dd_sstv_pixels forms its pixel edges.
//
//   k_ais_preamble    -- a workgroup stages the quantised audio of 256 starts and the reach of 24 bits in LDS, one thread per start
//                        decides the 24 template bits against the training bits' mean; a mask byte per sample, a count per workgroup
//   k_cand_list       -- (dd_candidates.h) the masks' pass bits as an ordered candidate list below the capacity
//   k_ais_demod       -- one wave per listed candidate: 1280 levels by ballot, NRZI, end flag, de-stuffing by masks and prefix counts,
//                        the CRC as a wave XOR of lone-bit remainders
#pragma once

#define DD_AIS_TILE 256               // starts per workgroup (mirrored by ais.TILE)
#define DD_AIS_TEMPLATE 24            // bits of the template: 16 training bits and the start flag
#define DD_AIS_MARGIN 8               // samples before a tile's first start that a window may touch (w <= 15)
#define DD_AIS_REACH 392              // samples past a tile's last start: floor(23.5 * 16) + 7 + 1 = 384, and room for a rounding
#define DD_AIS_BITS 1280              // raw bits behind the start flag, 20 per lane
#define DD_AIS_WORDS 20
#define DD_AIS_FRAME 160              // bytes per candidate of dd_ais_demod's frames
#define DD_AIS_PLUS 0x80CCCCu         // the template's + levels: (- - + +) x 4, seven -, one +; bit k = template bit k

enum { DD_AIS_OK = 0, DD_AIS_NO_END = 1, DD_AIS_ABORT = 2, DD_AIS_STUFFING = 3, DD_AIS_LENGTH = 4, DD_AIS_CRC = 5 };

struct DDAisGrid {
    double sps;                       // samples per bit
    int h, slack;                     // a bit value sums 2 h + 1 samples; template places that may differ
    int64_t nstart;                   // starts whose template ends inside the audio
};

struct DDAisTable {
    uint16_t z[DD_AIS_BITS];          // the CRC register m zero bits after a lone one bit entered an empty register
};

constexpr DDAisTable dd_ais_make_table() {
    DDAisTable t{};
    unsigned v = 0x8408u;
    for (int m = 0; m < DD_AIS_BITS; ++m) {
        t.z[m] = (uint16_t)v;
        v = (v & 1u) ? ((v >> 1) ^ 0x8408u) : (v >> 1);
    }
    return t;
}

__constant__ const DDAisTable dd_ais_table = dd_ais_make_table();

__global__ void __launch_bounds__(DD_AIS_TILE) k_ais_preamble(const double* __restrict__ x, int64_t n, const DDAisGrid gd,
                                                               uint8_t* __restrict__ mask, int* __restrict__ bsum) {
    __shared__ int qs[DD_AIS_MARGIN + DD_AIS_TILE + DD_AIS_REACH];   // qs[j] = q of sample base - margin + j, 0 outside the audio
    __shared__ int sh[256];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * DD_AIS_TILE;
    for (int j = tid; j < DD_AIS_MARGIN + DD_AIS_TILE + DD_AIS_REACH; j += DD_AIS_TILE) {
        const int64_t i = base - DD_AIS_MARGIN + j;
        qs[j] = (i >= 0 && i < n) ? dd_fm_q(x[i]) : 0;
    }
    __syncthreads();
    const int64_t t = base + tid;
    uint32_t m = 0;
    if (t < gd.nstart) {
        int v[DD_AIS_TEMPLATE];
        int S = 0;
#pragma unroll
        for (int k = 0; k < DD_AIS_TEMPLATE; ++k) {
            const int at = (int)(dd_bit_mid(t, k, gd.sps) - base) + DD_AIS_MARGIN;
            int s = 0;
            for (int j = -gd.h; j <= gd.h; ++j) s += qs[at + j];
            v[k] = s;
            if (k < 16) S += s;
        }
        uint32_t d = 0;
#pragma unroll
        for (int k = 0; k < DD_AIS_TEMPLATE; ++k) d |= 16 * v[k] > S ? 1u << k : 0u;
        const int mis = __popc(d ^ DD_AIS_PLUS);
        m = mis <= gd.slack ? 1u : (DD_AIS_TEMPLATE - mis <= gd.slack ? 3u : 0u);
    }
    dd_cand_tail(mask, t, n, m, (int)(m & 1u), sh, bsum);
}

// frames[160 c]: the de-stuffed bits, the first in bit 0 of byte 0 (AIS sends every byte lowest bit first, so these are the
// message's bytes), zero beyond the bit count; meta[4 c] = status, bit count, CRC register, polarity; score[c].
// A start outside the audio gives DD_AIS_NO_END and zeros.
__global__ void __launch_bounds__(64) k_ais_demod(const double* __restrict__ x, int64_t n, const DDAisGrid gd,
                                                  const int64_t* __restrict__ list, uint8_t* __restrict__ frames,
                                                  int* __restrict__ meta, int64_t* __restrict__ score) {
    __shared__ unsigned int ob[DD_AIS_FRAME / 4];
    __shared__ unsigned long long bw[DD_AIS_WORDS + 1];
    const int lane = threadIdx.x;
    const int64_t t = list[blockIdx.x];
    uint32_t* out = (uint32_t*)(frames + (int64_t)blockIdx.x * DD_AIS_FRAME);
    int* mt = meta + (int64_t)blockIdx.x * 4;
    if (lane < DD_AIS_FRAME / 4) ob[lane] = 0u;
    if (t < 0 || t >= n) {                                           // (uniform over the wave)
        if (lane < DD_AIS_FRAME / 4) out[lane] = 0u;
        if (lane == 0) {
            mt[0] = DD_AIS_NO_END;
            mt[1] = mt[2] = mt[3] = 0;
            score[blockIdx.x] = 0;
        }
        return;
    }
    const auto value = [&](int k) { return dd_window_sum(x, n, dd_bit_mid(t, k, gd.sps), gd.h); };
    // the template: S, the decisions' distance from the template, the score
    const int vt = lane < DD_AIS_TEMPLATE ? value(lane) : 0;
    int S = lane < 16 ? vt : 0;
    for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
    const unsigned long long tm = __ballot(lane < DD_AIS_TEMPLATE && 16 * vt > S);
    const int mis = __popc((uint32_t)tm ^ DD_AIS_PLUS);
    const int64_t dv = (int64_t)16 * vt - S;
    int64_t sc = lane < DD_AIS_TEMPLATE ? (dv < 0 ? -dv : dv) : 0;
    for (int o = 32; o > 0; o >>= 1) sc += __shfl_xor(sc, o);
    // the raw levels: bit i = 64 j + lane of the burst is bit lane of W[j]; B = the NRZI-decoded bits, 1 where the level repeats
    unsigned long long B[DD_AIS_WORDS + 1];
    unsigned long long carry = (tm >> (DD_AIS_TEMPLATE - 1)) & 1ull;
#pragma unroll
    for (int j = 0; j < DD_AIS_WORDS; ++j) {
        const unsigned long long W = __ballot(16 * value(DD_AIS_TEMPLATE + 64 * j + lane) > S);
        B[j] = ~(W ^ ((W << 1) | carry));
        carry = W >> 63;
    }
    B[DD_AIS_WORDS] = 0ull;                                          // bits past the last count as 0: no run goes on there
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j <= DD_AIS_WORDS; ++j) bw[j] = B[j];
    }
    __syncthreads();
    const auto bit = [&](int i) { return (int)((bw[i >> 6] >> (i & 63)) & 1ull); };
    // e = where the first run of six ones starts
    int e = -1;
#pragma unroll
    for (int j = DD_AIS_WORDS - 1; j >= 0; --j) {
        unsigned long long a = B[j];
#pragma unroll
        for (int s = 1; s < 6; ++s) a &= (B[j] >> s) | (B[j + 1] << (64 - s));
        if (a) e = 64 * j + __ffsll((long long)a) - 1;
    }
    int status = DD_AIS_OK, nbits = 0;
    uint32_t rem = 0;
    if (e < 0 || e + 6 >= DD_AIS_BITS) status = DD_AIS_NO_END;
    else if (bit(e + 6)) status = DD_AIS_ABORT;
    else {
        const int nd = e > 0 ? e - 1 : 0;                            // the data's raw bits: those before the end flag's first 0
        if (e >= 6 && bit(e - 2) && bit(e - 3) && bit(e - 4) && bit(e - 5) && bit(e - 6)) status = DD_AIS_STUFFING;
        // K = the data bits that stay: not a 0 behind five 1s
        int pre = 0;                                                 // kept bits before word j
        bool kept[DD_AIS_WORDS];
        int rank[DD_AIS_WORDS];
#pragma unroll
        for (int j = 0; j < DD_AIS_WORDS; ++j) {
            unsigned long long f = ~0ull;
#pragma unroll
            for (int s = 1; s < 6; ++s) f &= (B[j] << s) | (j > 0 ? B[j - 1] >> (64 - s) : 0ull);
            const int lo = 64 * j;
            const unsigned long long region = nd >= lo + 64 ? ~0ull : (nd > lo ? (1ull << (nd - lo)) - 1ull : 0ull);
            const unsigned long long K = ~(~B[j] & f) & region;
            kept[j] = (K >> lane) & 1ull;
            rank[j] = pre + __popcll(K & ((1ull << lane) - 1ull));
            pre += __popcll(K);
        }
        nbits = pre;
        if (status == DD_AIS_OK && (nbits < 40 || (nbits & 7))) status = DD_AIS_LENGTH;
        const bool crc = status == DD_AIS_OK;
#pragma unroll
        for (int j = 0; j < DD_AIS_WORDS; ++j) {
            if (!kept[j]) continue;
            const int p = rank[j];
            const unsigned one = (unsigned)((B[j] >> lane) & 1ull);
            if (one) atomicOr(&ob[p >> 5], 1u << (p & 31));
            if (crc && (one ^ (p < 16 ? 1u : 0u))) rem ^= dd_ais_table.z[nbits - 1 - p];   // (the preset: the first 16 bits inverted)
        }
        for (int o = 32; o > 0; o >>= 1) rem ^= __shfl_xor(rem, o);
        if (crc && rem != 0xF0B8u) status = DD_AIS_CRC;
    }
    __syncthreads();
    if (lane < DD_AIS_FRAME / 4) out[lane] = ob[lane];
    if (lane == 0) {
        mt[0] = status;
        mt[1] = nbits;
        mt[2] = (int)rem;
        mt[3] = mis > DD_AIS_TEMPLATE / 2 ? 1 : 0;
        score[blockIdx.x] = sc;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the C entries
// 0 when a size, the samples per bit, the window or the slack is not served, else 1 with the grid filled
static int dd_ais_grid(int64_t n, double sps, int w, int slack, DDAisGrid* gd) {
    if (n < 0 || n > 0x7FFFFFF0LL || !(sps >= 4.0 && sps <= 16.0) || w < 1 || w > 15 || !(w & 1) || slack < 0 || slack > 11) return 0;
    gd->sps = sps;
    gd->h = w / 2;
    gd->slack = slack;
    const int64_t reach = (int64_t)floor(23.5 * sps) + gd->h + 1;   // samples from a start to past its template's last
    gd->nstart = n >= reach ? n - reach + 1 : 0;
    return 1;
}

extern "C" int dd_ais_candidates(const double* audio, int64_t n, double sps, int w, int slack, int64_t* list, int64_t cap,
                                 int64_t* count_host, void* stream) {
    DDAisGrid gd = {};
    const bool served = cap >= 0 && dd_ais_grid(n, sps, w, slack, &gd);
    hipStream_t s = dd_stream(stream);
    return dd_cand_entry("dd_ais_candidates", served,
                         "dd_ais_candidates: need 0 <= n < 2^31, 4 <= sps <= 16, an odd w from 1 to 15, 0 <= slack <= 11 and cap >= 0", audio, n,
                         gd.nstart, 1, 1u, list, cap, count_host, s, [=](uint8_t* mask, int* bsum, int64_t nb) {
                             hipLaunchKernelGGL(k_ais_preamble, dim3((unsigned)nb), dim3(DD_AIS_TILE), 0, s, audio, n, gd, mask, bsum);
                         });
}

extern "C" int dd_ais_demod(const double* audio, int64_t n, double sps, int w, const int64_t* list, int64_t m, uint8_t* frames,
                            int32_t* meta, int64_t* score, void* stream) {
    DDAisGrid gd;
    DD_REQUIRE(m >= 0 && m <= 0x7FFFFFFFLL && dd_ais_grid(n, sps, w, 0, &gd),
               "dd_ais_demod: need 0 <= n < 2^31, 4 <= sps <= 16, an odd w from 1 to 15 and 0 <= m < 2^31");
    if (n == 0 || m == 0) return DD_OK;
    DD_REQUIRE(audio != nullptr && list != nullptr && frames != nullptr && meta != nullptr && score != nullptr, "dd_ais_demod: null buffer");
    hipLaunchKernelGGL(k_ais_demod, dim3((unsigned)m), dim3(64), 0, dd_stream(stream), audio, n, gd, list, frames, meta, score);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
