// Vaisala RS41 radiosonde telemetry, 2-GFSK at 4800 baud (beyond the reference; DESIGN.md section 4.26 defines every stage, rs41.py
// restates each kernel in NumPy), included by dd_afsk.hip after dd_candidates.h, whose quantiser, positions, LDS prefix sum, tail, list
// kernel and driver it uses, and after dd_lrpt_rs.h, whose wave decodes the two RS(255,231) codewords.  The audio is the FM
// discriminator's float64 output in radians per sample; everything behind the quantiser is integer, so sums in any order equal the
// restatement bit for bit.
//
//   k_rs41_sync       -- a workgroup stages the quantised audio of 256 starts and the reach of 64 bits in LDS and turns it into its
//                        exclusive prefix sum in place (dd_stage_prefix256; a window's sum is below 2^27, so differences are exact);
//                        one thread per start decides the 64 bits of the header against the midpoint of its two classes' means, two
//                        LDS reads per bit; a mask byte per sample, a count per workgroup
//   k_cand_list       -- (dd_candidates.h) the masks' pass bits as an ordered candidate list below the capacity
//   k_rs41_frame      -- one wave per listed start: the header's midpoint and polarity, 40 or 65 ballots of 8 bytes each, the
//                        whitening mask, the length from byte 56, the two codewords through dd_rs_wave<12, 1, 0>
//   k_rs41_rs_words   -- (a diagnostic) one wave per 255-byte word through dd_rs_wave<12, 1, 0>
#pragma once

#define DD_RS41_TILE 256              // starts per workgroup (mirrored by rs41.TILE)
#define DD_RS41_W_MAX 39              // samples summed per bit value at most: the odd number nearest 0.6 * 64
#define DD_RS41_SLACK_MAX 11          // the header slid into the preamble is 24 or more places from itself and its inverse: 11 + 11 < 24
#define DD_RS41_HDR 0xF812962211CAB610ull   // the header on the air, first-sent bit k in bit k: 25 ones, 39 zeros
#define DD_RS41_ONES 25
#define DD_RS41_ZEROS 39
#define DD_RS41_STD 320               // bytes of a standard frame
#define DD_RS41_EXT 518               // bytes of an extended frame
#define DD_RS41_TYPE 56               // the frame type's byte: 0x0F standard, 0xF0 extended
#define DD_RS41_T 12                  // RS(255,231) over 0x11D, roots alpha^0 .. alpha^23
#define DD_RS41_META 6

static_assert(DD_RS41_TILE + 63 * 64 + 32 + DD_RS41_W_MAX + 2 <= DD_CAND_SPAN, "a tile's span fits the LDS array");

enum { DD_RS41_OK = 0, DD_RS41_OUTSIDE = 1 };

struct DDRs41Grid {
    double sps;                       // samples per bit
    int h, slack;                     // a bit value sums 2 h + 1 samples; header places that may differ
    int span;                         // prefix entries of a tile: 256 + floor(63.5 sps) + 2 h + 2
    int64_t nstart;                   // starts whose header ends inside the audio
};

__constant__ const uint8_t dd_rs41_mask[64] = {
    0x96, 0x83, 0x3E, 0x51, 0xB1, 0x49, 0x08, 0x98, 0x32, 0x05, 0x59, 0x0E, 0xF9, 0x44, 0xC6, 0x26, 0x21, 0x60, 0xC2, 0xEA, 0x79, 0x5D,
    0x6D, 0xA1, 0x54, 0x69, 0x47, 0x0C, 0xDC, 0xE8, 0x5C, 0xF1, 0xF7, 0x76, 0x82, 0x7F, 0x07, 0x99, 0xA2, 0x2C, 0x93, 0x7C, 0x30, 0x63,
    0xF5, 0x10, 0x2E, 0x61, 0xD0, 0xBC, 0xB4, 0xB6, 0x06, 0xAA, 0xF4, 0x23, 0x78, 0x6E, 0x3B, 0xAE, 0xBF, 0x7B, 0x4C, 0xC1};

// The header's 64 values v[k] -> the mask bits.  With S1 the sum over the 25 one-places and S0 over the 39 zero-places, the midpoint
// of the two classes' means is (39 S1 + 25 S0) / (2 * 25 * 39): place k is high when 1950 v[k] lies strictly above 39 S1 + 25 S0 and
// low when strictly below.  Polarity 0 reads high as 1; polarity 1 is the same test of the negated audio, which reads low as 1.
__global__ void __launch_bounds__(DD_RS41_TILE) k_rs41_sync(const double* __restrict__ x, int64_t n, const DDRs41Grid gd,
                                                            uint8_t* __restrict__ mask, int* __restrict__ bsum) {
    __shared__ uint32_t ps[DD_CAND_SPAN];            // first q, then ps[j] = the sum of q over samples first .. first + j - 1 (mod 2^32)
    __shared__ int sh[256];
    __shared__ uint32_t tops[4];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * DD_RS41_TILE;
    const int64_t first = base - gd.h;               // the tile's first sample; 0 outside the audio
    dd_stage_prefix256([&](int64_t i) { return dd_fm_q(x[i]); }, n, first, gd.span, ps, tops);
    const int64_t t = base + tid;
    uint32_t m = 0;
    if (t < gd.nstart) {
        int v[64];
        int64_t S1 = 0, S0 = 0;
#pragma unroll
        for (int k = 0; k < 64; ++k) {
            const int at = (int)(dd_bit_mid(t, k, gd.sps) - first);      // h <= at, at + h + 1 < span (a rounding of the sum included)
            v[k] = (int)(ps[at + gd.h + 1] - ps[at - gd.h]);
            if ((DD_RS41_HDR >> k) & 1ull) S1 += v[k];
            else S0 += v[k];
        }
        const int64_t mid = DD_RS41_ZEROS * S1 + DD_RS41_ONES * S0;
        unsigned long long hi = 0, lo = 0;
#pragma unroll
        for (int k = 0; k < 64; ++k) {
            const int64_t c = (int64_t)(2 * DD_RS41_ONES * DD_RS41_ZEROS) * v[k];
            hi |= c > mid ? 1ull << k : 0ull;
            lo |= c < mid ? 1ull << k : 0ull;
        }
        m = __popcll(hi ^ DD_RS41_HDR) <= gd.slack ? 1u : (__popcll(lo ^ DD_RS41_HDR) <= gd.slack ? 3u : 0u);
    }
    dd_cand_tail(mask, t, n, m, (int)(m & 1u), sh, bsum);
}

// the wave's LDS stores before, its LDS loads behind: one wave is the whole workgroup, so no barrier is needed (dd_rs_wave's rule)
__device__ __forceinline__ void dd_rs41_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// fixed[518 c]: the frame de-whitened and corrected, zero beyond its length; recv[518 c]: de-whitened as received; meta[6 c] = status,
// polarity, length (320 or 518), the header's wrong places, the bytes changed in codeword 0 and in codeword 1 (-1: not decodable).  A
// start whose standard frame does not fit the audio gives DD_RS41_OUTSIDE and zeros.
__global__ void __launch_bounds__(64) k_rs41_frame(const double* __restrict__ x, int64_t n, const DDRs41Grid gd,
                                                   const int64_t* __restrict__ list, uint8_t* __restrict__ fixed, uint8_t* __restrict__ recv,
                                                   int* __restrict__ meta) {
    __shared__ uint8_t ex[512];
    __shared__ uint8_t lg[256];
    __shared__ uint8_t cw[2][256];
    __shared__ uint8_t rx[8 * 65];                   // the frame as received, de-whitened; 65 ballots of 8 bytes
    __shared__ uint8_t fx[8 * 65];                   // the frame corrected
    const int lane = threadIdx.x;
    const int64_t t = list[blockIdx.x];
    uint8_t* fo = fixed + (int64_t)blockIdx.x * DD_RS41_EXT;
    uint8_t* ro = recv + (int64_t)blockIdx.x * DD_RS41_EXT;
    int* mt = meta + (int64_t)blockIdx.x * DD_RS41_META;
    const auto fits = [&](int bytes) { return dd_bit_mid(t, 8 * bytes - 1, gd.sps) + gd.h < n; };
    if (t < 0 || t >= n || !fits(DD_RS41_STD)) {                          // (uniform over the wave)
        for (int i = lane; i < DD_RS41_EXT; i += 64) fo[i] = ro[i] = 0;
        if (lane < DD_RS41_META) mt[lane] = lane == 0 ? DD_RS41_OUTSIDE : 0;
        return;
    }
    for (int i = lane; i < 512; i += 64) ex[i] = dd_rs_tables_11d.ex[i];
    for (int i = lane; i < 256; i += 64) lg[i] = dd_rs_tables_11d.lg[i];
    for (int i = lane; i < 8 * 65; i += 64) rx[i] = 0;
    dd_rs41_wave_sync();
    const auto value = [&](int k) { return dd_window_sum(x, n, dd_bit_mid(t, k, gd.sps), gd.h); };
    // the header (a lane per place): the midpoint, the polarity
    const int v0 = value(lane);
    const bool one = (DD_RS41_HDR >> lane) & 1ull;
    int64_t S1 = one ? v0 : 0, S0 = one ? 0 : v0;
    for (int o = 32; o > 0; o >>= 1) {
        S1 += __shfl_xor(S1, o);
        S0 += __shfl_xor(S0, o);
    }
    const int64_t mid = DD_RS41_ZEROS * S1 + DD_RS41_ONES * S0;
    const int64_t c0 = (int64_t)(2 * DD_RS41_ONES * DD_RS41_ZEROS) * v0;
    const int mis0 = __popcll(__ballot(c0 > mid) ^ DD_RS41_HDR), mis1 = __popcll(__ballot(c0 < mid) ^ DD_RS41_HDR);
    const bool inv = mis1 < mis0;
    // bit 64 j + lane of the frame is lane `lane` of ballot j: byte 8 j + i is bits 8 i .. 8 i + 7 of the ballot, the first-sent in bit 0
    int bytes = DD_RS41_STD;
    for (int j = 0; 8 * j < bytes; ++j) {
        const int b = 64 * j + lane;
        int64_t c = c0;
        if (j > 0) c = b < 8 * bytes ? (int64_t)(2 * DD_RS41_ONES * DD_RS41_ZEROS) * value(b) : mid;
        const unsigned long long word = __ballot(inv ? c < mid : c > mid);
        if (lane < 8 && 8 * j + lane < bytes) rx[8 * j + lane] = (uint8_t)(word >> (8 * lane)) ^ dd_rs41_mask[(8 * j + lane) & 63];
        if (8 * j == DD_RS41_TYPE) {                                      // the length: the nearer of 0x0F and 0xF0, a tie is standard
            const uint32_t ty = ((uint32_t)word & 0xFFu) ^ dd_rs41_mask[DD_RS41_TYPE];
            if (__popc(ty ^ 0xF0u) < __popc(ty ^ 0x0Fu) && fits(DD_RS41_EXT)) bytes = DD_RS41_EXT;
        }
    }
    dd_rs41_wave_sync();
    // codeword j as dd_rs_wave wants it: position i holds c_(254 - i); c_p = frame[8 + 24 j + p] below 24, frame[56 + 2 (p - 24) + j]
    // from there on while the frame lasts, 0 behind it
    const int nmsg = (bytes - DD_RS41_TYPE) / 2;
    const int first_valid = DD_RS_N - 2 * DD_RS41_T - nmsg;
    const auto where = [&](int j, int i) {                                // the frame's byte of codeword j's position i, -1: none
        const int p = 254 - i;
        return p < 2 * DD_RS41_T ? 8 + 2 * DD_RS41_T * j + p : (p - 2 * DD_RS41_T < nmsg ? DD_RS41_TYPE + 2 * (p - 2 * DD_RS41_T) + j : -1);
    };
    for (int i = lane; i < 8 * 65; i += 64) fx[i] = rx[i];
    for (int j = 0; j < 2; ++j)
        for (int q = 0; q < 4; ++q) {
            const int i = lane + 64 * q, at = i < DD_RS_N ? where(j, i) : -1;
            if (i < DD_RS_N) cw[j][1 + i] = at >= 0 ? rx[at] : 0;
            else cw[j][0] = 0;
        }
    dd_rs41_wave_sync();
    int nerr[2];
    for (int j = 0; j < 2; ++j) {
        int pos[4], got[4], out[4];
        for (int q = 0; q < 4; ++q) {
            pos[q] = lane + 64 * q;
            got[q] = pos[q] < DD_RS_N ? cw[j][1 + pos[q]] : 0;
            out[q] = got[q];
        }
        nerr[j] = dd_rs_wave<DD_RS41_T, 1, 0>(ex, lg, cw[j], lane, pos, got, out, first_valid);
        for (int q = 0; q < 4; ++q) {
            const int at = pos[q] < DD_RS_N ? where(j, pos[q]) : -1;
            if (at >= 0) fx[at] = (uint8_t)out[q];
        }
    }
    dd_rs41_wave_sync();
    for (int i = lane; i < DD_RS41_EXT; i += 64) {
        fo[i] = fx[i];
        ro[i] = rx[i];
    }
    if (lane == 0) {
        mt[0] = DD_RS41_OK;
        mt[1] = inv ? 1 : 0;
        mt[2] = bytes;
        mt[3] = inv ? mis1 : mis0;
        mt[4] = nerr[0];
        mt[5] = nerr[1];
    }
}

// word blockIdx.x of m: fixed = the word corrected or as received, errors = the bytes changed or -1
__global__ void __launch_bounds__(64) k_rs41_rs_words(const uint8_t* __restrict__ words, int first_valid, uint8_t* __restrict__ fixed,
                                                      int* __restrict__ errors) {
    __shared__ uint8_t ex[512];
    __shared__ uint8_t lg[256];
    __shared__ uint8_t row[256];
    const int lane = threadIdx.x;
    const int64_t f = blockIdx.x;
    for (int i = lane; i < 512; i += 64) ex[i] = dd_rs_tables_11d.ex[i];
    for (int i = lane; i < 256; i += 64) lg[i] = dd_rs_tables_11d.lg[i];
    for (int i = lane; i < 256; i += 64) row[i] = i > 0 ? words[f * DD_RS_N + i - 1] : 0;
    dd_rs41_wave_sync();
    int pos[4], got[4], out[4];
    for (int q = 0; q < 4; ++q) {
        pos[q] = lane + 64 * q;
        got[q] = pos[q] < DD_RS_N ? row[1 + pos[q]] : 0;
        out[q] = got[q];
    }
    const int nerr = dd_rs_wave<DD_RS41_T, 1, 0>(ex, lg, row, lane, pos, got, out, first_valid);
    for (int q = 0; q < 4; ++q)
        if (pos[q] < DD_RS_N) fixed[f * DD_RS_N + pos[q]] = (uint8_t)out[q];
    if (lane == 0) errors[f] = nerr;
}

// ---------------------------------------------------------------------------------------------------------------- the C entries
// 0 when a size, the samples per bit, the window or the slack is not served, else 1 with the grid filled
static int dd_rs41_grid(int64_t n, double sps, int w, int slack, DDRs41Grid* gd) {
    if (n < 0 || n > 0x7FFFFFF0LL || !(sps >= 4.0 && sps <= 64.0) || w < 1 || w > DD_RS41_W_MAX || !(w & 1) || slack < 0 ||
        slack > DD_RS41_SLACK_MAX)
        return 0;
    gd->sps = sps;
    gd->h = w / 2;
    gd->slack = slack;
    const int64_t reach = (int64_t)floor(63.5 * sps) + gd->h + 1;       // samples from a start to past its header's last
    gd->span = (int)(DD_RS41_TILE + reach + gd->h + 1);
    gd->nstart = n >= reach ? n - reach + 1 : 0;
    return 1;
}

static auto dd_rs41_sync_launch(const double* audio, int64_t n, const DDRs41Grid& gd, hipStream_t s) {
    return [=](uint8_t* mask, int* bsum, int64_t nb) {
        hipLaunchKernelGGL(k_rs41_sync, dim3((unsigned)nb), dim3(DD_RS41_TILE), 0, s, audio, n, gd, mask, bsum);
    };
}

extern "C" int dd_rs41_candidates(const double* audio, int64_t n, double sps, int w, int slack, int64_t* list, int64_t cap,
                                  int64_t* count_host, void* stream) {
    DDRs41Grid gd = {};
    const bool served = cap >= 0 && dd_rs41_grid(n, sps, w, slack, &gd);
    hipStream_t s = dd_stream(stream);
    return dd_cand_entry("dd_rs41_candidates", served,
                         "dd_rs41_candidates: need 0 <= n < 2^31, 4 <= sps <= 64, an odd w from 1 to 39, 0 <= slack <= 11 and cap >= 0", audio, n,
                         gd.nstart, 1, 1u, list, cap, count_host, s, dd_rs41_sync_launch(audio, n, gd, s));
}

extern "C" int dd_rs41_frames(const double* audio, int64_t n, double sps, int w, const int64_t* list, int64_t m, uint8_t* fixed,
                              uint8_t* recv, int32_t* meta, void* stream) {
    DDRs41Grid gd;
    DD_REQUIRE(m >= 0 && m <= 0x7FFFFFFFLL && dd_rs41_grid(n, sps, w, 0, &gd),
               "dd_rs41_frames: need 0 <= n < 2^31, 4 <= sps <= 64, an odd w from 1 to 39 and 0 <= m < 2^31");
    if (m == 0) return DD_OK;
    DD_REQUIRE((audio != nullptr || n == 0) && list != nullptr && fixed != nullptr && recv != nullptr && meta != nullptr,
               "dd_rs41_frames: null buffer");                           // (n = 0: every start is outside, and the audio is never read)
    hipLaunchKernelGGL(k_rs41_frame, dim3((unsigned)m), dim3(64), 0, dd_stream(stream), audio, n, gd, list, fixed, recv, meta);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_debug_rs41_masks(const double* audio, int64_t n, double sps, int w, int slack, uint8_t* mask, void* stream) {
    DDRs41Grid gd = {};
    const bool served = dd_rs41_grid(n, sps, w, slack, &gd);
    hipStream_t s = dd_stream(stream);
    return dd_cand_masks_entry("dd_debug_rs41_masks", served,
                               "dd_debug_rs41_masks: need 0 <= n < 2^31, 4 <= sps <= 64, an odd w from 1 to 39 and 0 <= slack <= 11", audio, n,
                               gd.nstart, mask, s, dd_rs41_sync_launch(audio, n, gd, s));
}

extern "C" int dd_debug_rs41_rs(const uint8_t* words, int64_t m, int first_valid, uint8_t* fixed, int32_t* errors, void* stream) {
    DD_REQUIRE(m >= 0 && m <= 0x7FFFFFFFLL && first_valid >= 0 && first_valid <= DD_RS_N,
               "dd_debug_rs41_rs: need 0 <= m < 2^31 and 0 <= first_valid <= 255");
    if (m == 0) return DD_OK;
    DD_REQUIRE(words != nullptr && fixed != nullptr && errors != nullptr, "dd_debug_rs41_rs: null buffer");
    hipLaunchKernelGGL(k_rs41_rs_words, dim3((unsigned)m), dim3(64), 0, dd_stream(stream), words, first_valid, fixed, errors);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
