// Reed-Solomon correction of 255-byte codewords over GF(256), one wave per codeword, and Meteor-M2 LRPT's use of it: the (255,223)
// correction of a frame's four interleaved codewords (DESIGN.md section 4.15 defines that field, that code and the decoder's result;
// lrpt.py restates them in NumPy), included by dd_afsk.hip after dd_lrpt.h.
//
//   dd_rs_wave<T, BETA, ROOT0> -- one wave decodes one codeword of the code whose generator has the 2 T roots beta^ROOT0 ..
//                 beta^(ROOT0 + 2 T - 1), beta = alpha^BETA, over the field whose tables it is handed (T even, 2 T <= 32):
//                 syndromes, the all-zero exit, Berlekamp-Massey with a lane per locator coefficient, a search of the 255 positions
//                 with a lane per position, Forney's value in the same lane, and the corrected word's syndromes before anything is
//                 written.  <16, 11, 112> over 0x187 is the CCSDS code of k_lrpt_rs and of k_fc_rs (dd_funcube_frames.h, shortened);
//                 <12, 1, 0> over 0x11D is the RS41 radiosonde's (dd_rs41.h, section 4.26)
//   k_lrpt_rs  -- one workgroup per frame, one wave per codeword
#pragma once

#define DD_RS_N 255
#define DD_RS_T 16                    // the CCSDS code: t = 16,
#define DD_RS_BETA 11                 // beta = alpha^11,
#define DD_RS_ROOT0 112               // c(beta^j) = 0 for j = 112 .. 143

// GF(256) = GF(2)[x] / poly, alpha = 2: ex[i] = alpha^(i mod 255), so that ex[lg[a] + lg[b]] is a * b and
// ex[lg[a] + 255 - lg[b]] is a / b for non-zero a, b with no reduction of the sum
struct DDRsTables {
    uint8_t ex[512];
    uint8_t lg[256];
};

static constexpr DDRsTables dd_rs_make_tables(int poly) {
    DDRsTables t{};
    int v = 1;
    for (int i = 0; i < 255; ++i) {
        t.ex[i] = (uint8_t)v;
        t.lg[v] = (uint8_t)i;
        v <<= 1;
        if (v & 0x100) v ^= poly;
    }
    for (int i = 255; i < 512; ++i) t.ex[i] = t.ex[i - 255];
    return t;
}

__constant__ DDRsTables dd_rs_tables = dd_rs_make_tables(0x187);        // the CCSDS field
__constant__ DDRsTables dd_rs_tables_11d = dd_rs_make_tables(0x11D);    // the RS41 radiosonde's field

__device__ __forceinline__ int dd_gf_mul(const uint8_t* ex, const uint8_t* lg, int a, int b) {
    const int t = ex[lg[a] + lg[b]];              // lg[0] = 0: the load is in range whatever a and b are
    return (a != 0 && b != 0) ? t : 0;
}

// a * alpha^lb, lb in 0..254
__device__ __forceinline__ int dd_gf_mul_log(const uint8_t* ex, const uint8_t* lg, int a, int lb) {
    const int t = ex[lg[a] + lb];
    return a != 0 ? t : 0;
}

// S_j = c(beta^(ROOT0 + j)) in lane j < 2 T, 0 in the others.  row[0] = 0 and row[1 + i] = byte i, the coefficient of x^(254 - i):
// lane j runs Horner over row[0..127], lane 32 + j over row[128..255], and the first half is worth x^128 more.
template <int T, int BETA, int ROOT0>
__device__ __forceinline__ int dd_rs_syndrome(const uint8_t* ex, const uint8_t* lg, const uint8_t* row, int lane) {
    const int j = lane & 31;
    const int lr = (BETA * (ROOT0 + j)) % 255;
    const uint8_t* src = row + ((lane >> 5) << 7);
    int acc = 0;
    for (int s = 0; s < 128; ++s) acc = dd_gf_mul_log(ex, lg, acc, lr) ^ src[s];
    const int hi = __shfl(acc, j, 64), lo = __shfl(acc, j + 32, 64);
    return lane < 2 * T ? (dd_gf_mul_log(ex, lg, hi, (lr * 128) % 255) ^ lo) : 0;
}

// One wave, one codeword: row[0] = 0 and row[1 + i] = byte i of the wave's own 256-byte LDS row; pos[q] = lane + 64 q are the lane's
// positions, got[q] the bytes received there (0 at position 255) and out[] enters equal to got[].  Returns the bytes changed (0..T)
// with the corrected bytes in out[], or -1 with out[] = got[].  A root at a position below first_valid rejects the word: a shortened
// code has no non-zero byte there.
// The waves of a workgroup share nothing but the read-only tables, and a clean codeword leaves at the all-zero test while a damaged
// one runs on: there is NO workgroup barrier in here, nor in a caller below its staging barrier -- only wave-level operations.
template <int T, int BETA, int ROOT0>
__device__ __forceinline__ int dd_rs_wave(const uint8_t* ex, const uint8_t* lg, uint8_t* row, int lane, const int (&pos)[4],
                                          const int (&got)[4], int (&out)[4], int first_valid) {
    static_assert(T >= 2 && T <= 16 && T % 2 == 0, "a lane per syndrome, and Lambda' starts at the odd term T - 1");
    static_assert(BETA > 0 && BETA < 255 && ROOT0 >= 0 && ROOT0 < 255, "logarithms");
    const int S = dd_rs_syndrome<T, BETA, ROOT0>(ex, lg, row, lane);
    if (__ballot(S != 0) == 0) return 0;
    int nerr = -1;
    // Berlekamp-Massey: lane i holds the coefficients C_i, B_i; the discrepancy and all that follows from it are wave-uniform
    int C = lane == 0, B = C, L = 0, m = 1, b = 1;
#pragma unroll                                                          // all 2 T: n becomes a constant in the lane tests and shuffles
    for (int n = 0; n < 2 * T; ++n) {
        const int sv = __shfl(S, (n - lane) & 63, 64);                  // S_(n-i)
        int d = (lane <= L && lane <= n) ? dd_gf_mul(ex, lg, C, sv) : 0;
        for (int off = 32; off >= 1; off >>= 1) d ^= __shfl_xor(d, off, 64);
        d = __builtin_amdgcn_readfirstlane(d);
        const int Bs = __shfl(B, (lane - m) & 63, 64);                  // B_(i-m)
        if (d == 0) {
            ++m;
            continue;
        }
        const int coef = ex[lg[d] + 255 - lg[b]];
        const int was = C;
        C ^= (lane >= m && lane <= 2 * T) ? dd_gf_mul(ex, lg, coef, Bs) : 0;
        if (2 * L <= n) {
            L = n + 1 - L;
            B = was;
            b = d;
            m = 1;
        } else {
            ++m;
        }
    }
    const unsigned long long nz = __ballot(C != 0 && lane <= 2 * T);        // bit 0 is set: C_0 = 1
    if (L <= T && 63 - __clzll((long long)nz) == L) {
        int lam[T + 1], om[T];
        for (int k = 0; k <= T; ++k) lam[k] = __builtin_amdgcn_readlane(C, k);
        // Omega = S Lambda mod x^(2 T), of degree < L <= T: lane k < T forms Omega_k
        int mine = 0;
        for (int i = 0; i <= T; ++i) {
            const int sv = __shfl(S, (lane - i) & 63, 64);
            mine ^= (i <= lane && lane < T) ? dd_gf_mul(ex, lg, lam[i], sv) : 0;
        }
        for (int k = 0; k < T; ++k) om[k] = __builtin_amdgcn_readlane(mine, k);
        int roots = 0;
        bool bad = false;                                                        // a root with value 0, or below first_valid
        for (int q = 0; q < 4; ++q) {
            const bool in = pos[q] < DD_RS_N;
            const int lX = in ? (BETA * (254 - pos[q])) % 255 : 0;               // position i has locator X = beta^(254 - i)
            const int lx = (255 - lX) % 255, lx2 = (2 * lx) % 255;               // X^-1 and its square
            int v = lam[T];
            for (int k = T - 1; k >= 0; --k) v = dd_gf_mul_log(ex, lg, v, lx) ^ lam[k];
            const bool root = in && v == 0;
            int num = om[T - 1];
            for (int k = T - 2; k >= 0; --k) num = dd_gf_mul_log(ex, lg, num, lx) ^ om[k];
            int den = lam[T - 1];                                                // Lambda'(x): the odd terms, one degree down
            for (int k = T - 3; k >= 1; k -= 2) den = dd_gf_mul_log(ex, lg, den, lx2) ^ lam[k];
            // the value X^(1 - ROOT0) Omega(X^-1) / Lambda'(X^-1), the exponent modulo 255 (144 for the CCSDS code's 112)
            const int e = (num != 0 && den != 0) ? ex[(lg[num] + 255 - lg[den] + (lX * ((256 - ROOT0) % 255)) % 255) % 255] : 0;
            roots += __popcll(__ballot(root));
            bad = bad || __ballot(root && (e == 0 || pos[q] < first_valid)) != 0;
            if (root) out[q] = got[q] ^ e;
        }
        bool good = roots == L && !bad;
        if (good) {
            // the corrected word's syndromes, from the wave's own row: the stores are ordered before the loads within the wave
            for (int q = 0; q < 4; ++q)
                if (pos[q] < DD_RS_N) row[1 + pos[q]] = (uint8_t)out[q];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            good = __ballot(dd_rs_syndrome<T, BETA, ROOT0>(ex, lg, row, lane) != 0) == 0;
        }
        if (good) nerr = L;
    }
    if (nerr < 0)
        for (int q = 0; q < 4; ++q) out[q] = got[q];
    return nerr;
}

// Frame blockIdx.x, codeword w = the wave: body byte i is byte i / 4 of codeword i % 4
__global__ void __launch_bounds__(256) k_lrpt_rs(const uint8_t* __restrict__ bodies, uint8_t* __restrict__ fixed, int* __restrict__ errors) {
    __shared__ uint8_t ex[512];
    __shared__ uint8_t lg[256];
    __shared__ uint8_t cw[4][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t f = blockIdx.x;
    ex[tid] = dd_rs_tables.ex[tid];
    ex[tid + 256] = dd_rs_tables.ex[tid + 256];
    lg[tid] = dd_rs_tables.lg[tid];
    for (int i = tid; i < DD_LRPT_BODY; i += 256) cw[i & 3][1 + (i >> 2)] = bodies[f * DD_LRPT_BODY + i];
    if (tid < 4) cw[tid][0] = 0;
    __syncthreads();

    uint8_t* row = cw[w];
    int pos[4], got[4], out[4];
    for (int q = 0; q < 4; ++q) {
        pos[q] = lane + 64 * q;
        got[q] = pos[q] < DD_RS_N ? row[1 + pos[q]] : 0;
        out[q] = got[q];
    }
    const int nerr = dd_rs_wave<DD_RS_T, DD_RS_BETA, DD_RS_ROOT0>(ex, lg, row, lane, pos, got, out, 0);
    uint8_t* dst = fixed + f * DD_LRPT_BODY + w;
    for (int q = 0; q < 4; ++q)
        if (pos[q] < DD_RS_N) dst[4 * pos[q]] = (uint8_t)out[q];
    if (lane == 0) errors[4 * f + w] = nerr;
}

extern "C" int dd_lrpt_rs(const uint8_t* bodies, int64_t nframes, uint8_t* fixed, int32_t* errors, void* stream) {
    DD_REQUIRE(nframes >= 0 && nframes <= 0x7fffffff, "dd_lrpt_rs: sizes");
    if (nframes == 0) return DD_OK;
    DD_REQUIRE(bodies != nullptr && fixed != nullptr && errors != nullptr, "dd_lrpt_rs: null buffer");
    hipLaunchKernelGGL(k_lrpt_rs, dim3((unsigned)nframes), dim3(256), 0, dd_stream(stream), bodies, fixed, errors);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
