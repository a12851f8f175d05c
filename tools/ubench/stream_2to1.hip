// What can MI355X stream when a kernel reads 8 B and writes 4 B per sample (the traffic of the C2 chain: complex64 in,
// float32 angle out), independently of the FFT kernel?  (the "0.60 of 8 TB/s" ceiling of DESIGN 4.2c
// rested on k_chain_fft1k's own -DFF_NO_COMPUTE build.)
//
//   out[k] = x[k].re + x[k].im    over N = 2^26 samples, persistent waves, swept over
//     waves per CU            8, 12, 16, 24, 32             (256-thread workgroups, grid = CUs x waves / 4)
//     U  16-byte loads in flight per wave   2, 4, 6, 8     (one "unit" = one wave-wide dwordx4 load = 128 samples)
//     DB                      1: the next U loads are issued before the current U units are summed and stored
//                                (what k_chain_fft1k does: six loads per block fly during its tail), 0: load, wait, store
//     S  store width          4, 8, 16 bytes per lane
//     off                     output pointer 0 or -4 bytes off a 512-byte boundary (a stream START drops one angle, demod_fm.py:43-49)
//     map                     0: one contiguous run of units per wave (dd_fftfir.hip's q_begin..q_end), 1: block-cyclic
//                                (wave w takes pieces w, w + W, ...: the live working set is one moving window),
//                             2: block-cyclic per XCD (workgroup b lives on XCD b % 8: each XCD walks its own eighth)
//     NT                      non-temporal loads and stores
//   plus read-only, write-only and a float4 copy (the guide's 6.29 TB/s figure) as calibration.
//
//   and, last, k_chain_cos1k's own memory side with every choice of it a parameter (k_rows below; `cos1k` runs that table alone).
//
// hipcc --offload-arch=gfx950 -O3 -o bin/stream_2to1 stream_2to1.hip ; ./bin/stream_2to1 [quick | cos1k]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

template <bool NT> __device__ __forceinline__ v4f ld16(const v4f* p) { return NT ? __builtin_nontemporal_load(p) : *p; }
template <bool NT, typename T> __device__ __forceinline__ void st(T* p, T v) { if (NT) __builtin_nontemporal_store(v, p); else *p = v; }

// piece p (U units) -> where its first unit lives, for the three mappings
struct Map {
    long npieces;       // total
    int nwaves;         // total waves of the launch
    int mode;
};
__device__ __forceinline__ void my_range(const Map& m, int gw, int wg, int wave, int nwg, long& first, long& stride, long& count) {
    if (m.mode == 0) {                                   // contiguous run per wave
        const long b = m.npieces * gw / m.nwaves, e = m.npieces * (gw + 1) / m.nwaves;
        first = b; stride = 1; count = e - b;
    } else if (m.mode == 1) {                            // block-cyclic over all waves
        first = gw; stride = m.nwaves; count = (m.npieces - gw + m.nwaves - 1) / m.nwaves;
    } else {                                             // block-cyclic inside the XCD's eighth (workgroup b runs on XCD b % 8)
        const int xcd = wg & 7, wx = (wg >> 3) * 4 + wave, nwx = ((nwg + 7 - xcd) >> 3) * 4;      // waves of this XCD
        const long b = m.npieces * xcd / 8, e = m.npieces * (xcd + 1) / 8;
        first = b + wx; stride = nwx; count = (e - b - wx + nwx - 1) / nwx;
        if (e - b - wx <= 0) count = 0;
    }
}

template <int U, int S>
__device__ __forceinline__ void sum_store(const v4f (&x)[U], float* o, int lane, bool nt) {
    // o = the piece's first output
    if (S == 4) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // (two dword stores of 256 contiguous bytes each: what a 4-byte-per-lane layout would issue)
            if (nt) { __builtin_nontemporal_store(x[u].x + x[u].y, o + 128 * u + lane); __builtin_nontemporal_store(x[u].z + x[u].w, o + 128 * u + 64 + lane); }
            else { o[128 * u + lane] = x[u].x + x[u].y; o[128 * u + 64 + lane] = x[u].z + x[u].w; }
        }
    } else if (S == 8) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const v2f v = {x[u].x + x[u].y, x[u].z + x[u].w};
            if (nt) __builtin_nontemporal_store(v, reinterpret_cast<v2f*>(o + 128 * u + 2 * lane));
            else *reinterpret_cast<v2f*>(o + 128 * u + 2 * lane) = v;
        }
    } else {
#pragma unroll
        for (int u = 0; u + 1 < U; u += 2) {
            const v4f v = {x[u].x + x[u].y, x[u].z + x[u].w, x[u + 1].x + x[u + 1].y, x[u + 1].z + x[u + 1].w};
            if (nt) __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(o + 128 * u + 4 * lane));
            else *reinterpret_cast<v4f*>(o + 128 * u + 4 * lane) = v;
        }
    }
}

// S == 0: read-only (sums kept, stored never)
template <int U, int S, bool DB, bool NT>
__global__ void __launch_bounds__(256) k_s21(const v4f* __restrict__ in, float* __restrict__ out, Map m) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * 4 + wave;
    long first, stride, count;
    my_range(m, gw, blockIdx.x, wave, gridDim.x, first, stride, count);
    if (count <= 0) return;
    v4f a[U], b[U];
    float acc = 0.f;
    if (DB) {
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = ld16<NT>(in + (first * U + u) * 64 + lane);
    }
    for (long i = 0; i < count; ++i) {
        const long p = first + i * stride;
        if (DB) {
            const long pn = (i + 1 < count) ? p + stride : p;          // (the last one re-reads itself: no branch)
#pragma unroll
            for (int u = 0; u < U; ++u) b[u] = ld16<NT>(in + (pn * U + u) * 64 + lane);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) a[u] = ld16<NT>(in + (p * U + u) * 64 + lane);
        }
        if (S == 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) acc += a[u].x + a[u].y + a[u].z + a[u].w;
        } else {
            sum_store<U, S == 0 ? 8 : S>(a, out + p * U * 128, lane, NT);
        }
        if (DB) {
#pragma unroll
            for (int u = 0; u < U; ++u) a[u] = b[u];
        }
    }
    if (S == 0 && acc == 123.456f) out[0] = acc;
}

// write-only: 4 B per sample, S bytes per lane
template <int S>
__global__ void __launch_bounds__(256) k_wr(float* __restrict__ out, Map m) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * 4 + wave;
    long first, stride, count;
    my_range(m, gw, blockIdx.x, wave, gridDim.x, first, stride, count);
    for (long i = 0; i < count; ++i) {
        float* o = out + (first + i * stride) * 4 * 128;          // pieces of 4 units
        if (S == 8) {
#pragma unroll
            for (int u = 0; u < 4; ++u) *reinterpret_cast<v2f*>(o + 128 * u + 2 * lane) = (v2f){(float)i, (float)lane};
        } else {
#pragma unroll
            for (int u = 0; u < 4; u += 2) *reinterpret_cast<v4f*>(o + 128 * u + 4 * lane) = (v4f){(float)i, (float)lane, 1.f, 2.f};
        }
    }
}

// float4 copy (the guide's calibration: 6.29 TB/s), grid-stride, U loads then U stores
template <int U>
__global__ void __launch_bounds__(256) k_copy(const v4f* __restrict__ in, v4f* __restrict__ out, long n4) {
    const long nthreads = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += nthreads * U) {
        v4f v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { const long j = i + u * nthreads; v[u] = j < n4 ? in[j] : (v4f){0, 0, 0, 0}; }
#pragma unroll
        for (int u = 0; u < U; ++u) { const long j = i + u * nthreads; if (j < n4) out[j] = v[u]; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_chain_cos1k's memory side (dd_cosfir.hip), every choice of it a parameter: pieces of 8 units (one row: 1024 samples, 8 KB in, 4 KB
// out; a lane's eight 16-byte loads sit 1 KB apart, its four 16-byte stores too) in runs of R pieces.
//   map 3   run j goes to wave j mod nwaves (the kernel's dealing: every XCD touches the whole moving window)
//   map 4   the same runs, the waves counted XCD by XCD (workgroup b on XCD b mod 8): in each pass over the waves every XCD owns a
//           contiguous eighth of the window
//   LP / SP cache policy of the loads / the stores: the raw buffer builtins' aux word (0 plain, 2 nt, 16 sc1, 17 sc0 sc1, 18 nt sc1);
//           plain and nt go through a pointer, the others through a buffer resource over the piece (base wave-uniform, offset 32-bit)
//   DEFER   a piece's stores are issued after the NEXT piece's loads (c1_row: c1_flush_angles behind the prefetch), from registers
//           that were filled a piece earlier, so they wait for no load
//   PRIME   before a run the last 2 KB of the piece in front of it are read again (c1_prime_issue)
// 8 waves per CU (2 workgroups of 4), the next piece's loads always in flight during the current one's sums: the kernel's shape.
enum { P_PLAIN = 0, P_NT = 2, P_SC1 = 16, P_SC0SC1 = 17, P_NTSC1 = 18 };
typedef unsigned v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ const char* uni(const char* p) {
    const unsigned long long a = (unsigned long long)p;
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32)), lo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)a);
    return (const char*)(((unsigned long long)hi << 32) | lo);          // (the builtin returns int: unsigned before it widens)
}
template <int P> __device__ __forceinline__ v4f ldp(const char* row, unsigned bytes, unsigned off) {
    if (P == P_PLAIN) return *reinterpret_cast<const v4f*>(row + off);
    if (P == P_NT) return __builtin_nontemporal_load(reinterpret_cast<const v4f*>(row + off));
    return __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(__builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(uni(row)), 0, bytes, 0x00020000), off, 0, P));
}
template <int P> __device__ __forceinline__ void stp(char* row, unsigned bytes, unsigned off, v4f v) {
    if (P == P_PLAIN) *reinterpret_cast<v4f*>(row + off) = v;
    else if (P == P_NT) __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(row + off));
    else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(uni(row)), 0, bytes, 0x00020000), off, 0, P);
}
__device__ __forceinline__ int deal_pos(int b, int grid, int map) {          // dd_cosfir.hip: c1_deal_pos
    if (map != 4) return b;
    const int x = b & 7, rem = grid & 7;
    return x * (grid >> 3) + (x < rem ? x : rem) + (b >> 3);
}
template <int LP, int SP, bool DEFER, bool PRIME>
__global__ void __launch_bounds__(256, 2) k_rows(const char* __restrict__ in, char* __restrict__ out, int npieces, int R, int map) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = gridDim.x * 4, gw = deal_pos(blockIdx.x, gridDim.x, map) * 4 + wave;
    const int nruns = (npieces + R - 1) / R;
    const unsigned lo = 16 * lane;
    for (int run = gw; run < nruns; run += nwaves) {
        const int q0 = run * R, q1 = q0 + R < npieces ? q0 + R : npieces;
        v4f a[8], b[8], pend[4], xp[2];
        float keep = 0.f;
        if (PRIME && q0 > 0) {
            const char* prow = in + (long)(q0 - 1) * 8192;
            xp[0] = ldp<LP>(prow, 8192, lo + 1024 * 6);
            xp[1] = ldp<LP>(prow, 8192, lo + 1024 * 7);
        } else xp[0] = xp[1] = (v4f){0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = ldp<LP>(in + (long)q0 * 8192, 8192, lo + 1024 * j);
        if (PRIME) keep = xp[0].x + xp[0].y + xp[0].z + xp[0].w + xp[1].x + xp[1].y + xp[1].z + xp[1].w;
        bool have = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = a[j];
        for (int q = q0; q < q1; ++q) {
            if (q + 1 < q1) {                                           // (wave-uniform)
#pragma unroll
                for (int j = 0; j < 8; ++j) b[j] = ldp<LP>(in + (long)(q + 1) * 8192, 8192, lo + 1024 * j);
            }
            if (DEFER && have) {
#pragma unroll
                for (int g = 0; g < 4; ++g) stp<SP>(out + (long)(q - 1) * 4096, 4096, lo + 1024 * g, pend[g]);
            }
            v4f s[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) s[g] = (v4f){a[2 * g].x + a[2 * g].y, a[2 * g].z + a[2 * g].w, a[2 * g + 1].x + a[2 * g + 1].y, a[2 * g + 1].z + a[2 * g + 1].w + keep};
            if (DEFER) {
#pragma unroll
                for (int g = 0; g < 4; ++g) pend[g] = s[g];
                have = true;
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) stp<SP>(out + (long)q * 4096, 4096, lo + 1024 * g, s[g]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = b[j];
        }
        if (DEFER && have) {
#pragma unroll
            for (int g = 0; g < 4; ++g) stp<SP>(out + (long)(q1 - 1) * 4096, 4096, lo + 1024 * g, pend[g]);
        }
    }
}

static hipEvent_t e0, e1;
template <typename F>
static float time_ms(F launch, int warm, int reps) {
    for (int i = 0; i < warm; ++i) launch();
    CK(hipEventRecord(e0));
    for (int i = 0; i < reps; ++i) launch();
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    return ms / reps;
}

struct Row { int U, S, DB, NT, off, map; float tbs[5]; int waves[5]; };
static const int WAVES[5] = {8, 12, 16, 24, 32};
static int g_cus = 256;
static const long N = 1L << 26;
static v4f* d_in; static float* d_out;
static int g_warm = 10, g_reps = 40;

template <int U, int S, bool DB, bool NT>
static void run_cfg(std::vector<Row>& rows, int off, int map) {
    Row r; r.U = U; r.S = S; r.DB = DB; r.NT = NT; r.off = off; r.map = map;
    int maxwg = 0;
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&maxwg, k_s21<U, S, DB, NT>, 256, 0));
    const long units = N / 128, npieces = (units + U - 1) / U;
    for (int w = 0; w < 5; ++w) {
        int wgs = WAVES[w] / 4;
        if (wgs > maxwg) wgs = maxwg;               // (register-limited: reported with the waves it really runs)
        r.waves[w] = wgs * 4;
        if (w > 0 && r.waves[w] == r.waves[w - 1]) { r.tbs[w] = r.tbs[w - 1]; continue; }
        Map m; m.npieces = npieces; m.nwaves = g_cus * wgs * 4; m.mode = map;
        float* o = d_out + 128 - off;
        const float ms = time_ms([&] { hipLaunchKernelGGL((k_s21<U, S, DB, NT>), dim3(g_cus * wgs), dim3(256), 0, 0, d_in, o, m); }, g_warm, g_reps);
        const double bytes = (S == 0 ? 8.0 : 12.0) * (double)N;
        r.tbs[w] = (float)(bytes / (ms * 1e-3) / 1e12);
    }
    rows.push_back(r);
}

template <int U, int S>
static void run_db_nt(std::vector<Row>& rows, int off, int map, bool nt_too) {
    run_cfg<U, S, true, false>(rows, off, map);
    run_cfg<U, S, false, false>(rows, off, map);
    if (nt_too) { run_cfg<U, S, true, true>(rows, off, map); }
}
template <int S>
static void run_u(std::vector<Row>& rows, int off, int map, bool nt_too) {
    run_db_nt<2, S>(rows, off, map, nt_too);
    run_db_nt<4, S>(rows, off, map, nt_too);
    run_db_nt<6, S>(rows, off, map, nt_too);
    run_db_nt<8, S>(rows, off, map, nt_too);
}

static void print_rows(const std::vector<Row>& rows, size_t from) {
    for (size_t i = from; i < rows.size(); ++i) {
        const Row& r = rows[i];
        printf("map %d off %2d S %2d U %d DB %d NT %d |", r.map, -4 * r.off, r.S, r.U, r.DB, r.NT);
        for (int w = 0; w < 5; ++w) printf(" %5.2f%s", r.tbs[w], r.waves[w] == WAVES[w] ? " " : "*");
        printf("\n");
    }
    fflush(stdout);
}

// ---- k_chain_cos1k's memory side: every (LP, SP, DEFER, PRIME, map) against R
typedef void (*rows_fn)(const char*, char*, int, int, int);
struct RowsK { int lp, sp, defer, prime; rows_fn f; };
template <int LP, int SP> static void add_rows(std::vector<RowsK>& v) {
    v.push_back({LP, SP, 0, 0, k_rows<LP, SP, false, false>});
    v.push_back({LP, SP, 0, 1, k_rows<LP, SP, false, true>});
    v.push_back({LP, SP, 1, 0, k_rows<LP, SP, true, false>});
    v.push_back({LP, SP, 1, 1, k_rows<LP, SP, true, true>});
}
template <int LP> static void add_rows_lp(std::vector<RowsK>& v) {
    add_rows<LP, P_PLAIN>(v); add_rows<LP, P_NT>(v); add_rows<LP, P_SC1>(v); add_rows<LP, P_SC0SC1>(v); add_rows<LP, P_NTSC1>(v);
}
static const char* pol_name(int p) { return p == P_PLAIN ? "plain" : p == P_NT ? "nt" : p == P_SC1 ? "sc1" : p == P_SC0SC1 ? "sc0sc1" : "ntsc1"; }
static const int RS[6] = {1, 2, 4, 8, 12, 16};
static float rows_tbs(const RowsK& k, int map, int R) {
    const int npieces = (int)(N / 1024);
    float ms[3];
    for (int t = 0; t < 3; ++t)
        ms[t] = time_ms([&] { hipLaunchKernelGGL(k.f, dim3(g_cus * 2), dim3(256), 0, 0, (const char*)d_in, (char*)d_out, npieces, R, map); }, t ? 0 : g_warm, g_reps);
    std::sort(ms, ms + 3);
    return (float)(12.0 * (double)N / (ms[1] * 1e-3) / 1e12);
}
static void cos1k_table() {
    std::vector<RowsK> ks;
    add_rows_lp<P_PLAIN>(ks); add_rows_lp<P_NT>(ks); add_rows_lp<P_SC1>(ks);
    printf("# k_chain_cos1k's memory side: rows of 8 units in runs of R rows, 8 waves per CU, TB/s of the 12 B/sample (median of 3 x %d launches;\n", g_reps);
    printf("# the prime's 2 KB per run are not counted); columns R = 1 2 4 8 12 16\n");
    float now = 0.f;
    struct Best { float v; const RowsK* k; int map, R; } best = {0.f, nullptr, 0, 0};
    std::vector<float> all(ks.size() * 2 * 6);
    for (int map = 3; map <= 4; ++map)
        for (size_t i = 0; i < ks.size(); ++i) {
            const RowsK& k = ks[i];
            printf("map %d loads %-5s stores %-6s defer %d prime %d |", map, pol_name(k.lp), pol_name(k.sp), k.defer, k.prime);
            for (int r = 0; r < 6; ++r) {
                const float v = rows_tbs(k, map, RS[r]);
                all[(i * 2 + (map - 3)) * 6 + r] = v;
                printf(" %5.2f", v);
                if (v > best.v) best = {v, &k, map, RS[r]};
                if (map == 3 && RS[r] == 8 && k.lp == P_NT && k.sp == P_PLAIN && k.defer && k.prime) now = v;
            }
            printf("\n");
            fflush(stdout);
        }
    printf("# the kernel's shape today (map 3, R 8, nt loads, deferred plain stores, prime): %.2f TB/s = %.3f of 8; 7.1 TB/s - that = %.2f\n", now, now / 8.0, 7.1 - now);
    printf("# best of the table: %.2f TB/s: map %d R %d loads %s stores %s defer %d prime %d\n", best.v, best.map, best.R, pol_name(best.k->lp),
           pol_name(best.k->sp), best.k->defer, best.k->prime);
    printf("# one change at a time from today's shape:\n");
    for (size_t i = 0; i < ks.size(); ++i)
        for (int map = 3; map <= 4; ++map)
            for (int r = 0; r < 6; ++r) {
                const RowsK& k = ks[i];
                const int changes = (map != 3) + (RS[r] != 8) + (k.lp != P_NT) + (k.sp != P_PLAIN) + !k.defer + !k.prime;
                if (changes == 1)
                    printf("#   map %d R %2d loads %-5s stores %-6s defer %d prime %d: %.2f (%+.2f)\n", map, RS[r], pol_name(k.lp), pol_name(k.sp), k.defer, k.prime,
                           all[(i * 2 + (map - 3)) * 6 + r], all[(i * 2 + (map - 3)) * 6 + r] - now);
            }
}

int main(int argc, char** argv) {
    const bool quick = argc > 1 && !strcmp(argv[1], "quick");
    const bool cos1k_only = argc > 1 && !strcmp(argv[1], "cos1k");       // the last table alone
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    g_cus = prop.multiProcessorCount;
    printf("# %s, %d CUs; N = 2^26 samples: 512 MiB complex64 in, 256 MiB float32 out (>> 256 MiB Infinity Cache); TB/s of the 12 B/sample\n", prop.name, g_cus);
    printf("# (8 TB/s spec peak: 0.70 = 5.60, 0.60 = 4.80); columns = waves per CU %d %d %d %d %d (* = register-limited below that)\n", WAVES[0], WAVES[1], WAVES[2], WAVES[3], WAVES[4]);
    CK(hipMalloc(&d_in, N * 8 + (1 << 20)));
    CK(hipMalloc(&d_out, N * 4 + (1 << 20)));
    CK(hipMemset(d_in, 0, N * 8 + (1 << 20)));
    CK(hipMemset(d_out, 0, N * 4 + (1 << 20)));
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    if (quick) { g_warm = 3; g_reps = 10; }
    if (cos1k_only) { g_reps = 20; cos1k_table(); return 0; }

    // ---- calibration: copy, read-only, write-only
    for (int wgs : {2, 4, 8}) {
        const long n4 = N * 8 / 16 / 2;          // 256 MiB -> 256 MiB
        float ms = time_ms([&] { hipLaunchKernelGGL((k_copy<4>), dim3(g_cus * wgs), dim3(256), 0, 0, d_in, reinterpret_cast<v4f*>(d_out), n4); }, g_warm, g_reps);
        printf("copy float4 256 MiB -> 256 MiB, %2d waves/CU, 4 loads then 4 stores: %.4f ms = %.2f TB/s (read + written)\n", wgs * 4, ms, 2.0 * n4 * 16 / (ms * 1e-3) / 1e12);
    }
    {
        std::vector<Row> rows;
        printf("# read-only (8 B/sample, 512 MiB), TB/s of the bytes read\n");
        for (int map = 0; map < 3; ++map) { run_cfg<4, 0, true, false>(rows, 0, map); run_cfg<8, 0, true, false>(rows, 0, map); run_cfg<8, 0, false, false>(rows, 0, map); }
        print_rows(rows, 0);
        printf("# write-only (4 B/sample, 256 MiB), TB/s of the bytes written; 8 then 16 bytes per lane; maps 0 1 2; waves/CU 8 16 32\n");
        for (int S : {8, 16})
            for (int map = 0; map < 3; ++map) {
                printf("write-only S %2d map %d |", S, map);
                for (int wgs : {2, 4, 8}) {
                    Map m; m.npieces = N / 128 / 4; m.nwaves = g_cus * wgs * 4; m.mode = map;
                    float ms = S == 8 ? time_ms([&] { hipLaunchKernelGGL((k_wr<8>), dim3(g_cus * wgs), dim3(256), 0, 0, d_out, m); }, g_warm, g_reps)
                                      : time_ms([&] { hipLaunchKernelGGL((k_wr<16>), dim3(g_cus * wgs), dim3(256), 0, 0, d_out, m); }, g_warm, g_reps);
                    printf(" %5.2f", 4.0 * N / (ms * 1e-3) / 1e12);
                }
                printf("\n");
            }
    }
    // ---- the sweep
    std::vector<Row> rows;
    for (int map = 0; map < 3; ++map)
        for (int off = 0; off < 2; ++off) {
            const size_t from = rows.size();
            const bool nt = !quick;
            run_u<4>(rows, off, map, nt);
            run_u<8>(rows, off, map, nt);
            run_u<16>(rows, off, map, nt);
            print_rows(rows, from);
        }
    // ---- best configurations
    std::vector<std::pair<float, std::pair<int, int>>> best;
    for (size_t i = 0; i < rows.size(); ++i)
        for (int w = 0; w < 5; ++w) best.push_back({rows[i].tbs[w], {(int)i, w}});
    std::sort(best.begin(), best.end(), [](auto& a, auto& b) { return a.first > b.first; });
    printf("# top 12\n");
    for (int k = 0; k < 12 && k < (int)best.size(); ++k) {
        const Row& r = rows[best[k].second.first];
        printf("%.2f TB/s = %.3f of 8 TB/s: map %d off %d S %d U %d DB %d NT %d waves/CU %d\n", best[k].first, best[k].first / 8.0, r.map, -4 * r.off, r.S, r.U, r.DB, r.NT, r.waves[best[k].second.second]);
    }
    // the product kernel's shape: contiguous run per wave, 12 waves/CU, 6 loads ahead, 8-byte stores
    for (const Row& r : rows)
        if (r.map == 0 && r.S == 8 && r.U == 6 && r.DB == 1 && r.NT == 0)
            printf("# k_chain_fft1k's shape (map 0, S 8, U 6, DB 1, 12 waves/CU), off %d: %.2f TB/s\n", -4 * r.off, r.tbs[1]);
    cos1k_table();
    return 0;
}
