// A1: demod_am.demod -- abs(hilbert(x)) per block (demod_am.py:18-29, decode_noaa.py:644-653): dd_am_envelope_f64, and everything about
// Hilbert envelopes that more than one part uses.  In the order of the file:
//   * the block walk's PLAN (DDEnvWalk, envelope_plan): the chunker rule, the route of the full blocks and of the ragged last one, the
//     work areas -- pure host code, which tests/host/envelope_plan_check.cpp compiles alone (DD_ENVELOPE_PLAN_ONLY);
//   * the Hilbert-kernel spectra (closed forms, host transform, ONE walk through the device and host caches: hilbert_spectrum);
//   * the four routes of one group of equal blocks -- own split / own plain (hc_block_envelope), the library's real transform pair
//     (envelope_real_pair) and its zero-padded real convolution (envelope_padded, which the accurate-sync windows' stage shares);
//   * the RUNNER envelope_walk, which dd_am_envelope_f64 (here) and dd_noaa_crude_tail call; dd_noaa_prepare reads the plan only.
// The first of the six parts of dd_audio.hip (one translation unit: the parts share the plan cache, the float64 transform and the
// scratch buffers of dd_audio.hip and are included there, each using only the parts before it).  Internal; not a stand-alone header.
// ---------------------------------------------------------------- the block walk's plan (host only)
static int64_t largest_prime_factor(int64_t n) {
    int64_t best = 1;
    for (int64_t p = 2; p * p <= n; ++p)
        while (n % p == 0) { best = p; n /= p; }
    return n > 1 ? n : best;
}
// cyclic length of dd_hconv_kernels.h for the envelope of a block of N real samples, 0 = not on this route; *split: the even / odd form
static int64_t hc_block_len(int64_t N, bool* split) {
    *split = false;
    if (N < 2) return 0;
    if ((N & 1) == 0 && N - 1 <= ((int64_t)1 << 18)) { *split = true; return N - 1 <= ((int64_t)1 << 17) ? (int64_t)1 << 17 : (int64_t)1 << 18; }
    if (2 * N + 2 <= ((int64_t)1 << 17)) return (int64_t)1 << 17;
    if (2 * N + 2 <= ((int64_t)1 << 18)) return (int64_t)1 << 18;
    return 0;
}
// Route of a group of equal blocks.  Blocks that fit the own float64 transform go through it (a 240 000-sample block by the even / odd
// split of the Hilbert kernel): no FFT-library plan, whose creation costs a process's first call 0.9 s.  The others, and all under
// DD_AM_HILBERT=lib (tools / tests), take the library's real-to-complex / complex-to-real pair -- half the transform work of the complex
// pair -- except a ragged last block whose length has a prime factor above 17 (under lib, 14 100 = 2^2 3 5^2 47 for a minute of audio): the library
// would run Bluestein's algorithm, twenty launches, so it takes the zero-padded cyclic convolution with the Hilbert kernel that the
// accurate-sync windows use, four launches and two power-of-two transforms.
enum DDEnvRoute { DD_ENV_NONE = 0, DD_ENV_OWN_SPLIT, DD_ENV_OWN_PLAIN, DD_ENV_LIB_PAIR, DD_ENV_LIB_PADDED };
struct DDEnvGroup {
    DDEnvRoute route;
    int64_t N, M;                     // block length; cyclic length (0 on DD_ENV_LIB_PAIR)
};
struct DDEnvWalk {
    int64_t block, nfull, batch;      // nfull full blocks of `block` samples, and how many of them one group takes (16; own plain form: 1)
    DDEnvGroup full, last;            // full.route = DD_ENV_NONE without full blocks; last.N = the remainder, 1 .. block
    size_t T_elems, spec_elems, y_elems;      // work areas: complex image T (c128), spectrum (c128), real scratch y (f64)
};
static DDEnvGroup envelope_route(int64_t N, bool own_ok, bool last) {
    bool split = false;
    const int64_t M = own_ok ? hc_block_len(N, &split) : 0;
    if (M) return DDEnvGroup{split ? DD_ENV_OWN_SPLIT : DD_ENV_OWN_PLAIN, N, M};
    if (!(last && N >= 2 && largest_prime_factor(N) > 17)) return DDEnvGroup{DD_ENV_LIB_PAIR, N, 0};
    int64_t Mp = 1;
    while (Mp < 2 * N + 2) Mp <<= 1;
    return DDEnvGroup{DD_ENV_LIB_PADDED, N, Mp};
}
// block list by the chunker rule (decode_noaa.py:644-653 via chunker.py:36-45): full blocks while one more fits strictly inside, then
// the remainder (a full-size last block when n is an exact multiple).  n >= 1, block >= 1.
static DDEnvWalk envelope_plan(int64_t n, int64_t block) {
    static const char* amh_env = getenv("DD_AM_HILBERT");
    const bool own_ok = !(amh_env && !strcmp(amh_env, "lib"));
    DDEnvWalk w = {};
    w.block = block;
    w.nfull = (n - 1) / block;
    w.last = envelope_route(n - w.nfull * block, own_ok, true);
    if (w.nfull) w.full = envelope_route(block, own_ok, false);
    w.batch = w.full.route == DD_ENV_OWN_PLAIN ? 1 : std::min<int64_t>(w.nfull, 16);
    const DDEnvGroup* g[2] = {&w.full, &w.last};
    for (int i = 0; i < 2; ++i) {
        const int64_t jobs = i ? 1 : w.batch, N = g[i]->N, M = g[i]->M;
        size_t T = 0, sp = 0, y = 0;
        if (g[i]->route == DD_ENV_OWN_SPLIT || g[i]->route == DD_ENV_OWN_PLAIN) T = (size_t)(jobs * M);
        if (g[i]->route == DD_ENV_LIB_PAIR) { sp = (size_t)(jobs * (N / 2 + 1)); y = (size_t)(jobs * N); }
        if (g[i]->route == DD_ENV_LIB_PADDED) { sp = (size_t)(M / 2 + 1); y = (size_t)(2 * M); }
        w.T_elems = std::max(w.T_elems, T); w.spec_elems = std::max(w.spec_elems, sp); w.y_elems = std::max(w.y_elems, y);
    }
    return w;
}
#ifndef DD_ENVELOPE_PLAN_ONLY
// ---------------------------------------------------------------- abs(hilbert(x)) as scipy computes it (the accurate-sync windows' "fft" route)
// scipy.signal.hilbert: Xf = fft(x); h[0] = 1, h[1..(N-1)/2 or N/2-1] = 2, h[N/2] = 1 (N even),
// 0 elsewhere; ifft(Xf * h); demod_am takes the magnitude (demod_am.py:29).
// blockIdx.y = block (or window) of the batch
__global__ void __launch_bounds__(256) k_hilbert_mask_b(double2* __restrict__ X, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double h;
    if ((n & 1) == 0) h = (i == 0 || i == n / 2) ? 1.0 : (i < n / 2 ? 2.0 : 0.0);
    else h = (i == 0) ? 1.0 : (i < (n + 1) / 2 ? 2.0 : 0.0);
    double2* p = X + (int64_t)blockIdx.y * n + i;
    *p = make_double2(p->x * h, p->y * h);
}
__global__ void __launch_bounds__(256) k_cplx_abs_b(const double2* __restrict__ in, double* __restrict__ out, int64_t n, double inv_n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double2 v = in[(int64_t)blockIdx.y * n + i];
    out[(int64_t)blockIdx.y * n + i] = hypot(v.x * inv_n, v.y * inv_n);
}

// ---------------------------------------------------------------- the envelope as one real convolution (all sync entry points)
// abs(hilbert(x)) = |x + j (x (*) hh)| where (*) is the length-N
// circular convolution and hh = imag(ifft(h)) the Hilbert kernel of scipy's spectrum mask h (the real part
// of ifft(h) is the unit impulse).  The accurate-sync window length N = 118 151 has a large prime factor, so the library's
// length-N transforms are Bluestein chirp-z: two padded power-of-two transforms each way, complex.  The
// circular convolution needs only outputs [0, N), which a length-M >= 2N-1 cyclic convolution with the kernel
// laid out at offsets -(N-1)..N-1 gives without wrap-around: one real-to-complex and one complex-to-real
// power-of-two transform per window, a quarter of the work.  The kernel spectrum is built once per length
// from the closed form of hh.
__global__ void __launch_bounds__(256) k_spec_mul(double2* __restrict__ S, const double2* __restrict__ HH, int64_t nb) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nb) return;
    double2* p = S + (int64_t)blockIdx.y * nb + k;
    const double2 a = *p, h = HH[k];
    *p = make_double2(a.x * h.x - a.y * h.y, a.x * h.y + a.y * h.x);
}
__global__ void __launch_bounds__(256) k_env_hypot(const double* __restrict__ XR, const double* __restrict__ YR, int64_t M, int64_t n,
                                                   double* __restrict__ env) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    env[(int64_t)blockIdx.y * n + i] = hypot(XR[(int64_t)blockIdx.y * M + i], YR[(int64_t)blockIdx.y * M + i]);
}

// (device, N) -> spectrum of the padded kernel / M.  On the heap, never deleted: nothing is freed at exit
static std::map<std::pair<int, int64_t>, DDDevBuf<double2>>& g_hilb = *new std::map<std::pair<int, int64_t>, DDDevBuf<double2>>();
static std::vector<std::pair<int, int64_t>> g_hilb_order;
// sin(pi num / den) for integers num >= 0, den > 0: the argument is reduced to [0, pi/2] exactly in integers first
static double dd_sinpi_frac(int64_t num, int64_t den) {
    int64_t r = num % (2 * den);
    double sg = 1.0;
    if (r >= den) { r -= den; sg = -1.0; }
    if (2 * r > den) r = den - r;
    return sg * sin(3.14159265358979323846 * (double)r / (double)den);
}

// In-place radix-2 transform of a power-of-two length on the HOST, float64, twiddles from one table (once per Hilbert-kernel
// spectrum: 2^18 points take a few milliseconds).  Round 5: the kernel spectra no longer go through the FFT library -- its first plan of
// a process costs hundreds of milliseconds, and the reference decodes one file per process (main.py:208-270).
static void host_fft_pow2(std::vector<std::complex<double>>& v) {
    // (plain arrays and spelt-out complex arithmetic: std::complex's operator* goes through a NaN-checking library call)
    const size_t n = v.size();
    double* a = reinterpret_cast<double*>(v.data());
    std::vector<double> wr(n / 2), wi(n / 2);
    const double step0 = -6.283185307179586476925286766559 / (double)n;
    // one octant by the library, the rest by symmetry of the unit circle (k -> n/4 - k, then k -> k + n/4)
    const size_t q = n / 4;
    for (size_t k = 0; k <= q / 2 && k < n / 2; ++k) {
        const double c = cos(step0 * (double)k), sn = sin(step0 * (double)k);
        wr[k] = c; wi[k] = sn;
        if (q >= k && q - k < n / 2) { wr[q - k] = -sn; wi[q - k] = -c; }
    }
    for (size_t k = 0; k < q && k + q < n / 2; ++k) { wr[k + q] = wi[k]; wi[k + q] = -wr[k]; }
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(a[2 * i], a[2 * j]); std::swap(a[2 * i + 1], a[2 * j + 1]); }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const size_t half = len / 2, step = n / len;
        for (size_t i = 0; i < n; i += len) {
            double* lo = a + 2 * i;
            double* hi = a + 2 * (i + half);
            for (size_t k = 0; k < half; ++k) {
                const double c = wr[k * step], sn = wi[k * step];
                const double xr = hi[2 * k] * c - hi[2 * k + 1] * sn, xi = hi[2 * k] * sn + hi[2 * k + 1] * c;
                const double ur = lo[2 * k], ui = lo[2 * k + 1];
                lo[2 * k] = ur + xr; lo[2 * k + 1] = ui + xi;
                hi[2 * k] = ur - xr; hi[2 * k + 1] = ui - xi;
            }
        }
    }
}
// the spectrum of a real kernel image of length M (divided by M): the M/2 + 1 bins the library's real transforms multiply, and -- for the
// lengths of dd_hconv_kernels.h -- once more behind them in the order its row pass reads (out[N2 k1 + k2] = bin k1 + 512 k2).  Host part:
// no device call (dd_noaa_prepare runs it while the runtime is still busy with the process's first copy).
static void kernel_spectrum_host(const std::vector<double>& img, int64_t M, std::vector<double2>& h) {
    std::vector<std::complex<double>> v((size_t)M);
    for (int64_t i = 0; i < M; ++i) v[(size_t)i] = std::complex<double>(img[(size_t)i], 0.0);
    host_fft_pow2(v);
    const int64_t nb = M / 2 + 1;
    const bool own = hc_length_ok(M);
    h.resize((size_t)(nb + (own ? M : 0)));
    const double sc = 1.0 / (double)M;
    for (int64_t k = 0; k < nb; ++k) h[(size_t)k] = make_double2(v[(size_t)k].real() * sc, v[(size_t)k].imag() * sc);
    if (own) {
        const int lg = hc_lg(M);
        for (int64_t i = 0; i < M; ++i) {
            const int64_t k = (i >> lg) + DD_HC_N * (i & (((int64_t)1 << lg) - 1));
            h[(size_t)(nb + i)] = make_double2(v[(size_t)k].real() * sc, v[(size_t)k].imag() * sc);
        }
    }
}
// device part: one allocation, one copy
static int kernel_spectrum_put(const std::vector<double2>& h, DDDevBuf<double2>* out, hipStream_t s) {
    DDDevBuf<double2> HH;
    DD_HIP_CHECK(HH.alloc(h.size()));
    hipError_t e = hipMemcpyAsync(HH, h.data(), sizeof(double2) * h.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);                          // (the staging vector dies with the caller)
    if (e != hipSuccess) { dd_set_error("Hilbert kernel spectrum: %s", hipGetErrorString(e)); return DD_ERR_HIP; }
    *out = std::move(HH);
    return DD_OK;
}
// the cache takes the uploaded spectrum over; returns its device address
static double2* hilb_cache_put(std::pair<int, int64_t> key, DDDevBuf<double2>& HH) {
    // (one spectrum per length: up to 8 MB each; a process that walks through recordings of many different lengths keeps the
    // eight most recently built -- the callers hold g_sync_mu and leave nothing in flight when they return (DDSyncOnExit))
    g_hilb_order.push_back(key);
    while (g_hilb_order.size() > 8) {
        auto old = g_hilb.find(g_hilb_order.front());
        if (old != g_hilb.end()) { (void)hipDeviceSynchronize(); g_hilb.erase(old); }      // (dd_am_envelope_f64 returns with its kernels in flight)
        g_hilb_order.erase(g_hilb_order.begin());
    }
    return (g_hilb[key] = std::move(HH)).get();
}
// The spectra on the HOST, kept for the life of the process (at most eight, 3-8 MB each).  Two reasons: dd_noaa_prepare builds them ahead
// without a device call (its thread runs beside the runtime's first copy and the recording's upload; the call that needs one uploads it,
// 0.3 ms), and a pageable staging vector of a megabyte or more must not be FREED after its copy: the runtime pins such a source in place, and
// returning pinned pages to the system (free -> munmap of a large block) stalled the next device operation of the process by 25-40 ms
// (tools/debug/cold_c4_trace.py: the upload of the second spectrum after the first one's vector had died, in the thread that did it or in
// any other).  Own mutex: prepare fills it without g_sync_mu, the other callers hold g_sync_mu.
static std::mutex g_hilb_host_mu;
static std::map<std::pair<int, int64_t>, std::vector<double2>*> g_hilb_host;
static const std::vector<double2>* hilb_host_find(std::pair<int, int64_t> key) {
    std::lock_guard<std::mutex> lk(g_hilb_host_mu);
    auto it = g_hilb_host.find(key);
    return it == g_hilb_host.end() ? nullptr : it->second;
}
static const std::vector<double2>* hilb_host_keep(std::pair<int, int64_t> key, std::vector<double2>& h) {
    std::lock_guard<std::mutex> lk(g_hilb_host_mu);
    auto it = g_hilb_host.find(key);
    if (it != g_hilb_host.end()) return it->second;               // (another thread was first: its copy stays, ours is dropped unused -- never pinned)
    if (g_hilb_host.size() >= 8) return nullptr;                  // (a process walking through many lengths: the ninth and later are not kept)
    std::vector<double2>* p = new std::vector<double2>();
    p->swap(h);
    g_hilb_host[key] = p;
    return p;
}
static int lg_of(int64_t M) {
    int lgM = 0;
    while (((int64_t)1 << lgM) < M) ++lgM;
    return lgM;
}

// hh[n] = imag(ifft(h))[n] = (2/N) sum_{k=1..m} sin(2 pi k n / N), m = the number of doubled bins of scipy's mask
// ((N-1)/2 for odd N, N/2 - 1 for even N) = (2/N) sin(pi m n/N) sin(pi (m+1) n/N) / sin(pi n/N): a closed form, so no
// length-N (Bluestein) plan is ever built for it; accurate to a few 1e-17 (checked against a long-double sum).
static void hilbert_kernel_host(int64_t n, int64_t M, std::vector<double2>& h) {
    const int64_t m = (n & 1) ? (n - 1) / 2 : n / 2 - 1;
    std::vector<double> host((size_t)M, 0.0);                 // buf[j mod M] = hh[j mod N], j in [-(N-1), N-1]
    for (int64_t j = 1; j < n; ++j) {
        const double v = (2.0 / (double)n) * dd_sinpi_frac(m * j, n) * dd_sinpi_frac((m + 1) * j, n) / dd_sinpi_frac(j, n);
        host[(size_t)j] = v;
        host[(size_t)(M - n + j)] = v;
    }
    kernel_spectrum_host(host, M, h);
}
// The Hilbert kernel of an EVEN length N is zero at even lags, hh[2j] = 0, hh[2j+1] = (2/N) cot(pi (2j+1) / N) =: g[j]: the length-N circular
// convolution falls apart into two of length N/2 with the same kernel,
//     H(x)[2m+1] = (g (*) x_even)[m]        H(x)[2m] = (g (*) x_odd)[m-1]        (indices mod N/2)
// and z = x_even + j x_odd carries both through ONE complex convolution.  decode_noaa.py:647-653 takes the envelope in blocks of 240 000
// samples: two length-120 000 convolutions fit the cyclic length 2^18 of dd_hconv_kernels.h (>= 2 (N/2) - 1), the block itself does not
// (it would need 2^19).  This is g's spectrum for that image -- g[j mod N/2] at lags j in [-(N/2 - 1), N/2 - 1] -- in row-pass order.
static void hilbert_split_host(int64_t N, int64_t M, std::vector<double2>& h) {
    const int64_t N2 = N / 2;
    std::vector<double> host((size_t)M, 0.0);
    auto g = [&](int64_t j) {                                  // (2/N) cot(pi (2j+1) / N), arguments reduced in integers
        const int64_t k = 2 * j + 1;
        return (2.0 / (double)N) * dd_sinpi_frac(2 * k + N, 2 * N) / dd_sinpi_frac(k, N);      // cos(pi k / N) = sin(pi (2k + N) / (2N))
    };
    for (int64_t j = 0; j < N2; ++j) {
        const double v = g(j);
        host[(size_t)j] = v;                                   // lag +j
        if (j > 0) host[(size_t)(M - N2 + j)] = v;             // lag j - N/2 (the same circular index)
    }
    kernel_spectrum_host(host, M, h);
}
// (length and cyclic length; negative: the split kernel of length n, beside the full ones)
static std::pair<int, int64_t> hilbert_key(int dev, int64_t n, int64_t M, bool split) {
    const int64_t k = (n << 6) | lg_of(M);
    return std::make_pair(dev, split ? -k : k);
}
static void hilbert_host(int64_t n, int64_t M, bool split, std::vector<double2>& h) {
    if (split) hilbert_split_host(n, M, h); else hilbert_kernel_host(n, M, h);
}
// ONE walk for both kernels: device cache, host cache, build, keep, upload, put.  *out: the M/2 + 1 bins of the library's real
// transforms; for the lengths of dd_hconv_kernels.h the row-pass order follows at *out + M/2 + 1.  The caller holds g_sync_mu.
static int hilbert_spectrum(int64_t n, int64_t M, bool split, const double2** out, hipStream_t s) {
    int dev = 0;
    DD_HIP_CHECK(hipGetDevice(&dev));
    const auto key = hilbert_key(dev, n, M, split);
    auto it = g_hilb.find(key);
    if (it != g_hilb.end()) { *out = it->second; return DD_OK; }
    std::vector<double2> h;
    const std::vector<double2>* hp = hilb_host_find(key);
    if (!hp) { hilbert_host(n, M, split, h); hp = hilb_host_keep(key, h); }
    DDDevBuf<double2> HH;
    const int rc = kernel_spectrum_put(hp ? *hp : h, &HH, s);
    if (rc != DD_OK) return rc;
    *out = hilb_cache_put(key, HH);
    return DD_OK;
}

// ---------------------------------------------------------------- the four routes of one group of equal blocks
// a block of real float64 audio as the source and its envelope as the sink of the three launches; job = block.
// Split form (even block length N): element n of the image = (x[2n], x[2n+1]), n < N/2; result element m = (H(x)[2m+1], H(x)[2(m+1)]).
struct HcBlkSplitIO {
    const double* x;
    double* env;
    int64_t N, N2;
    __device__ int rows(int, int cols) const { return (int)((N2 + cols - 1) / cols); }
    __device__ double2 at(int job, int64_t n) const {
        if (n >= N2) return make_double2(0.0, 0.0);
        const double* p = x + (int64_t)job * N + 2 * n;
        return make_double2(p[0], p[1]);
    }
    __device__ void put(int job, int64_t m, double2 y) const {
        if (m >= N2) return;
        const double* p = x + (int64_t)job * N;
        double* e = env + (int64_t)job * N;
        e[2 * m + 1] = hypot(p[2 * m + 1], y.x);
        const int64_t m1 = m + 1 == N2 ? 0 : m + 1;
        e[2 * m1] = hypot(p[2 * m1], y.y);
    }
};
// Plain form (any length n with 2 n + 2 <= M): element i = (x[i], 0); result element i = (H(x)[i], -)
struct HcBlkRealIO {
    const double* x;
    double* env;
    int64_t n;
    __device__ int rows(int, int cols) const { return (int)((n + cols - 1) / cols); }
    __device__ double2 at(int, int64_t i) const { return i < n ? make_double2(x[i], 0.0) : make_double2(0.0, 0.0); }
    __device__ void put(int, int64_t i, double2 y) const { if (i < n) env[i] = hypot(x[i], y.x); }
};
// envelope of `jobs` blocks of N samples each (x + job N) through dd_hconv_kernels.h; T: [jobs][M] c128 work buffer.  split: the
// even / odd form above (N even, N - 1 <= M); else the plain form (one block, 2 N + 2 <= M).  M: hc_block_len's.
static int hc_block_envelope(const double* x, double* env, int64_t N, int jobs, bool split, int64_t M, double2* T, hipStream_t s) {
    const double2* HH = nullptr;
    const int rc = hilbert_spectrum(N, M, split, &HH, s);
    if (rc != DD_OK) return rc;
    const HcOneSpec sp = {HH + (M / 2 + 1)};
    if (split) {
        const HcBlkSplitIO io = {x, env, N, N / 2};
        return hc_run(M, io, sp, io, T, jobs, s);
    }
    const HcBlkRealIO io = {x, env, N};
    return hc_run(M, io, sp, io, T, 1, s);
}

// The library's real pair: envelope = hypot(x, H x) with H x from a real-to-complex / complex-to-real transform pair per block (bin k of
// the spectrum times -j for 0 < k < N/2, zero at DC and Nyquist: the imaginary part of scipy.signal.hilbert's analytic signal), `batch`
// consecutive blocks of N samples in one batched pair.  spec: [batch][N/2 + 1], y: [batch][N]
__global__ void __launch_bounds__(256) k_hilb_bins(double2* __restrict__ S, int64_t nb, int64_t N) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nb) return;
    double2* p = S + (int64_t)blockIdx.y * nb + k;
    const double2 v = *p;
    const bool zero = k == 0 || (2 * k == N);
    *p = zero ? make_double2(0.0, 0.0) : make_double2(v.y, -v.x);          // -j X[k]
}
__global__ void __launch_bounds__(256) k_env_hypot_flat(const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ env, int64_t n, double inv_n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) env[i] = hypot(x[i], y[i] * inv_n);
}
static int envelope_real_pair(const double* x, double* env, int64_t N, int batch, double2* spec, double* y, hipStream_t s) {
    hipfftHandle pf, pb;
    int rc = get_plan(&pf, HIPFFT_D2Z, N, batch, s);
    if (rc == DD_OK) rc = get_plan(&pb, HIPFFT_Z2D, N, batch, s);
    if (rc != DD_OK) return rc;
    const int64_t nb = N / 2 + 1;
    DD_FFT_CHECK(hipfftExecD2Z(pf, (hipfftDoubleReal*)x, (hipfftDoubleComplex*)spec));
    hipLaunchKernelGGL(k_hilb_bins, dim3(grid1(nb), batch), dim3(256), 0, s, spec, nb, N);
    DD_FFT_CHECK(hipfftExecZ2D(pb, (hipfftDoubleComplex*)spec, (hipfftDoubleReal*)y));
    hipLaunchKernelGGL(k_env_hypot_flat, dim3(grid1(N * batch)), dim3(256), 0, s, x, y, env, N * batch, 1.0 / (double)N);
    return DD_OK;
}
// The zero-padded real convolution behind its pad kernel: XR [batch][M] holds the padded images (k_pad_f64 here, k_sync_fm_pad for the
// accurate-sync windows), HH the kernel spectrum of hilbert_spectrum(n, M, false); SP: [batch][M/2 + 1], YR: [batch][M]; env: [batch][n]
__global__ void __launch_bounds__(256) k_pad_f64(const double* __restrict__ x, int64_t n, double* __restrict__ XR, int64_t M) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < M) XR[j] = j < n ? x[j] : 0.0;
}
static int envelope_padded(double* XR, double2* SP, double* YR, const double2* HH, int64_t M, int64_t n, int batch, double* env, hipStream_t s) {
    hipfftHandle pf, pb;
    int rc = get_plan(&pf, HIPFFT_D2Z, M, batch, s);
    if (rc == DD_OK) rc = get_plan(&pb, HIPFFT_Z2D, M, batch, s);
    if (rc != DD_OK) return rc;
    const int64_t nb = M / 2 + 1;
    DD_FFT_CHECK(hipfftExecD2Z(pf, XR, (hipfftDoubleComplex*)SP));
    hipLaunchKernelGGL(k_spec_mul, dim3(grid1(nb), batch), dim3(256), 0, s, SP, HH, nb);
    DD_FFT_CHECK(hipfftExecZ2D(pb, (hipfftDoubleComplex*)SP, YR));
    hipLaunchKernelGGL(k_env_hypot, dim3(grid1(n), batch), dim3(256), 0, s, XR, YR, M, n, env);
    return DD_OK;
}

// ---------------------------------------------------------------- the runner
static int envelope_group(const DDEnvGroup& g, const double* x, double* env, int jobs, double2* T, double2* spec, double* y, hipStream_t s) {
    if (g.route == DD_ENV_LIB_PAIR) return envelope_real_pair(x, env, g.N, jobs, spec, y, s);
    if (g.route != DD_ENV_LIB_PADDED) return hc_block_envelope(x, env, g.N, jobs, g.route == DD_ENV_OWN_SPLIT, g.M, T, s);
    const double2* HH = nullptr;
    const int rc = hilbert_spectrum(g.N, g.M, false, &HH, s);
    if (rc != DD_OK) return rc;
    hipLaunchKernelGGL(k_pad_f64, dim3(grid1(g.M)), dim3(256), 0, s, x, g.N, y, g.M);
    return envelope_padded(y, spec, y + g.M, HH, g.M, g.N, 1, env, s);
}
// enqueues the whole envelope of x [n] by the plan w = envelope_plan(n, block); T, spec, y: w's element counts.  The caller holds
// g_sync_mu (the spectrum cache) and keeps the three work areas until the stream has run
static int envelope_walk(const DDEnvWalk& w, const double* x, double* env, double2* T, double2* spec, double* y, hipStream_t s) {
    int rc = DD_OK;
    for (int64_t b0 = 0; b0 < w.nfull && rc == DD_OK; b0 += w.batch)
        rc = envelope_group(w.full, x + b0 * w.block, env + b0 * w.block, (int)std::min(w.nfull - b0, w.batch), T, spec, y, s);
    if (rc == DD_OK) rc = envelope_group(w.last, x + w.nfull * w.block, env + w.nfull * w.block, 1, T, spec, y, s);
    if (rc == DD_OK) DD_LAUNCH_CHECK();
    return rc;
}

extern "C" int dd_am_envelope_f64(const double* in, double* out, int64_t n, int64_t block, void* stream) {
    DD_REQUIRE(n >= 0 && block >= 1, "n/block");
    if (n == 0) return DD_OK;
    DD_REQUIRE(in && out, "null buffer");
    hipStream_t s = dd_stream(stream);
    const DDEnvWalk w = envelope_plan(n, block);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_spec = al(sizeof(double2) * w.T_elems), o_y = o_spec + al(sizeof(double2) * w.spec_elems);
    DDScratchLock scr;                      // held until this entry point has enqueued everything; it returns with the work in flight
    const int rc = scr.get(o_y + sizeof(double) * w.y_elems, s);
    if (rc != DD_OK) return rc;
    std::lock_guard<std::mutex> lk(g_sync_mu);
    return envelope_walk(w, in, out, (double2*)scr.ptr, (double2*)(scr.ptr + o_spec), (double*)(scr.ptr + o_y), s);
}
#endif  // DD_ENVELOPE_PLAN_ONLY
