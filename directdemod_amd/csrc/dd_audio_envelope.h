// A1: demod_am.demod -- abs(hilbert(x)) per block (demod_am.py:18-29, decode_noaa.py:644-653): dd_am_envelope_f64, and everything about
// Hilbert envelopes that more than one part uses: the Hilbert-kernel spectra (closed forms, host transform, device and host caches)
// and the block envelope through the own float64 transform (hc_block_envelope).
// The first of the six parts of dd_audio.hip (one translation unit: the parts share the plan cache, the float64 transform and the
// scratch buffers of dd_audio.hip and are included there, each using only the parts before it).  Internal; not a stand-alone header.
// ---------------------------------------------------------------- A1: abs(hilbert(x)) per block
// scipy.signal.hilbert: Xf = fft(x); h[0] = 1, h[1..(N-1)/2 or N/2-1] = 2, h[N/2] = 1 (N even),
// 0 elsewhere; ifft(Xf * h); demod_am takes the magnitude (demod_am.py:29).
__global__ void __launch_bounds__(256) k_real_to_cplx(const double* __restrict__ in, double2* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = make_double2(in[i], 0.0);
}
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
        const int lg = M == ((int64_t)1 << 18) ? 9 : 8;
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
static std::pair<int, int64_t> hilbert_kernel_key(int dev, int64_t n, int64_t M) { return std::make_pair(dev, (n << 6) | lg_of(M)); }      // (length and cyclic length)
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
static int hilbert_kernel_spectrum(int64_t n, int64_t M, const double2** out, hipStream_t s) {
    int dev = 0;
    DD_HIP_CHECK(hipGetDevice(&dev));
    const auto key = hilbert_kernel_key(dev, n, M);
    auto it = g_hilb.find(key);
    if (it != g_hilb.end()) { *out = it->second; return DD_OK; }
    std::vector<double2> h;
    const std::vector<double2>* hp = hilb_host_find(key);
    if (!hp) { hilbert_kernel_host(n, M, h); hp = hilb_host_keep(key, h); }
    DDDevBuf<double2> HH;
    const int rc = kernel_spectrum_put(hp ? *hp : h, &HH, s);
    if (rc != DD_OK) return rc;
    *out = hilb_cache_put(key, HH);
    return DD_OK;
}

// The Hilbert kernel of an EVEN length N is zero at even lags, hh[2j] = 0, hh[2j+1] = (2/N) cot(pi (2j+1) / N) =: g[j]: the length-N circular
// convolution falls apart into two of length N/2 with the same kernel,
//     H(x)[2m+1] = (g (*) x_even)[m]        H(x)[2m] = (g (*) x_odd)[m-1]        (indices mod N/2)
// and z = x_even + j x_odd carries both through ONE complex convolution.  decode_noaa.py:647-653 takes the envelope in blocks of 240 000
// samples: two length-120 000 convolutions fit the cyclic length 2^18 of dd_hconv_kernels.h (>= 2 (N/2) - 1), the block itself does not
// (it would need 2^19).  This is g's spectrum for that image -- g[j mod N/2] at lags j in [-(N/2 - 1), N/2 - 1] -- in row-pass order.
static std::pair<int, int64_t> hilbert_split_key(int dev, int64_t N, int64_t M) { return std::make_pair(dev, -((N << 6) | lg_of(M))); }    // (negative: the split kernel of length N, beside the full ones)
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
static int hilbert_split_spectrum(int64_t N, int64_t M, const double2** out_perm, hipStream_t s) {
    int dev = 0;
    DD_HIP_CHECK(hipGetDevice(&dev));
    const auto key = hilbert_split_key(dev, N, M);
    auto it = g_hilb.find(key);
    if (it != g_hilb.end()) { *out_perm = it->second + (M / 2 + 1); return DD_OK; }
    std::vector<double2> h;
    const std::vector<double2>* hp = hilb_host_find(key);
    if (!hp) { hilbert_split_host(N, M, h); hp = hilb_host_keep(key, h); }
    DDDevBuf<double2> HH;
    const int rc = kernel_spectrum_put(hp ? *hp : h, &HH, s);
    if (rc != DD_OK) return rc;
    *out_perm = hilb_cache_put(key, HH) + (M / 2 + 1);
    return DD_OK;
}

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
// even / odd form above (N even, N - 1 <= M); else the plain form (one block, 2 N + 2 <= M).  DD_ERR_UNSUPPORTED: the caller's other route.
static int hc_block_envelope(const double* x, double* env, int64_t N, int jobs, bool split, int64_t M, double2* T, hipStream_t s) {
    if (!hc_length_ok(M)) return DD_ERR_UNSUPPORTED;
    const int lg = M == ((int64_t)1 << 18) ? 9 : 8;
    const double2 *TA = nullptr, *TB = nullptr;
    int rc = hc_tables(lg, &TA, &TB);
    if (rc != DD_OK) return rc;
    const double2* HHp = nullptr;
    if (split) {
        rc = hilbert_split_spectrum(N, M, &HHp, s);
        if (rc != DD_OK) return rc;
        const HcBlkSplitIO io = {x, env, N, N / 2};
        const HcOneSpec sp = {HHp};
        if (lg == 9) { rc = hc_ready<9, HcBlkSplitIO, HcBlkSplitIO>(); if (rc == DD_OK) hc_convolve<9>(io, sp, io, T, jobs, TA, TB, s); }
        else { rc = hc_ready<8, HcBlkSplitIO, HcBlkSplitIO>(); if (rc == DD_OK) hc_convolve<8>(io, sp, io, T, jobs, TA, TB, s); }
    } else {
        const double2* HH = nullptr;
        rc = hilbert_kernel_spectrum(N, M, &HH, s);
        if (rc != DD_OK) return rc;
        HHp = HH + (M / 2 + 1);
        const HcBlkRealIO io = {x, env, N};
        const HcOneSpec sp = {HHp};
        if (lg == 9) { rc = hc_ready<9, HcBlkRealIO, HcBlkRealIO>(); if (rc == DD_OK) hc_convolve<9>(io, sp, io, T, 1, TA, TB, s); }
        else { rc = hc_ready<8, HcBlkRealIO, HcBlkRealIO>(); if (rc == DD_OK) hc_convolve<8>(io, sp, io, T, 1, TA, TB, s); }
    }
    return rc;
}

// cyclic length of dd_hconv_kernels.h for the envelope of a block of N real samples, 0 = not on this route; *split: the even / odd form
static int64_t hc_block_len(int64_t N, bool* split) {
    if (N < 2) return 0;
    if ((N & 1) == 0 && N - 1 <= ((int64_t)1 << 18)) { *split = true; return N - 1 <= ((int64_t)1 << 17) ? (int64_t)1 << 17 : (int64_t)1 << 18; }
    *split = false;
    if (2 * N + 2 <= ((int64_t)1 << 17)) return (int64_t)1 << 17;
    if (2 * N + 2 <= ((int64_t)1 << 18)) return (int64_t)1 << 18;
    return 0;
}

// `batch` consecutive blocks of n samples each: one batched transform pair
static int envelope_blocks(const double* in, double* out, int64_t n, int batch, double2* work, hipStream_t s) {
    hipfftHandle plan;
    int rc = get_plan(&plan, HIPFFT_Z2Z, n, batch, s);
    if (rc != DD_OK) return rc;
    hipLaunchKernelGGL(k_real_to_cplx, dim3(grid1(n * batch)), dim3(256), 0, s, in, work, n * batch);
    DD_FFT_CHECK(hipfftExecZ2Z(plan, (hipfftDoubleComplex*)work, (hipfftDoubleComplex*)work, HIPFFT_FORWARD));
    hipLaunchKernelGGL(k_hilbert_mask_b, dim3(grid1(n), batch), dim3(256), 0, s, work, n);
    DD_FFT_CHECK(hipfftExecZ2Z(plan, (hipfftDoubleComplex*)work, (hipfftDoubleComplex*)work, HIPFFT_BACKWARD));
    hipLaunchKernelGGL(k_cplx_abs_b, dim3(grid1(n), batch), dim3(256), 0, s, work, out, n, 1.0 / (double)n);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_am_envelope_f64(const double* in, double* out, int64_t n, int64_t block, void* stream) {
    DD_REQUIRE(n >= 0 && block >= 1, "n/block");
    if (n == 0) return DD_OK;
    DD_REQUIRE(in && out, "null buffer");
    hipStream_t s = dd_stream(stream);
    // block list by the chunker rule (decode_noaa.py:644-653 via chunker.py:36-45): full blocks while one more
    // fits strictly inside, then the remainder (a full-size last block when n is an exact multiple)
    int64_t nfull = 0;
    while ((nfull + 1) * block < n) ++nfull;
    const int64_t rem = n - nfull * block;                  // 1 .. block
    const int GB = 16;                                       // full blocks per batched transform
    const int64_t gb = nfull < GB ? nfull : GB;
    // Round 5: blocks that fit the own float64 transform go through it (hc_block_envelope: a 240 000-sample block by the even / odd split
    // of the Hilbert kernel) -- no FFT-library plan, whose creation costs a process's first call 0.9 s.  DD_AM_HILBERT=lib: the library.
    static const char* amh_env = getenv("DD_AM_HILBERT");
    const bool own_ok = !(amh_env && !strcmp(amh_env, "lib"));
    bool split_b = false, split_r = false;
    const int64_t Mb = (own_ok && nfull > 0) ? hc_block_len(block, &split_b) : 0;
    const int64_t Mr = own_ok ? hc_block_len(rem, &split_r) : 0;
    const int64_t wlen = nfull ? std::max<int64_t>(Mb ? (split_b ? gb * Mb : Mb) : 0, Mb ? 0 : gb * block) : 0;
    const int64_t wrem = Mr ? Mr : rem;
    DDScratchLock scr;                      // held until this entry point has enqueued everything
    int rc = scr.get(sizeof(double2) * (size_t)(wlen > wrem ? wlen : wrem), s);
    char* base = scr.ptr;
    if (rc != DD_OK) return rc;
    double2* work = reinterpret_cast<double2*>(base);
    if (Mb) {
        std::lock_guard<std::mutex> lk(g_sync_mu);           // (the kernel-spectrum cache)
        const int per = split_b ? (int)gb : 1;
        for (int64_t b0 = 0; b0 < nfull && rc == DD_OK; b0 += per)
            rc = hc_block_envelope(in + b0 * block, out + b0 * block, block, (int)(nfull - b0 < per ? nfull - b0 : per), split_b, Mb, work, s);
    } else {
        for (int64_t b0 = 0; b0 < nfull && rc == DD_OK; b0 += GB) {
            const int nbk = (int)(nfull - b0 < GB ? nfull - b0 : GB);
            rc = envelope_blocks(in + b0 * block, out + b0 * block, block, nbk, work, s);
        }
    }
    if (rc == DD_OK) {
        if (Mr) {
            std::lock_guard<std::mutex> lk(g_sync_mu);
            rc = hc_block_envelope(in + nfull * block, out + nfull * block, rem, 1, split_r, Mr, work, s);
        } else {
            rc = envelope_blocks(in + nfull * block, out + nfull * block, rem, 1, work, s);
        }
    }
    return rc;
}
