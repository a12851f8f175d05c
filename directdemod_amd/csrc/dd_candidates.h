// What the burst decoders share (ADS-B, AIS, POCSAG, ACARS, RS41, RDS; dd_sstv.h uses the block scan for its class counts), included by
// dd_afsk.hip before them.  Each of them tests every sample as a start, 256 to a workgroup, lists the starts that pass in order below a
// capacity and hands one wave to each survivor; here are the pieces of the first two stages and what the survivors' kernels read alike.
//
//   dd_scan256, k_scan_tops   -- the inclusive scan of one int per thread of a workgroup; the workgroups' counts into their exclusive scan
//   dd_prefix256              -- an LDS array of a workgroup into its exclusive wrap-around prefix sum in place
//   dd_stage_prefix256        -- a tile's values staged in LDS, 0 outside the data, and prefixed: how a sync kernel opens
//   dd_cand_tail              -- the mask byte of a start and the workgroup's pass count: how a sync kernel ends
//   k_cand_list               -- the masks' set bits among `keep` as an ordered candidate list below the capacity
//   dd_cand_run               -- the driver: the sync kernel, k_scan_tops, the count to the host, k_cand_list
//   dd_cand_entry, dd_cand_masks_entry -- the C entries *_candidates and dd_debug_*_masks around the driver
//   dd_fm_q, dd_bit_mid, dd_window_sum -- FM audio quantised, the middle sample of a bit, a bit's value as the survivors' waves sum it
#pragma once

#define DD_CAND_TILE 256              // starts per workgroup of every sync kernel, threads of every kernel here
#define DD_CAND_SPAN 4368             // prefix entries of a POCSAG or RS41 tile at most: 257 + floor(31.5 * 128) + 2 * 38 + 1 = 4366
#define DD_FM_SCALE (1048576.0 / 3.14159265358979323846)
#define DD_FM_CLIP 2097152.0          // |q| <= 2^21: twice what a discriminator can give; beyond it and for a NaN q = 0

static inline size_t dd_up16(size_t b) { return (b + 15) & ~(size_t)15; }

// the FM discriminator's output in radians per sample as an integer: one multiply and one rint
__device__ __forceinline__ int dd_fm_q(double x) {
    const double r = rint(x * DD_FM_SCALE);
    return (r >= -DD_FM_CLIP && r <= DD_FM_CLIP) ? (int)r : 0;
}

// the middle sample of bit k of the start t
__device__ __forceinline__ int64_t dd_bit_mid(int64_t t, int k, double sps) {
    return (int64_t)floor((double)t + ((double)k + 0.5) * sps);
}

// the sum of q over the samples at - h .. at + h that lie inside the audio
__device__ __forceinline__ int dd_window_sum(const double* __restrict__ x, int64_t n, int64_t at, int h) {
    int s = 0;
    for (int j = -h; j <= h; ++j) {
        const int64_t i = at + j;
        if (i >= 0 && i < n) s += dd_fm_q(x[i]);
    }
    return s;
}

// inclusive scan of one int per thread over a workgroup of 256; sh holds 256 ints
__device__ __forceinline__ int dd_scan256(int v, int* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int a = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    return sh[t];
}

// bsum[nb] -> its exclusive scan in place, the total in bsum[nb]; one workgroup of 256
__global__ void __launch_bounds__(256) k_scan_tops(int* __restrict__ bsum, int64_t nb) {
    __shared__ int sh[256];
    int carry = 0;
    for (int64_t base = 0; base < nb; base += 256) {
        const int64_t b = base + threadIdx.x;
        const int v = b < nb ? bsum[b] : 0;
        const int s = dd_scan256(v, sh);
        if (b < nb) bsum[b] = carry + s - v;
        carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

// inclusive wrap-around scan of one value per thread over a workgroup of 256; sh holds 4 values
__device__ __forceinline__ uint32_t dd_prefix_scan256(uint32_t v, uint32_t* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t a = __shfl_up(v, o);
        if (lane >= o) v += a;
    }
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    for (int k = 0; k < wave; ++k) v += sh[k];
    return v;
}

// ps[0 .. span) of a workgroup of 256, staged and synchronised, in place into its exclusive wrap-around prefix sum: ps[j] = the sum
// of the former ps[0 .. j) mod 2^32; synchronised on return.  tops holds 4 values.
__device__ __forceinline__ void dd_prefix256(uint32_t* ps, int span, uint32_t* tops) {
    const int tid = threadIdx.x;
    // thread t owns entries [t c, t c + c): c is odd, so a wave's 64 words of one step fall into distinct banks, 32 per lane group
    const int c = ((span + DD_CAND_TILE - 1) / DD_CAND_TILE) | 1;
    const int lo = tid * c < span ? tid * c : span;
    const int hi = lo + c < span ? lo + c : span;
    uint32_t own = 0;
    for (int j = lo; j < hi; ++j) own += ps[j];
    uint32_t run = dd_prefix_scan256(own, tops) - own;
    for (int j = lo; j < hi; ++j) {
        const uint32_t q = ps[j];
        ps[j] = run;
        run += q;
    }
    __syncthreads();
}

// ps[j] = load(first + j) for j < span, 0 where first + j lies outside the n values, then dd_prefix256 of it: ps[j] becomes the sum
// of the values first .. first + j - 1 (mod 2^32)
template <class Load>
__device__ __forceinline__ void dd_stage_prefix256(Load load, int64_t n, int64_t first, int span, uint32_t* ps, uint32_t* tops) {
    for (int j = threadIdx.x; j < span; j += DD_CAND_TILE) {
        const int64_t i = first + j;
        ps[j] = (i >= 0 && i < n) ? (uint32_t)load(i) : 0u;
    }
    __syncthreads();
    dd_prefix256(ps, span, tops);
}

// the end of a sync kernel: the mask byte m of the start t, where the mask has one, and how many of the workgroup's 256 threads
// pass into bsum; sh holds 256 ints
__device__ __forceinline__ void dd_cand_tail(uint8_t* __restrict__ mask, int64_t t, int64_t n_mask, uint32_t m, int pass, int* sh,
                                             int* __restrict__ bsum) {
    if (t < n_mask) mask[t] = (uint8_t)m;
    const int total = dd_scan256(pass, sh);
    if (threadIdx.x == 255) bsum[blockIdx.x] = total;
}

// list[boff[block] + rank] = k for every set mask bit among `keep` whose place is below cap: ordered, nothing written past cap
__global__ void __launch_bounds__(DD_CAND_TILE) k_cand_list(const uint8_t* __restrict__ mask, int64_t n, int Q, uint32_t keep,
                                                            const int* __restrict__ boff, int64_t* __restrict__ list, int64_t cap) {
    __shared__ int sh[256];
    const int64_t at = (int64_t)blockIdx.x * DD_CAND_TILE + threadIdx.x;
    uint32_t m = at < n ? mask[at] & keep : 0u;
    const int c = __popc(m);
    int64_t place = (int64_t)boff[blockIdx.x] + dd_scan256(c, sh) - c;
    while (m) {
        const int i = __ffs(m) - 1;
        m &= m - 1;
        if (place < cap) list[place] = at * Q + i;
        ++place;
    }
}

// The masks of n_mask samples into scratch or into mask_out, and unless mask_out is given the count and the list of the set bits
// among `keep` below cap, bit i of byte j as j Q + i.  sync(mask, bsum, nb) launches the kernel that tests the nstart starts, 256 per
// workgroup, and leaves a mask byte per sample and the passes of each workgroup.  A count above cap is the caller's to report.
template <class Sync>
static int dd_cand_run(int64_t n_mask, int64_t nstart, int Q, uint32_t keep, uint8_t* mask_out, int64_t* list, int64_t cap,
                       int64_t* count_host, hipStream_t s, Sync sync) {
    const int64_t nb = (nstart + DD_CAND_TILE - 1) / DD_CAND_TILE;
    const size_t bM = mask_out ? 0 : dd_up16((size_t)n_mask), bB = dd_up16(((size_t)nb + 1) * 4);
    DDScratchLock scr;
    int rc = scr.get(bM + bB, s);
    if (rc != DD_OK) return rc;
    uint8_t* mask = mask_out ? mask_out : (uint8_t*)scr.ptr;
    int* bsum = (int*)(scr.ptr + bM);
    sync(mask, bsum, nb);
    DD_LAUNCH_CHECK();
    if (mask_out) {
        DD_HIP_CHECK(hipStreamSynchronize(s));                            // (the scratch is given back on return)
        return DD_OK;
    }
    hipLaunchKernelGGL(k_scan_tops, dim3(1), dim3(256), 0, s, bsum, nb);
    DD_LAUNCH_CHECK();
    int total = 0;
    DD_HIP_CHECK(hipMemcpyAsync(&total, bsum + nb, sizeof(int), hipMemcpyDeviceToHost, s));
    DD_HIP_CHECK(hipStreamSynchronize(s));
    *count_host = total;
    const int64_t kept = total < cap ? total : cap;
    if (kept > 0) {
        hipLaunchKernelGGL(k_cand_list, dim3((unsigned)nb), dim3(DD_CAND_TILE), 0, s, (const uint8_t*)mask, n_mask, Q, keep, (const int*)bsum,
                           list, kept);
        DD_LAUNCH_CHECK();
    }
    return DD_OK;
}

#define DD_CAND_REQUIRE(cond, who, what)                              \
    do {                                                              \
        if (!(cond)) {                                                \
            dd_set_error("invalid argument: %s: %s", who, what);      \
            return DD_ERR_INVALID;                                    \
        }                                                             \
    } while (0)

// A *_candidates entry `who` behind its own grid check (served: the grid's verdict with cap >= 0, need: the entry's text for a
// refusal): the count cleared, nothing to do without data or starts, the driver, and a list that proved too small reported last
template <class Sync>
static int dd_cand_entry(const char* who, bool served, const char* need, const void* data, int64_t n_mask, int64_t nstart, int Q,
                         uint32_t keep, int64_t* list, int64_t cap, int64_t* count_host, hipStream_t s, Sync sync) {
    DD_REQUIRE(served, need);
    DD_CAND_REQUIRE(count_host != nullptr, who, "count");
    *count_host = 0;
    if (n_mask == 0) return DD_OK;
    DD_CAND_REQUIRE(data != nullptr && (cap == 0 || list != nullptr), who, "null buffer");
    if (nstart == 0) return DD_OK;
    int rc = dd_cand_run(n_mask, nstart, Q, keep, nullptr, list, cap, count_host, s, sync);
    if (rc != DD_OK) return rc;
    DD_CAND_REQUIRE(*count_host <= cap, who, "candidate list too small");
    return DD_OK;
}

// A dd_debug_*_masks entry `who` likewise: the mask byte of every sample, 0 behind the last start
template <class Sync>
static int dd_cand_masks_entry(const char* who, bool served, const char* need, const void* data, int64_t n_mask, int64_t nstart,
                               uint8_t* mask, hipStream_t s, Sync sync) {
    DD_REQUIRE(served, need);
    if (n_mask == 0) return DD_OK;
    DD_CAND_REQUIRE(data != nullptr && mask != nullptr, who, "null buffer");
    if (nstart < n_mask) DD_HIP_CHECK(hipMemsetAsync(mask, 0, (size_t)n_mask, s));
    if (nstart == 0) return DD_OK;
    return dd_cand_run(n_mask, nstart, 1, 1u, mask, nullptr, 0, nullptr, s, sync);
}
