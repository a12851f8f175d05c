// What the channel decoders share (DESIGN.md sections 4.14, 4.17 and 4.18; lrpt.py and funcube_fec.py restate it in NumPy), included
// by dd_afsk.hip before dd_lrpt.h.  All arithmetic is integer.
//
//   dd_k7_signs, dd_k7_acs, dd_k7_traceback, dd_k7_mismatch
//                   -- the rate 1/2, K = 7 trellis of one wave, lane = state: k_lrpt_viterbi and k_fc_viterbi choose the steps, the
//                      start metrics and the start state, and walk through these
//   dd_pn           -- the CCSDS pseudo-noise sequence's period as bytes
//   dd_cand_slot    -- where a search kernel's (position, value, score) candidate goes: a capped list with a full count
//   dd_with_spans   -- (host) a call's (position, flag) pairs up to the device, around one launch
#pragma once

#define DD_LRPT_G1 0x79
#define DD_LRPT_G2 0x5B

// State ns is lane ns; it is entered from the states ((ns & 31) << 1) | x, x = 0, 1, with the register r = (input bit, predecessor):
// s1[x], s2[x] = 2 c - 1 of that branch's two code bits.
__device__ __forceinline__ void dd_k7_signs(int lane, int (&s1)[2], int (&s2)[2]) {
    for (int x = 0; x < 2; ++x) {
        const int r = ((lane >> 5) << 6) | ((lane & 31) << 1) | x;
        s1[x] = 2 * (__popc(r & DD_LRPT_G1) & 1) - 1;
        s2[x] = 2 * (__popc(r & DD_LRPT_G2) & 1) - 1;
    }
}

// Add-compare-select over the steps c .. c + nj - 1, nj <= 64: lane j holds the soft pair (a, b) of step c + j, m is the lane's
// metric.  The predecessors' metrics come by cross-lane reads, x = 1 survives only when strictly larger.  The 64 decisions of a
// step are one ballot word; lane j returns the word of step c + j (0 for j >= nj).
__device__ __forceinline__ unsigned long long dd_k7_acs(int a, int b, int nj, int lane, const int (&s1)[2], const int (&s2)[2], int& m) {
    const int pred0 = (lane & 31) << 1;
    unsigned long long w = 0;
    for (int j = 0; j < nj; ++j) {
        const int aj = __builtin_amdgcn_readlane(a, j), bj = __builtin_amdgcn_readlane(b, j);
        const int c0 = __shfl(m, pred0, 64) + s1[0] * aj + s2[0] * bj;
        const int c1 = __shfl(m, pred0 | 1, 64) + s1[1] * aj + s2[1] * bj;
        const bool d = c1 > c0;
        const unsigned long long word = __ballot(d);
        m = d ? c1 : c0;
        if (lane == j) w = word;
    }
    return w;
}

// one step back from the wave-uniform state st: lane j holds the step's decision word as the halves (wl, wh)
__device__ __forceinline__ int dd_k7_back(int wl, int wh, int j, int st) {
    const uint32_t half = (uint32_t)(st < 32 ? __builtin_amdgcn_readlane(wl, j) : __builtin_amdgcn_readlane(wh, j));
    return ((st & 31) << 1) | (int)((half >> (st & 31)) & 1);
}

// Traceback through a group's steps nj - 1 down to 0 (lane j holds dd_k7_acs's word w of step j), from the state st after step
// nj - 1: the decoded bit of a step j in [first, last) goes to ob[j - first], and the walk ends below first.  The window is counted
// from the group's step 0, so first < 0 when it began in an earlier group.  Returns the state before the last step walked.  Two
// loops, the steps past the window and the steps inside it, so that no step pays for a window test.
__device__ __forceinline__ int dd_k7_traceback(unsigned long long w, int nj, int first, int last, int st, int lane, uint8_t* ob) {
    const int wl = (int)(uint32_t)w, wh = (int)(uint32_t)(w >> 32);
    const int lo = first > 0 ? first : 0, hi = last > 0 ? last : 0;
    int j = nj - 1;
    for (; j >= hi; --j) st = dd_k7_back(wl, wh, j, st);
    for (; j >= lo; --j) {
        if (lane == 0) ob[j - first] = (uint8_t)(st >> 5);
        st = dd_k7_back(wl, wh, j, st);
    }
    return st;
}

// how many of a step's two hard bits (a > 0, b > 0) differ from the code bits of r = the decoded bits t-6 .. t, bit t in r's bit 6
__device__ __forceinline__ int dd_k7_mismatch(int r, int a, int b) {
    return ((__popc(r & DD_LRPT_G1) & 1) != (a > 0)) + ((__popc(r & DD_LRPT_G2) & 1) != (b > 0));
}

// the pseudo-noise sequence's first 255 bytes (its period: 255 bits): register all ones, output r[0], feedback r[0] ^ r[3] ^ r[5] ^ r[7]
struct DDPn {
    uint8_t b[255];
};

static constexpr DDPn dd_make_pn() {
    DDPn pn{};
    int r[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    for (int i = 0; i < 255 * 8; ++i) {
        pn.b[i >> 3] = (uint8_t)(pn.b[i >> 3] | (r[0] << (7 - (i & 7))));
        const int fb = r[0] ^ r[3] ^ r[5] ^ r[7];
        for (int q = 0; q < 7; ++q) r[q] = r[q + 1];
        r[7] = fb;
    }
    return pn;
}

__constant__ DDPn dd_pn = dd_make_pn();

// One more candidate of a search kernel: every one is counted, and the first cap of them (in arrival order) get the three entries
// returned for (position, value, score); the others get nullptr.
__device__ __forceinline__ int64_t* dd_cand_slot(int64_t cap, int64_t* __restrict__ cand, unsigned long long* __restrict__ count) {
    const unsigned long long c = atomicAdd(count, 1ull);
    return (int64_t)c < cap ? cand + 3 * c : nullptr;
}

// the (p, flag) pairs go up to a device array of the call, launch(that array) enqueues the kernel, the stream is drained before it is freed
template <class Launch>
static int dd_with_spans(const int64_t* spans_host, int64_t nspans, const char* who, void* stream, Launch launch) {
    DDDevBuf<int64_t> d;
    DD_HIP_CHECK(d.alloc((size_t)nspans * 2));
    int rc = DD_OK;
    if (hipMemcpyAsync(d, spans_host, d.bytes(), hipMemcpyHostToDevice, dd_stream(stream)) != hipSuccess) rc = DD_ERR_HIP;
    if (rc == DD_OK) {
        launch(d.get());
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(dd_stream(stream)) != hipSuccess) rc = DD_ERR_HIP;
    }
    DD_SYM_REQUIRE(rc == DD_OK, who, "launch failed");
    return DD_OK;
}
