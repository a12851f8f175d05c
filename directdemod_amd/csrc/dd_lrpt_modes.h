// The LRPT modes of the Meteor-M N2-x satellites, from soft symbols (beyond the reference; DESIGN.md section 4.18 defines every
// stage bit for bit, lrpt.py restates it in NumPy), included by dd_afsk.hip after dd_lrpt.h.  All arithmetic is integer.
//
// The marker search against the NRZ-M template and the frame finish of a differential stream are dd_lrpt.h's k_lrpt_asm_t and
// k_lrpt_finish<true>; their entry points are here.
//
//   k_lrpt_deint_scores -- the 8-bit marker 0x27 against the hard bits at every symbol under the eight hypotheses, summed per
//                          (segment, symbol mod 40, hypothesis)
//   k_lrpt_deinterleave -- the gather through the convolutional interleaver: marker symbols dropped, one output pair per lane
//   k_lrpt_restagger    -- the rails of an OQPSK demodulator's output brought back together: pair k = (I[k], Q[k + s]) (section 4.19)
#pragma once

#define DD_LRPT_PERIOD 40             // symbols per marker period: 4 of the marker, 36 of interleaved code bits
#define DD_LRPT_MARK_SYMS 4
#define DD_LRPT_GROUP 72              // interleaved bits per period
#define DD_LRPT_MARK_I 0x5u           // the marker 0x27 = 0 0 1 0 0 1 1 1: its even bits (I rail) and its odd bits (Q rail),
#define DD_LRPT_MARK_Q 0x3u           // first symbol in bit 3

// One symbol q per lane; the workgroup's 256 + 3 symbols are staged as four sign bits each.  A lane whose marker fits
// (q + 4 <= nsym) scores its 8 hard bits under each hypothesis and adds the score into [q / (40 seg)][q % 40][h].  The lanes of the
// workgroup's first segment add into the 320 LDS bins, flushed with one global atomic per non-zero bin; a lane of a later segment
// (seg < 7: a segment shorter than the workgroup) adds to global memory itself.  Integer adds: the result does not depend on order.
__global__ void __launch_bounds__(256) k_lrpt_deint_scores(const char2* __restrict__ soft, int64_t nsym, int64_t seglen,
                                                            int* __restrict__ scores) {
    __shared__ uint8_t sg[256 + DD_LRPT_MARK_SYMS - 1];
    __shared__ int bins[DD_LRPT_PERIOD * 8];
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * 256;
    dd_lrpt_stage_signs(soft, nsym, p0, 256 + DD_LRPT_MARK_SYMS - 1, sg);
    for (int i = tid; i < DD_LRPT_PERIOD * 8; i += 256) bins[i] = 0;
    __syncthreads();
    const int64_t seg0 = p0 / seglen;
    const int64_t q = p0 + tid;
    if (q + DD_LRPT_MARK_SYMS <= nsym) {
        uint32_t m[4];                        // per sign bit: the 4 symbols from q, the first in bit 3
        dd_lrpt_sign_masks(sg + tid, DD_LRPT_MARK_SYMS, m);
        const int64_t sgm = q / seglen;
        const int slot = (int)(q % DD_LRPT_PERIOD) * 8;
        for (int h = 0; h < 8; ++h) {
            uint32_t hi, hq;
            dd_lrpt_hyp_hard(m, h, hi, hq);
            const int score = __popc(~(hi ^ DD_LRPT_MARK_I) & 0xFu) + __popc(~(hq ^ DD_LRPT_MARK_Q) & 0xFu);
            if (sgm == seg0) atomicAdd(&bins[slot + h], score);
            else if (score) atomicAdd(&scores[sgm * (DD_LRPT_PERIOD * 8) + slot + h], score);
        }
    }
    __syncthreads();
    for (int i = tid; i < DD_LRPT_PERIOD * 8; i += 256)
        if (bins[i]) atomicAdd(&scores[seg0 * (DD_LRPT_PERIOD * 8) + i], bins[i]);
}

// output pair k = deinterleaved bits n = 2k, 2k + 1: data position n + B M (n mod B), group t = position / 72 and index i inside it,
// symbol o + 40 t + 4 + i / 2, rail i % 2, under h; 128 is stored as 127.  span = B M; every position is below 72 * groups by the
// choice of nout (host), so every symbol read is below nsym.
__global__ void __launch_bounds__(256) k_lrpt_deinterleave(const char2* __restrict__ soft, int o, int h, int branches, int64_t span,
                                                            char2* __restrict__ out, int64_t nout) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nout) return;
    int v[2];
    for (int e = 0; e < 2; ++e) {
        const int64_t n = 2 * k + e;
        const int64_t pos = n + span * (n % branches);
        const int64_t t = pos / DD_LRPT_GROUP;
        const int i = (int)(pos % DD_LRPT_GROUP);
        const char2 s = soft[o + DD_LRPT_PERIOD * t + DD_LRPT_MARK_SYMS + (i >> 1)];
        int a, b;
        dd_lrpt_hyp(s.x, s.y, h, a, b);
        const int w = (i & 1) ? b : a;
        v[e] = w > 127 ? 127 : w;
    }
    out[k] = make_char2((signed char)v[0], (signed char)v[1]);
}

// s = -1, 0, +1: output pair j = (I[j + lead], Q[j + lead + s]) with lead = 1 for s = -1, else 0; nout = nsym - |s| pairs, so both
// indices lie inside the nsym input pairs.  One lane per pair, one char2 store.
__global__ void __launch_bounds__(256) k_lrpt_restagger(const signed char* __restrict__ soft, int s, char2* __restrict__ out, int64_t nout) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nout) return;
    const int64_t k = j + (s < 0 ? 1 : 0);
    out[j] = make_char2(soft[2 * k], soft[2 * (k + s) + 1]);
}

extern "C" int dd_lrpt_restagger(const int8_t* soft, int64_t nsym, int s, int8_t* out, void* stream) {
    DD_REQUIRE(nsym >= 0 && s >= -1 && s <= 1, "dd_lrpt_restagger: nsym >= 0 and a stagger of -1, 0 or 1 expected");
    const int64_t nout = nsym - (s != 0 ? 1 : 0);
    if (nout <= 0) return DD_OK;
    DD_REQUIRE(soft != nullptr && out != nullptr, "dd_lrpt_restagger: null buffer");
    DD_REQUIRE((nout + 255) / 256 <= 0x7fffffff, "dd_lrpt_restagger: too many symbols");
    hipLaunchKernelGGL(k_lrpt_restagger, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, dd_stream(stream), (const signed char*)soft, s,
                       (char2*)out, nout);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_lrpt_asm_search_t(const int8_t* soft, int64_t nsym, unsigned long long encoded, int min_score, int64_t cap, int64_t* cand,
                                    unsigned long long* count, void* stream) {
    return dd_lrpt_asm_run("dd_lrpt_asm_search_t", soft, nsym, encoded, min_score, cap, cand, count, stream);
}

extern "C" int dd_lrpt_finish_nrzm(const uint8_t* bits_packed, const int8_t* soft, int64_t nsym, const int64_t* spans_host, int64_t nspans,
                                   uint8_t* bodies, int32_t* info, void* stream) {
    return dd_lrpt_finish_run("dd_lrpt_finish_nrzm", true, bits_packed, soft, nsym, spans_host, nspans, bodies, info, stream);
}

extern "C" int dd_lrpt_deint_scores(const int8_t* soft, int64_t nsym, int64_t seg, int32_t* scores, void* stream) {
    DD_REQUIRE(nsym >= 0 && seg >= 1 && seg <= (1 << 24), "dd_lrpt_deint_scores: nsym >= 0 and 1 <= seg <= 2^24 expected");
    if (nsym == 0) return DD_OK;
    DD_REQUIRE(soft != nullptr && scores != nullptr, "dd_lrpt_deint_scores: null buffer");
    const int64_t seglen = DD_LRPT_PERIOD * seg;
    const int64_t nseg = (nsym + seglen - 1) / seglen;
    DD_REQUIRE((nsym + 255) / 256 <= 0x7fffffff, "dd_lrpt_deint_scores: too many symbols");
    DD_HIP_CHECK(hipMemsetAsync(scores, 0, (size_t)nseg * DD_LRPT_PERIOD * 8 * sizeof(int32_t), dd_stream(stream)));
    if (nsym < DD_LRPT_MARK_SYMS) return DD_OK;
    hipLaunchKernelGGL(k_lrpt_deint_scores, dim3((unsigned)((nsym - DD_LRPT_MARK_SYMS + 1 + 255) / 256)), dim3(256), 0, dd_stream(stream),
                       (const char2*)soft, nsym, seglen, scores);
    DD_LAUNCH_CHECK();
    return DD_OK;
}

extern "C" int dd_lrpt_deinterleave(const int8_t* soft, int64_t nsym, int o, int h, int branches, int delay, int8_t* out,
                                    int64_t* nsym_out, void* stream) {
    DD_REQUIRE(nsym >= 0 && nsym_out != nullptr, "dd_lrpt_deinterleave: sizes");
    DD_REQUIRE(o >= 0 && o < DD_LRPT_PERIOD, "dd_lrpt_deinterleave: offset outside 0..39");
    DD_REQUIRE(h >= 0 && h < 8, "dd_lrpt_deinterleave: hypothesis outside 0..7");
    DD_REQUIRE(branches >= 1 && DD_LRPT_GROUP % branches == 0, "dd_lrpt_deinterleave: branches must divide 72");
    DD_REQUIRE(delay >= 0, "dd_lrpt_deinterleave: delay < 0");
    const int64_t span = (int64_t)branches * delay;                        // below 72 * 2^31
    const int64_t groups = nsym > o ? (nsym - o) / DD_LRPT_PERIOD : 0;
    const int64_t nbits = DD_LRPT_GROUP * groups - span * (branches - 1);  // the largest position read is nbits - 1 + span (B - 1)
    const int64_t nout = nbits > 0 ? nbits / 2 : 0;
    *nsym_out = nout;
    if (nout == 0) return DD_OK;
    DD_REQUIRE(soft != nullptr && out != nullptr, "dd_lrpt_deinterleave: null buffer");
    DD_REQUIRE((nout + 255) / 256 <= 0x7fffffff, "dd_lrpt_deinterleave: too many symbols");
    hipLaunchKernelGGL(k_lrpt_deinterleave, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, dd_stream(stream), (const char2*)soft, o, h,
                       branches, span, (char2*)out, nout);
    DD_LAUNCH_CHECK();
    return DD_OK;
}
