// Meteor-M2 LRPT: the image packets' JPEG-like payload -- Huffman decoding, dequantisation and the 8x8 inverse transform of a
// packet's 14 blocks (DESIGN.md section 4.16 defines every quantity, all of them integers; lrpt.py restates them in NumPy),
// included by dd_afsk.hip after dd_lrpt_rs.h.
//
//   k_lrpt_jpeg  -- one wave per packet and no workgroup barrier.  The bit stream is serial and wave-uniform: a 64-bit window in
//                   scalar registers, fed 32 bits at a time from 256 bytes of the packet staged in LDS, which the 64 lanes refill
//                   together (no load reaches past the packet's last byte; what lies beyond reads as zero and is never
//                   accepted).  A code's length is found across the lanes (lane l < 16 holds length l + 1's first code and
//                   count, a ballot's lowest bit is the length), its value comes from the lanes' registers, and lane k writes
//                   zigzag position k's dequantised coefficient: no LDS read lies between two symbols but the window's.
//                   Then lane = pixel: the column pass into LDS, the row pass into a byte store.
#pragma once

#define DD_JPEG_MCUS 14
#define DD_JPEG_WIN 256               // bytes of the packet staged in LDS at a time

struct DDJpegTables {
    uint16_t first[2][16];            // per table (0 DC, 1 AC) and length - 1: the first code, how many, the first one's index
    uint16_t count[2][16];
    uint16_t index[2][16];
    uint8_t values[162];              // the AC table's; the DC table's value is its index
    uint8_t zigzag[64];
    uint8_t quant[64];
    int16_t m[8][8];
};

static constexpr DDJpegTables dd_jpeg_make_tables() {
    DDJpegTables t{};
    const int bits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}};
    const uint8_t ac[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
        0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
        0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
        0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
        0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
        0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
        0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
        0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    for (int i = 0; i < 162; ++i) t.values[i] = ac[i];
    for (int tb = 0; tb < 2; ++tb) {
        int code = 0, k = 0;
        for (int l = 0; l < 16; ++l) {
            t.first[tb][l] = (uint16_t)code;
            t.count[tb][l] = (uint16_t)bits[tb][l];
            t.index[tb][l] = (uint16_t)k;
            code = (code + bits[tb][l]) << 1;
            k += bits[tb][l];
        }
    }
    const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    const uint8_t qs[64] = {16, 11, 10, 16, 24, 40, 51, 61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24,  40,  57,
                            69, 56, 14, 17, 22, 29, 51, 87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35,  55,  64,
                            81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    for (int i = 0; i < 64; ++i) {
        t.zigzag[i] = zz[i];
        t.quant[i] = qs[i];
    }
    const int16_t m[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},     {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                             {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                             {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                             {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
    for (int k = 0; k < 8; ++k)
        for (int n = 0; n < 8; ++n) t.m[k][n] = m[k][n];
    return t;
}

__constant__ DDJpegTables dd_jpeg_tables = dd_jpeg_make_tables();

// what the wave's lanes wrote to LDS is visible to its lanes' reads that follow
__device__ __forceinline__ void dd_jpeg_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The packet's bit stream: a 64-bit window in scalar registers, the next bit at bit 63, refilled 32 bits at a time from stage[],
// which holds the packet's bytes base .. base + 255 (zero from the packet's end on).  Every quantity here is wave-uniform.
struct DDJpegBits {
    const uint8_t* src;               // the packet's first byte
    int len;                          // its bytes (the entry point keeps a packet below 2^27 bytes)
    int bit;                          // bits consumed
    int rd;                           // the packet byte that enters the window next, a multiple of 4
    int base;                         // the packet byte in stage[0]
    uint64_t win;
    int have;                         // bits in the window, zero fill past the packet's end included
    uint32_t* stage;
    int lane;

    __device__ __forceinline__ void fill() {
        dd_jpeg_wave_sync();                                    // the reads of the old bytes are over
        base = rd;
        uint8_t* bytes = (uint8_t*)stage;
        for (int q = 0; q < DD_JPEG_WIN / 64; ++q) {
            const int at = base + lane + 64 * q;
            bytes[lane + 64 * q] = at < len ? src[at] : (uint8_t)0;
        }
        dd_jpeg_wave_sync();
    }

    // at least 32 bits in the window: enough for a code (16) and its value (11) without another look
    __device__ __forceinline__ void ensure() {
        if (have >= 32) return;
        if (rd - base >= DD_JPEG_WIN) fill();
        const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_bswap32(stage[(rd - base) >> 2]));
        win |= (uint64_t)w << (32 - have);
        have += 32;
        rd += 4;
    }

    __device__ __forceinline__ void take(int n) {
        win <<= n;
        have -= n;
        bit += n;
    }
};

// One Huffman code (lane l < 16 holds first, count, index of length l + 1) -> the index of its value, or -1: no code of up to 16
// bits matches, or the code runs past the packet's end
__device__ __forceinline__ int dd_jpeg_code(DDJpegBits& b, int first, int count, int index) {
    b.ensure();
    const int l = b.lane & 15;
    const int top = (int)((uint32_t)(b.win >> 32) >> (31 - l)) - first;     // the window's top l + 1 bits against that length's first code
    const unsigned long long hit = __ballot(b.lane < 16 && top >= 0 && top < count);
    if (hit == 0) return -1;
    const int len = __ffsll((long long)hit);                     // 1..16
    const int idx = __builtin_amdgcn_readlane(index + top, len - 1);
    b.take(len);
    return b.bit > 8 * b.len ? -1 : idx;
}

// EXTEND(next n bits, n) for 1 <= n <= 11, right after dd_jpeg_code; ok = false when they run past the packet's end
__device__ __forceinline__ int dd_jpeg_value(DDJpegBits& b, int n, bool& ok) {
    const int v = (int)(b.win >> (64 - n));
    b.take(n);
    ok = b.bit <= 8 * b.len;
    return v >= (1 << (n - 1)) ? v : v - (1 << n) + 1;
}

// Packet blockIdx.x: desc = offsets[n + 1], then dst[n], then q[n]
__global__ void __launch_bounds__(64) k_lrpt_jpeg(const uint8_t* __restrict__ data, const int64_t* __restrict__ desc, int64_t npackets,
                                                  int64_t pitch, uint8_t* __restrict__ out, int* __restrict__ mcus) {
    __shared__ uint32_t stage[DD_JPEG_WIN / 4];
    __shared__ int16_t coef[DD_JPEG_MCUS][64];
    __shared__ int mid[64];
    const int lane = threadIdx.x;
    const int64_t pkt = blockIdx.x;
    const int64_t start = desc[pkt], end = desc[pkt + 1], dst = desc[npackets + 1 + pkt];
    const int q = __builtin_amdgcn_readfirstlane((int)desc[2 * npackets + 1 + pkt]);

    // lane k keeps zigzag position k's row-major index and quantiser step, and writes that position's coefficients
    const int myat = dd_jpeg_tables.zigzag[lane];
    int myq;
    {
        const int s = dd_jpeg_tables.quant[myat];
        const int v = (q >= 21 && q <= 49) ? (100 * s + q) / (2 * q) : ((200 - 2 * q > 0 ? 200 - 2 * q : 0) * s + 50) / 100;
        myq = v > 1 ? v : 1;
    }
    // the AC table's 162 values across the lanes, three each; the DC table's value is its index
    const int v0 = dd_jpeg_tables.values[lane], v1 = dd_jpeg_tables.values[64 + lane];
    const int v2 = dd_jpeg_tables.values[128 + (lane < 34 ? lane : 0)];
    int first[2], count[2], index[2];
    for (int tb = 0; tb < 2; ++tb) {
        first[tb] = dd_jpeg_tables.first[tb][lane & 15];
        count[tb] = dd_jpeg_tables.count[tb][lane & 15];
        index[tb] = dd_jpeg_tables.index[tb][lane & 15];
    }
    for (int m = 0; m < DD_JPEG_MCUS; ++m) coef[m][lane] = 0;
    DDJpegBits b{data + start, __builtin_amdgcn_readfirstlane((int)(end - start)), 0, 0, 0, 0, 0, stage, lane};
    b.fill();

    // every pass of the loops below consumes at least one bit or leaves: they end within 8 * len + 1 passes
    int done = 0, pred = 0;
    for (; done < DD_JPEG_MCUS; ++done) {
        bool ok = true;
        const int n = dd_jpeg_code(b, first[0], count[0], index[0]);
        if (n < 0) break;
        if (n > 0) pred += dd_jpeg_value(b, n, ok);
        if (!ok) break;
        if (lane == 0) coef[done][0] = (int16_t)max(-2048, min(2047, pred * myq));
        int k = 1;
        while (k < 64) {
            const int idx = dd_jpeg_code(b, first[1], count[1], index[1]);
            if (idx < 0) { ok = false; break; }
            const int rs = __builtin_amdgcn_readlane(idx < 64 ? v0 : (idx < 128 ? v1 : v2), idx & 63);
            const int run = rs >> 4, size = rs & 15;
            if (size == 0) {
                if (run == 0) break;
                k += 16;
                if (run != 15 || k > 63) { ok = false; break; }
                continue;
            }
            k += run;
            if (k > 63) { ok = false; break; }
            const int c = dd_jpeg_value(b, size, ok);
            if (!ok) break;
            if (lane == k) coef[done][myat] = (int16_t)max(-2048, min(2047, c * myq));
            ++k;
        }
        if (!ok) break;
    }
    if (lane == 0) mcus[pkt] = done;
    if (dst < 0) return;
    dd_jpeg_wave_sync();

    // lane = (y, v) in the column pass and (y, x) in the row pass
    const int y = lane >> 3, x = lane & 7;
    int my[8], mx[8];
    for (int u = 0; u < 8; ++u) {
        my[u] = dd_jpeg_tables.m[u][y];
        mx[u] = dd_jpeg_tables.m[u][x];
    }
    uint8_t* row = out + dst + (int64_t)y * pitch + x;
    for (int m = 0; m < done; ++m) {
        int t = 1024;
        for (int u = 0; u < 8; ++u) t += my[u] * coef[m][8 * u + x];
        dd_jpeg_wave_sync();                                    // the last block's row pass has read mid[]
        mid[lane] = t >> 11;
        dd_jpeg_wave_sync();
        int p = 16384;
        for (int v = 0; v < 8; ++v) p += mid[8 * y + v] * mx[v];
        p = (p >> 15) + 128;
        row[8 * m] = (uint8_t)max(0, min(255, p));
    }
}

// npackets packets: data[offsets_host[i] .. offsets_host[i + 1]) are packet i's entropy-coded bytes, q_host[i] its quality factor,
// dst_host[i] the byte offset in out of its top-left pixel (-1: decode, write no pixel), rows pitch bytes apart
extern "C" int dd_lrpt_jpeg(const uint8_t* data, const int64_t* offsets_host, const uint8_t* q_host, const int64_t* dst_host,
                            int64_t npackets, int64_t pitch, uint8_t* out, int32_t* mcus, void* stream) {
    DD_REQUIRE(npackets >= 0 && npackets <= 0x7fffffff, "dd_lrpt_jpeg: sizes");
    DD_REQUIRE(pitch >= 8 * DD_JPEG_MCUS, "dd_lrpt_jpeg: pitch below 112");
    if (npackets == 0) return DD_OK;
    DD_REQUIRE(data != nullptr && offsets_host != nullptr && q_host != nullptr && dst_host != nullptr && out != nullptr && mcus != nullptr,
               "dd_lrpt_jpeg: null buffer");
    DD_REQUIRE(offsets_host[0] >= 0, "dd_lrpt_jpeg: negative offset");
    std::vector<int64_t> desc((size_t)npackets * 3 + 1);
    for (int64_t i = 0; i < npackets; ++i) {
        DD_REQUIRE(offsets_host[i + 1] >= offsets_host[i], "dd_lrpt_jpeg: decreasing offsets");
        DD_REQUIRE(offsets_host[i + 1] - offsets_host[i] < (1 << 27), "dd_lrpt_jpeg: a packet of 2^27 bytes or more");
        DD_REQUIRE(dst_host[i] >= -1, "dd_lrpt_jpeg: dst below -1");
        desc[(size_t)i] = offsets_host[i];
        desc[(size_t)(npackets + 1 + i)] = dst_host[i];
        desc[(size_t)(2 * npackets + 1 + i)] = q_host[i];
    }
    desc[(size_t)npackets] = offsets_host[npackets];
    DDDevBuf<int64_t> d;
    DD_HIP_CHECK(d.alloc(desc.size()));
    int rc = DD_OK;
    if (hipMemcpyAsync(d, desc.data(), d.bytes(), hipMemcpyHostToDevice, dd_stream(stream)) != hipSuccess) rc = DD_ERR_HIP;
    if (rc == DD_OK) {
        hipLaunchKernelGGL(k_lrpt_jpeg, dim3((unsigned)npackets), dim3(64), 0, dd_stream(stream), data, (const int64_t*)d.get(), npackets,
                           pitch, out, mcus);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(dd_stream(stream)) != hipSuccess) rc = DD_ERR_HIP;
    }
    DD_SYM_REQUIRE(rc == DD_OK, "dd_lrpt_jpeg", "launch failed");
    return DD_OK;
}
