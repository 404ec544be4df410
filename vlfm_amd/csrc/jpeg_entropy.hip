// jpeg_entropy.hip -- gfx950 baseline JPEG encoder for a batch of frames: the files that libjpeg-turbo writes as Pillow drives
// it (save(format="JPEG", quality=q, subsampling="4:2:0")), byte for byte.  tests/jpeg_huff_ref.py is the NumPy form, held to
// Pillow.  The coefficient pass is jpeg_codec.hip's coding kernel stopped after quantisation; this file turns the
// coefficients into files: header (jcmarker.c), Huffman coding with the standard tables (jchuff.c encode_one_block), byte
// stuffing and EOI.
//
// Seven launches per call, whatever the batch, and no host round trip between them:
//
//   jpeg_code_kernel<true,*>   (jpeg_codec.hip) every block of the scan as 64 int16 in zigzag order, blocks in scan order,
//                              dummy edge blocks resolved: 768 B per MCU.
//   jpeg_length_kernel         one wavefront per block, lane = zigzag position.  The ballot of the non-zero lanes gives
//                              every lane its zero run; a lane's token is its ZRLs + run/size code + amplitude bits (lane 0:
//                              DC category code + bits; lane 63, if zero: EOB).  A wave sum gives the block's bit count.
//   jpeg_offsets_kernel        one workgroup per frame: exclusive scan of the block bit counts, in place; the frame's total.
//                              It also zeroes the stream words that two pack workgroups share.
//   jpeg_pack_kernel           one workgroup per 16 consecutive blocks: the tokens again, ORed into an LDS window of the
//                              unstuffed stream (ds atomics), flushed as whole words -- plain stores for the words the
//                              workgroup owns, one global atomic OR for its first and its last word.
//   jpeg_ff_count_kernel       one workgroup per 4096 stream bytes: how many are 0xFF.
//   jpeg_ff_offsets_kernel     one workgroup per frame: exclusive scan of those counts; writes the frame's length, the
//                              623-byte header and EOI.
//   jpeg_stuff_kernel          one workgroup per 4096 stream bytes: copies them behind the header with a zero after each 0xFF.
//
// No workgroup waits for another one: every scan is either inside one workgroup or a launch of its own.  All combining is
// integer OR / integer sums of fixed operands, so the bytes do not depend on scheduling.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "jpeg_common.h"
#include "profile.h"

namespace vlfm {
namespace jpeg {

constexpr int kHeaderBytes = 623;
// The most bits one block can take: a DC code of at most 11 bits + 11 amplitude bits, and 63 AC coefficients each with a
// 16-bit run/size code + 10 amplitude bits (no ZRL fits between adjacent non-zero coefficients).
constexpr int kMaxBlockBits = 11 + 11 + 63 * (16 + 10);   // 1660
constexpr int GROUP = 16;                                 // blocks per pack workgroup
constexpr int WINDOW_WORDS = GROUP * kMaxBlockBits / 32 + 2 + 6;
constexpr int CHUNK = 4096;                               // stream bytes per stuffing workgroup: 256 threads x 16 B

struct HuffTables {
    uint32_t ac[2][256];   // code << 5 | length, by run/size symbol; luma, chroma
    uint32_t dc[2][12];    // by category
};
struct Header {
    uint32_t w[(kHeaderBytes + 3) / 4];   // the header's bytes, little-endian in each word
};

struct Layout {
    int n, nb;              // frames, blocks per frame: 6 * MCUs
    int groups, chunks;     // pack workgroups / stuffing workgroups (at the bound) per frame
    size_t stream_words;    // per frame
    size_t bits_off, meta_off, stream_off, ff_off, total;   // byte offsets into the scratch buffer; coefficients at 0
};

// ---------------------------------------------------------------------------------------------------------------- tokens
struct Token {
    uint64_t bits;   // right-aligned
    int len;         // 0: nothing to emit; at most 3 * 11 + 16 + 10 = 59
};

// jchuff.c encode_one_block for zigzag position `lane` of block j of a frame whose coefficients start at `cf`.
__device__ __forceinline__ Token block_token(const int16_t* __restrict__ cf, int j, int lane, const HuffTables& ht) {
    const int c = cf[(size_t)j * 64 + lane];
    const unsigned long long nz = __ballot(c != 0) | 1ull;   // position 0 ends every run
    const int k = j % 6, tab = k >= 4;
    Token t{0, 0};
    if (lane == 0) {
        // the previous block of the same component: Y00 follows the previous MCU's Y11, chroma its own six blocks back
        const int pj = k == 0 ? j - 3 : k < 4 ? j - 1 : j - 6;
        const int diff = c - (pj >= 0 ? (int)cf[(size_t)pj * 64] : 0);
        const int size = min(32 - __clz(abs(diff)), 11);
        const uint32_t e = ht.dc[tab][size];
        t.bits = (uint64_t)(e >> 5) << size | (uint32_t)((diff < 0 ? diff - 1 : diff) & ((1 << size) - 1));
        t.len = (int)(e & 31) + size;
    } else if (c != 0) {
        const unsigned long long below = nz & ((1ull << lane) - 1);
        const int run = lane - (63 - __clzll((long long)below)) - 1;
        const int size = 32 - __clz(abs(c));
        const uint32_t e = ht.ac[tab][(run & 15) << 4 | size];
        t.bits = (uint64_t)(e >> 5) << size | (uint32_t)((c < 0 ? c - 1 : c) & ((1 << size) - 1));
        t.len = (int)(e & 31) + size;
        const uint32_t zrl = ht.ac[tab][0xF0];
        for (int z = run >> 4; z > 0; --z) {
            t.bits |= (uint64_t)(zrl >> 5) << t.len;
            t.len += (int)(zrl & 31);
        }
    } else if (lane == 63) {
        const uint32_t e = ht.ac[tab][0];   // EOB
        t.bits = e >> 5;
        t.len = (int)(e & 31);
    }
    return t;
}

// Exclusive sum of v over the kThreads threads of the workgroup; *total gets the sum.  `part` holds kThreads / 64 words.
template <int kThreads>
__device__ __forceinline__ uint32_t block_exclusive_sum(uint32_t v, uint32_t* part, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = (uint32_t)wave_inclusive_sum((int)v, lane);
    __syncthreads();   // (part may still be read from an earlier call)
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const uint32_t p = part[w];
        before += w < wave ? p : 0;
        all += p;
    }
    *total = all;
    return before + incl - v;
}

__global__ void __launch_bounds__(256) jpeg_length_kernel(const int16_t* __restrict__ coef, HuffTables ht, int nb,
                                                          size_t blocks, uint32_t* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const size_t id = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (id >= blocks) return;
    const size_t f = id / nb;
    const int j = (int)(id - f * nb);
    const Token t = block_token(coef + f * nb * 64, j, lane, ht);
    const int incl = wave_inclusive_sum(t.len, lane);
    if (lane == 63) bits[id] = (uint32_t)incl;
}

__global__ void __launch_bounds__(1024) jpeg_offsets_kernel(uint32_t* __restrict__ bits, int nb, uint32_t* __restrict__ meta,
                                                            uint32_t* __restrict__ stream, size_t stream_words) {
    __shared__ uint32_t part[16];
    const int f = blockIdx.x, t = threadIdx.x;
    uint32_t* fb = bits + (size_t)f * nb;
    uint32_t* sw = stream + (size_t)f * stream_words;
    const int per = (nb + 1023) / 1024;
    const int i0 = min(t * per, nb), i1 = min(i0 + per, nb);
    uint32_t sum = 0;
    for (int i = i0; i < i1; ++i) sum += fb[i];
    uint32_t total;
    uint32_t off = block_exclusive_sum<1024>(sum, part, &total);
    for (int i = i0; i < i1; ++i) {
        const uint32_t b = fb[i];
        fb[i] = off;
        if (i % GROUP == 0) sw[off >> 5] = 0;   // the word a pack workgroup shares with the one before it
        off += b;
    }
    if (t == 0) {
        meta[f] = total;
        sw[total >> 5] = 0;
    }
}

__global__ void __launch_bounds__(256) jpeg_pack_kernel(const int16_t* __restrict__ coef, HuffTables ht, int nb, int groups,
                                                        const uint32_t* __restrict__ offs, const uint32_t* __restrict__ meta,
                                                        uint32_t* __restrict__ stream, size_t stream_words) {
    __shared__ uint32_t win[WINDOW_WORDS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int f = blockIdx.x / groups, gi = blockIdx.x - f * groups;
    const int j0 = gi * GROUP, j1 = min(j0 + GROUP, nb);
    const uint32_t* fo = offs + (size_t)f * nb;
    const uint32_t start = fo[j0], end = j1 < nb ? fo[j1] : meta[f];
    const uint32_t w0 = start >> 5;
    const int nw = min((int)((end >> 5) - w0) + 1, WINDOW_WORDS);
    for (int i = t; i < nw; i += 256) win[i] = 0;
    __syncthreads();
    const int16_t* cf = coef + (size_t)f * nb * 64;
    for (int j = j0 + wave; j < j1; j += 4) {
        const Token tk = block_token(cf, j, lane, ht);
        const int incl = wave_inclusive_sum(tk.len, lane);
        if (tk.len) {
            const uint32_t rel = fo[j] + (uint32_t)(incl - tk.len) - (w0 << 5);
            const int wi = (int)(rel >> 5), sh = (int)(rel & 31);
            const uint64_t left = tk.bits << (64 - tk.len);        // MSB first: left-aligned, then moved right by sh
            const uint64_t hi = left >> sh;
            const uint32_t a = (uint32_t)(hi >> 32), b = (uint32_t)hi;
            const uint32_t c = sh ? (uint32_t)((left << (64 - sh)) >> 32) : 0u;
            if (a && wi < nw) atomicOr(&win[wi], a);
            if (b && wi + 1 < nw) atomicOr(&win[wi + 1], b);
            if (c && wi + 2 < nw) atomicOr(&win[wi + 2], c);
        }
    }
    __syncthreads();
    uint32_t* sw = stream + (size_t)f * stream_words + w0;
    for (int i = t; i < nw; i += 256) {
        const uint32_t v = win[i];
        if (i == 0 || i == nw - 1) {
            if (v) atomicOr(&sw[i], v);
        } else {
            sw[i] = v;
        }
    }
}

// The 16 stream bytes [byte0, byte0 + 16) of a frame whose stream holds T bits: byte i is bits 8i .. 8i+7, MSB first, the
// last byte padded with 1-bits (jchuff.c flush_bits).  Returns how many of them exist (bytes at and past ceil(T/8) do not).
__device__ __forceinline__ int stream_bytes16(const uint32_t* __restrict__ sw, uint32_t byte0, uint32_t T, uint32_t* b) {
    const uint32_t U = (T + 7) >> 3;
    if (byte0 >= U) return 0;
    const uint4 v = *reinterpret_cast<const uint4*>(sw + (byte0 >> 2));
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const int n = (int)min(16u, U - byte0);
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = (w[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu;
    if ((T & 7) && byte0 + 16 >= U) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (byte0 + i == U - 1) b[i] |= 0xffu >> (T & 7);
    }
    return n;
}

__global__ void __launch_bounds__(256) jpeg_ff_count_kernel(const uint32_t* __restrict__ stream, size_t stream_words,
                                                            const uint32_t* __restrict__ meta, int chunks,
                                                            uint32_t* __restrict__ ffc) {
    __shared__ uint32_t part[4];
    const int f = blockIdx.x / chunks, c = blockIdx.x - f * chunks;
    const uint32_t T = meta[f];
    if ((uint32_t)c * CHUNK >= ((T + 7) >> 3)) return;
    uint32_t b[16];
    const int n = stream_bytes16(stream + (size_t)f * stream_words, (uint32_t)c * CHUNK + threadIdx.x * 16, T, b);
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) cnt += (i < n && b[i] == 0xffu) ? 1 : 0;
    uint32_t total;
    block_exclusive_sum<256>(cnt, part, &total);
    if (threadIdx.x == 0) ffc[(size_t)f * chunks + c] = total;
}

__global__ void __launch_bounds__(256) jpeg_ff_offsets_kernel(uint32_t* __restrict__ ffc, int chunks,
                                                              const uint32_t* __restrict__ meta, Header hdr,
                                                              uint8_t* __restrict__ out, size_t capacity,
                                                              uint32_t* __restrict__ lengths) {
    __shared__ uint32_t part[4];
    const int f = blockIdx.x, t = threadIdx.x;
    const uint32_t U = (meta[f] + 7) >> 3;
    const int nch = (int)((U + CHUNK - 1) / CHUNK);
    uint32_t* fc = ffc + (size_t)f * chunks;
    const int per = (nch + 255) / 256;
    const int i0 = min(t * per, nch), i1 = min(i0 + per, nch);
    uint32_t sum = 0;
    for (int i = i0; i < i1; ++i) sum += fc[i];
    uint32_t total;
    uint32_t off = block_exclusive_sum<256>(sum, part, &total);
    for (int i = i0; i < i1; ++i) {
        const uint32_t c = fc[i];
        fc[i] = off;
        off += c;
    }
    uint8_t* fo = out + (size_t)f * capacity;
    for (int i = t; i < kHeaderBytes; i += 256)
        if ((size_t)i < capacity) fo[i] = (uint8_t)(hdr.w[i >> 2] >> (8 * (i & 3)));
    if (t == 0) {
        const size_t eoi = (size_t)kHeaderBytes + U + total;
        if (eoi < capacity) fo[eoi] = 0xff;
        if (eoi + 1 < capacity) fo[eoi + 1] = 0xd9;
        lengths[f] = (uint32_t)(eoi + 2);
    }
}

__global__ void __launch_bounds__(256) jpeg_stuff_kernel(const uint32_t* __restrict__ stream, size_t stream_words,
                                                         const uint32_t* __restrict__ meta, int chunks,
                                                         const uint32_t* __restrict__ ffoff, uint8_t* __restrict__ out,
                                                         size_t capacity) {
    __shared__ uint32_t part[4];
    const int f = blockIdx.x / chunks, c = blockIdx.x - f * chunks;
    const uint32_t T = meta[f];
    if ((uint32_t)c * CHUNK >= ((T + 7) >> 3)) return;
    const uint32_t byte0 = (uint32_t)c * CHUNK + threadIdx.x * 16;
    uint32_t b[16];
    const int n = stream_bytes16(stream + (size_t)f * stream_words, byte0, T, b);
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) cnt += (i < n && b[i] == 0xffu) ? 1 : 0;
    uint32_t total;
    const uint32_t before = block_exclusive_sum<256>(cnt, part, &total);
    uint8_t* fo = out + (size_t)f * capacity;
    size_t p = (size_t)kHeaderBytes + byte0 + ffoff[(size_t)f * chunks + c] + before;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (i < n) {
            if (p < capacity) fo[p] = (uint8_t)b[i];
            ++p;
            if (b[i] == 0xffu) {
                if (p < capacity) fo[p] = 0;
                ++p;
            }
        }
    }
}

}  // namespace jpeg
}  // namespace vlfm

// ================================================================================================ host side, C ABI
using namespace vlfm;
using namespace vlfm::jpeg;

namespace {
// jcparam.c std_huff_tables (JPEG Annex K.3 - K.6): BITS[1..16], then HUFFVAL
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// jchuff.c jpeg_make_c_derived_tbl: codes of each length in increasing order, as the symbols are listed.
void derive(const uint8_t* bits, const uint8_t* vals, uint32_t* table) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) table[vals[k++]] = code++ << 5 | (uint32_t)len;
        code <<= 1;
    }
}

const HuffTables& huff_tables() {
    static const HuffTables tables = [] {
        HuffTables t;
        memset(&t, 0, sizeof t);
        derive(kAcLumaBits, kAcLumaVals, t.ac[0]);
        derive(kAcChromaBits, kAcChromaVals, t.ac[1]);
        derive(kDcLumaBits, kDcVals, t.dc[0]);
        derive(kDcChromaBits, kDcVals, t.dc[1]);
        return t;
    }();
    return tables;
}

// blocks per frame, or 0 where the encoder does not go: invalid sizes, and frames whose stream could pass 2^32 bits (bit
// offsets and lengths are 32-bit: about 10 000 x 10 000 pixels).
size_t frame_blocks(int H, int W) {
    Geometry g;
    if (!geometry(1, H, W, &g)) return 0;   // (one frame: only H and W are in question here)
    const size_t nb = 6 * g.mcus();
    return nb * kMaxBlockBits + 64 > 0xffffffffull ? 0 : nb;
}

bool layout(int n, int H, int W, Layout* l) {
    const size_t nb = frame_blocks(H, W);
    if (n <= 0 || nb == 0) return false;
    l->n = n;
    l->nb = (int)nb;
    l->groups = (int)((nb + GROUP - 1) / GROUP);
    const size_t stream_bytes = (nb * kMaxBlockBits + 7) / 8;
    l->chunks = (int)((stream_bytes + CHUNK - 1) / CHUNK);
    l->stream_words = align16(stream_bytes + 4 + 16) / 4;   // + the word at total >> 5, + a whole 16-byte load at the end
    l->bits_off = align16((size_t)n * nb * 128);
    l->meta_off = l->bits_off + align16((size_t)n * nb * 4);
    l->stream_off = l->meta_off + align16((size_t)n * 4);
    l->ff_off = l->stream_off + (size_t)n * l->stream_words * 4;
    l->total = l->ff_off + align16((size_t)n * l->chunks * 4);
    return true;
}

void put_segment(uint8_t*& p, int marker, const uint8_t* payload, int len) {
    *p++ = 0xff;
    *p++ = (uint8_t)marker;
    *p++ = (uint8_t)((len + 2) >> 8);
    *p++ = (uint8_t)(len + 2);
    memcpy(p, payload, len);
    p += len;
}

// jcmarker.c write_file_header / write_frame_header / write_scan_header for a 3-component 4:2:0 baseline frame.
void make_header(const uint16_t* tables, int H, int W, uint8_t* out) {
    uint8_t* p = out;
    *p++ = 0xff;
    *p++ = 0xd8;
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    put_segment(p, 0xe0, jfif, 14);
    for (int t = 0; t < 2; ++t) {
        uint8_t dqt[65];
        dqt[0] = (uint8_t)t;
        for (int i = 0; i < 64; ++i) dqt[1 + i] = (uint8_t)tables[64 * t + kNaturalOrder[i]];
        put_segment(p, 0xdb, dqt, 65);
    }
    const uint8_t sof[15] = {8, (uint8_t)(H >> 8), (uint8_t)H, (uint8_t)(W >> 8), (uint8_t)W, 3, 1, 0x22, 0, 2, 0x11, 1,
                             3, 0x11, 1};
    put_segment(p, 0xc0, sof, 15);
    const struct { int id; const uint8_t* bits; const uint8_t* vals; int n; } dht[4] = {
        {0x00, kDcLumaBits, kDcVals, 12}, {0x10, kAcLumaBits, kAcLumaVals, 162},
        {0x01, kDcChromaBits, kDcVals, 12}, {0x11, kAcChromaBits, kAcChromaVals, 162}};
    for (const auto& d : dht) {
        uint8_t seg[1 + 16 + 162];
        seg[0] = (uint8_t)d.id;
        memcpy(seg + 1, d.bits, 16);
        memcpy(seg + 17, d.vals, d.n);
        put_segment(p, 0xc4, seg, 17 + d.n);
    }
    const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    put_segment(p, 0xda, sos, 10);
}
}  // namespace

extern "C" int vlfm_jpeg_header_host(int quality, int H, int W, uint8_t* h_out, size_t cap, size_t* len) {
    uint16_t tables[128];
    Geometry g;
    if (!h_out || !len || !geometry(1, H, W, &g))   // (one frame: g only checks H and W)
        return fail(VLFM_ERR_INVALID, "jpeg_header_host: bad argument");
    if (int rc = vlfm_jpeg_quant_tables_host(quality, tables)) return rc;
    *len = kHeaderBytes;
    if (cap < (size_t)kHeaderBytes) return fail(VLFM_ERR_CAPACITY, "jpeg_header_host: the header takes 623 bytes");
    make_header(tables, H, W, h_out);
    return VLFM_OK;
}

extern "C" size_t vlfm_jpeg_encode_bound(int H, int W) {
    const size_t nb = frame_blocks(H, W);
    return nb ? (size_t)kHeaderBytes + 2 * ((nb * kMaxBlockBits + 7) / 8) + 2 : 0;
}

extern "C" size_t vlfm_jpeg_encode_scratch_bytes(int n, int H, int W) {
    Layout l;
    return layout(n, H, W, &l) ? l.total : 0;
}

extern "C" int vlfm_jpeg_encode_batched(const uint8_t* d_in, int n, int H, int W, int rgb_order, const uint16_t* h_tables,
                                        uint8_t* d_out, size_t capacity, uint32_t* d_lengths, void* d_scratch,
                                        size_t scratch_bytes, void* stream) {
    Layout l;
    QuantTables qt;
    if (!d_in || !d_out || !d_lengths || !h_tables || capacity == 0 || (rgb_order != 0 && rgb_order != 1))
        return fail(VLFM_ERR_INVALID, "jpeg_encode_batched: bad argument");
    if (!layout(n, H, W, &l))
        return fail(VLFM_ERR_INVALID, "jpeg_encode_batched: bad frame size (or a frame too large for 32-bit bit offsets)");
    if (!load_quant_tables(h_tables, &qt))
        return fail(VLFM_ERR_INVALID, "jpeg_encode_batched: quantisation table entries must be 1..255");
    if (!d_scratch || (reinterpret_cast<uintptr_t>(d_scratch) & 15))
        return fail(VLFM_ERR_INVALID, "jpeg_encode_batched: scratch must be a 16-byte aligned device buffer");
    if (scratch_bytes < l.total) return fail(VLFM_ERR_CAPACITY, "jpeg_encode_batched: scratch too small");
    const size_t blocks = (size_t)n * l.nb;
    const size_t length_grid = (blocks + 3) / 4, pack_grid = (size_t)n * l.groups, stuff_grid = (size_t)n * l.chunks;
    if (length_grid > 0x7fffffff || pack_grid > 0x7fffffff || stuff_grid > 0x7fffffff)
        return fail(VLFM_ERR_INVALID, "jpeg_encode_batched: batch too large for one launch");

    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    int16_t* coef = reinterpret_cast<int16_t*>(base);
    uint32_t* bits = reinterpret_cast<uint32_t*>(base + l.bits_off);
    uint32_t* meta = reinterpret_cast<uint32_t*>(base + l.meta_off);
    uint32_t* strm = reinterpret_cast<uint32_t*>(base + l.stream_off);
    uint32_t* ffc = reinterpret_cast<uint32_t*>(base + l.ff_off);
    hipStream_t st = (hipStream_t)stream;
    const HuffTables& ht = huff_tables();
    Header hdr;
    memset(&hdr, 0, sizeof hdr);
    make_header(h_tables, H, W, reinterpret_cast<uint8_t*>(hdr.w));   // (little-endian host: byte i of the word array)

    if (int rc = launch_coefficients(d_in, n, H, W, rgb_order, qt, coef, st)) return rc;
    {
        VLFM_TIMED("jpeg_length_kernel", st);
        VLFM_KLAUNCH(jpeg_length_kernel, dim3((unsigned)length_grid), dim3(256), 0, st, coef, ht, l.nb, blocks, bits);
    }
    if (int rc = check_launch("jpeg_length_kernel")) return rc;
    {
        VLFM_TIMED("jpeg_offsets_kernel", st);
        VLFM_KLAUNCH(jpeg_offsets_kernel, dim3((unsigned)n), dim3(1024), 0, st, bits, l.nb, meta, strm, l.stream_words);
    }
    if (int rc = check_launch("jpeg_offsets_kernel")) return rc;
    {
        VLFM_TIMED("jpeg_pack_kernel", st);
        VLFM_KLAUNCH(jpeg_pack_kernel, dim3((unsigned)pack_grid), dim3(256), 0, st, coef, ht, l.nb, l.groups, bits, meta,
                     strm, l.stream_words);
    }
    if (int rc = check_launch("jpeg_pack_kernel")) return rc;
    {
        VLFM_TIMED("jpeg_ff_count_kernel", st);
        VLFM_KLAUNCH(jpeg_ff_count_kernel, dim3((unsigned)stuff_grid), dim3(256), 0, st, strm, l.stream_words, meta,
                     l.chunks, ffc);
    }
    if (int rc = check_launch("jpeg_ff_count_kernel")) return rc;
    {
        VLFM_TIMED("jpeg_ff_offsets_kernel", st);
        VLFM_KLAUNCH(jpeg_ff_offsets_kernel, dim3((unsigned)n), dim3(256), 0, st, ffc, l.chunks, meta, hdr, d_out, capacity,
                     d_lengths);
    }
    if (int rc = check_launch("jpeg_ff_offsets_kernel")) return rc;
    {
        VLFM_TIMED("jpeg_stuff_kernel", st);
        VLFM_KLAUNCH(jpeg_stuff_kernel, dim3((unsigned)stuff_grid), dim3(256), 0, st, strm, l.stream_words, meta, l.chunks,
                     ffc, d_out, capacity);
    }
    return check_launch("jpeg_stuff_kernel");
}
