// jpeg_codec.hip -- gfx950 round trip of a batch of frames through baseline 4:2:0 JPEG at quality q: encode, then decode,
// bit-exact to libjpeg-turbo as Pillow drives it (the reference's client -> server transport, vlfm/vlm/server_wrapper.py:57-68,
// restated on the host by vlfm_amd/vlm/transport.py:jpeg_roundtrip).  Huffman coding is lossless, so only the quantised DCT
// coefficients decide the decoded frame; they never leave the workgroup that makes them.
//
// Two kernels per call, frames [n][H][W][3] uint8 packed back to back (slot 2 = R, slot 0 = B, as cv2.imencode reads an RGB
// frame):
//
//   jpeg_code_kernel      one 192-thread workgroup per 16 x 64 pixel tile (one MCU row of 4 MCUs = 16 luma + 4 Cb + 4 Cr
//                         blocks).  16 B/lane loads of the tile's interleaved rows into LDS (edge columns and rows
//                         replicated), colour conversion and 2x2 downsampling, islow FDCT rows -> LDS -> FDCT columns,
//                         quantise, dequantise and islow IDCT columns in the same registers -> LDS -> IDCT rows, range
//                         limit.  Decoded Y, Cb, Cr samples go to the scratch planes.
//   jpeg_upsample_kernel  one thread per 16-pixel output run: h2v2 fancy chroma upsampling and YCbCr -> RGB, 3 x 16 B stores.
//
// The encoder (jpeg_entropy.hip) uses jpeg_code_kernel<true, *>: the same kernel stopped after quantisation, storing the
// quantised coefficients of every block of the scan instead of decoding them.
//
// Upsampling output rows 16k-1 and 16k needs a decoded chroma row of the neighbouring MCU row; the plane pass makes that a
// read of the scratch plane instead of a recomputed halo (why, and what the planes cost in bytes).
//
// Each step restates a libjpeg-turbo routine (tests/jpeg_ref.py is the NumPy form, held to Pillow):
//   jccolor.c rgb_ycc_convert, jcsample.c fullsize_downsample / h2v2_downsample, jcprepct.c edge padding, jfdctint.c
//   jpeg_fdct_islow, jcdctmgr.c quantize, jidctint.c jpeg_idct_islow, jdmaster.c range-limit table, jdsample.c
//   h2v2_fancy_upsample / h2v2_upsample, jdcolor.c ycc_rgb_convert.
//
// int32 is enough.  Every pre-descale value of a transform is, up to the rounding of the earlier pass, a linear form in its
// block's 64 inputs.  FDCT: inputs are level-shifted samples, |x| <= 128, and the largest L1 norm of any intermediate form
// (column pass, including the row pass's scaling) is 2.69e6 (kFdctFormL1), so |v| <= 3.5e8 + rounding < 2^29.  IDCT: by
// Parseval the orthonormal DCT of a block has Euclidean norm <= 8 * 128 = 1024; dequantising moves each of the 64
// coefficients by at most qtab/2 <= 127.5, i.e. by at most 8 * 127.5 = 1020 in Euclidean norm, so the dequantised block has
// norm <= 2044 (+ < 1 of FDCT rounding).  The largest Euclidean norm of any intermediate IDCT form over the 64 dequantised
// inputs (row pass, including the column pass's descale) is 3.36e5 (kIdctFormNorm), so |v| <= 3.36e5 * 2045 + rounding
// < 7e8 < 2^30.  (The largest value met on worst-case sign-pattern blocks at q = 1, 90 and 100 was 2.47e8.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_common.h"
#include "profile.h"

namespace vlfm {
namespace jpeg {

constexpr double kFdctFormL1 = 2.69e6, kIdctFormNorm = 3.36e5;
// (the rounding slack: < 1 per element of the earlier pass, times the largest L1 norm of a form over that pass: < 2^21)
static_assert(kFdctFormL1 * 128.0 + (1 << 21) < 2147483647.0, "islow FDCT intermediates must fit in int32");
static_assert(kIdctFormNorm * 2045.0 + (1 << 21) < 2147483647.0, "islow IDCT intermediates must fit in int32");

constexpr int CSTRIDE = 9;                   // LDS coefficient row stride (ints): rows of a block on different banks
constexpr int CBLOCK = 8 * CSTRIDE;
static_assert(THREADS == 16 * TILE_ROW_BYTES / 16, "one 16-byte load per thread fills the tile");

// jccolor.c / jdcolor.c: FIX(x) = (INT32)(x * (1 << 16) + 0.5), ONE_HALF = 1 << 15, CBCR_OFFSET = 128 << 16
constexpr int fix16(double x) { return (int)(x * 65536.0 + 0.5); }
constexpr int ONE_HALF = 1 << 15;
constexpr int CBCR_OFFSET = 128 << 16;

// jfdctint.c / jidctint.c (CONST_BITS 13, PASS1_BITS 2)
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633;
constexpr int F1501 = 12299, F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One 8-point pass of jpeg_fdct_islow.  Pass 1 (rows): even outputs << PASS1_BITS, others descaled by CONST-PASS1.
// Pass 2 (columns): even outputs descaled by PASS1_BITS, others by CONST+PASS1.
template <bool kPass1>
__device__ __forceinline__ void fdct8(int* d) {
    constexpr int kOdd = kPass1 ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7];
    int tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5];
    int tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3;
    int tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (kPass1) {
        d[0] = (tmp10 + tmp11) * (1 << PASS1_BITS);
        d[4] = (tmp10 - tmp11) * (1 << PASS1_BITS);
    } else {
        d[0] = descale(tmp10 + tmp11, PASS1_BITS);
        d[4] = descale(tmp10 - tmp11, PASS1_BITS);
    }
    int z1 = (tmp12 + tmp13) * F0541;
    d[2] = descale(z1 + tmp13 * F0765, kOdd);
    d[6] = descale(z1 - tmp12 * F1847, kOdd);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    int z5 = (z3 + z4) * F1175;
    tmp4 *= F0298; tmp5 *= F2053; tmp6 *= F3072; tmp7 *= F1501;
    z1 *= -F0899; z2 *= -F2562; z3 = z3 * -F1961 + z5; z4 = z4 * -F0390 + z5;
    d[7] = descale(tmp4 + z1 + z3, kOdd);
    d[5] = descale(tmp5 + z2 + z4, kOdd);
    d[3] = descale(tmp6 + z2 + z3, kOdd);
    d[1] = descale(tmp7 + z1 + z4, kOdd);
}

// One 8-point pass of jpeg_idct_islow with the final descale by kShift (pass 1: CONST-PASS1 = 11; pass 2: CONST+PASS1+3 =
// 18).  The C code's all-AC-zero shortcuts give the same values as this full form.
template <int kShift>
__device__ __forceinline__ void idct8(int* x) {
    int z1 = (x[2] + x[6]) * F0541;
    int tmp2 = z1 - x[6] * F1847;
    int tmp3 = z1 + x[2] * F0765;
    int tmp0 = (x[0] + x[4]) * (1 << CONST_BITS);
    int tmp1 = (x[0] - x[4]) * (1 << CONST_BITS);
    int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3;
    int tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    int z5 = (z3 + z4) * F1175;
    t0 *= F0298; t1 *= F2053; t2 *= F3072; t3 *= F1501;
    z1 *= -F0899; z2 *= -F2562; z3 = z3 * -F1961 + z5; z4 = z4 * -F0390 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    x[0] = descale(tmp10 + t3, kShift);
    x[7] = descale(tmp10 - t3, kShift);
    x[1] = descale(tmp11 + t2, kShift);
    x[6] = descale(tmp11 - t2, kShift);
    x[2] = descale(tmp12 + t1, kShift);
    x[5] = descale(tmp12 - t1, kShift);
    x[3] = descale(tmp13 + t0, kShift);
    x[4] = descale(tmp13 - t0, kShift);
}

// jdmaster.c prepare_range_limit_table, the post-IDCT part indexed by x & 1023.
__device__ __forceinline__ uint32_t range_limit(int x) {
    int j = x & 1023;
    return (uint32_t)(j < 128 ? j + 128 : j < 512 ? 255 : j < 896 ? 0 : j - 896);
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// kEncode = false: the round trip (decoded planes to `scratch`).  kEncode = true: the encoder's coefficient pass, which
// stops after quantisation and stores every block of the scan as 64 int16 in zigzag order, blocks in scan order (MCUs
// row-major; Y00 Y01 Y10 Y11 Cb Cr), to `scratch`; kRgb then reads slot 0 of a pixel as R instead of slot 2.
template <bool kEncode, bool kRgb>
__global__ void __launch_bounds__(THREADS) jpeg_code_kernel(const uint8_t* __restrict__ in, QuantTables qt, Geometry g,
                                                            uint8_t* __restrict__ scratch) {
    __shared__ uint4 px4[16 * TILE_ROW_BYTES / 16];   // 16 interleaved sample rows of the tile
    __shared__ int coef[BLOCKS * CBLOCK];
    __shared__ int qdiv[2][64];
    __shared__ float qrcp[2][64];

    const int t = threadIdx.x;
    const int per_frame = g.mh * g.tiles_x;
    const int f = blockIdx.x / per_frame;
    const int rem = blockIdx.x - f * per_frame;
    const int m = rem / g.tiles_x;
    const int x0 = (rem - m * g.tiles_x) * TILE_W;
    const int y0 = m * 16;
    const size_t row_bytes = (size_t)3 * g.W;
    const uint8_t* frame = in + (size_t)f * g.H * row_bytes;

    if (t < 128) {
        const int d = (int)qt.q[t >> 6][t & 63] << 3;
        qdiv[t >> 6][t & 63] = d;
        qrcp[t >> 6][t & 63] = 1.0f / (float)d;
    }
    // ---- load: tile row lr, 16-byte chunk k.  Rows past H replicate row H-1 (jcprepct.c expand_bottom_edge), columns
    // past W replicate column W-1 (jcsample.c expand_right_edge).
    {
        const int lr = t / 12, k = t - lr * 12;
        const uint8_t* src = frame + (size_t)min(y0 + lr, g.H - 1) * row_bytes;
        if (g.vec_in && x0 + TILE_W <= g.W) {
            px4[t] = *reinterpret_cast<const uint4*>(src + 3 * x0 + 16 * k);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int e = 16 * k + j, p = e / 3, c = e - 3 * p;
                w[j >> 2] |= (uint32_t)src[3 * min(x0 + p, g.W - 1) + c] << (8 * (j & 3));
            }
            px4[t] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    __syncthreads();

    const uint32_t* pxw = reinterpret_cast<const uint32_t*>(px4);
    const int b = t >> 3, r = t & 7;   // block, row of the block
    int v[8];
    if (b < 16) {
        // jccolor.c rgb_ycc_convert, Y only (waves 0 and 1); jcsample.c fullsize_downsample copies it
        const int lrow = (b >> 3) * 8 + r, bc = b & 7;
        uint32_t w[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i] = pxw[(lrow * TILE_ROW_BYTES + bc * 24) / 4 + i];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int B = byte_of(w, 3 * i + (kRgb ? 2 : 0)), G = byte_of(w, 3 * i + 1);
            const int R = byte_of(w, 3 * i + (kRgb ? 0 : 2));
            v[i] = ((fix16(0.299) * R + fix16(0.587) * G + fix16(0.114) * B + ONE_HALF) >> 16) - 128;
        }
    } else {
        // Cb (blocks 16..19) and Cr (20..23) in wave 2: jccolor.c, then jcsample.c h2v2_downsample: 2x2 sums plus a bias
        // alternating 1, 2 along the row, >> 2.  Chroma rows past the real chroma height ceil(H/2) replicate its last row
        // (jcprepct.c pads the downsampled component).
        const int u = b - 16, plane = u >> 2, bc = u & 3;
        const int cr_r = plane ? fix16(0.5) : -fix16(0.16874);
        const int cr_g = plane ? -fix16(0.41869) : -fix16(0.33126);
        const int cr_b = plane ? -fix16(0.08131) : fix16(0.5);
        const int li = min(r, g.ch - 1 - 8 * m);
        int s[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = (i & 1) ? 2 : 1;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            uint32_t w[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) w[i] = pxw[((2 * li + rr) * TILE_ROW_BYTES + bc * 48) / 4 + i];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int B = byte_of(w, 3 * i + (kRgb ? 2 : 0)), G = byte_of(w, 3 * i + 1);
                const int R = byte_of(w, 3 * i + (kRgb ? 0 : 2));
                s[i >> 1] += (cr_r * R + cr_g * G + cr_b * B + CBCR_OFFSET + ONE_HALF - 1) >> 16;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (s[i] >> 2) - 128;
    }
    fdct8<true>(v);
    int* cb = coef + b * CBLOCK;
#pragma unroll
    for (int i = 0; i < 8; ++i) cb[r * CSTRIDE + i] = v[i];
    __syncthreads();

    // ---- column c = r of block b: FDCT pass 2, jcdctmgr.c quantize (divide by qtab << 3, round half away from zero),
    // dequantise (jddctmgr.c: coef * quantval), IDCT pass 1 (columns) -- all in registers.
    {
        const int c = r, tab = b < 16 ? 0 : 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = cb[i * CSTRIDE + c];
        fdct8<false>(v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int d = qdiv[tab][i * 8 + c];
            const int num = abs(v[i]) + (d >> 1);
            int q = (int)((float)num * qrcp[tab][i * 8 + c]);   // off by at most one (num < 2^18): corrected below
            const int rest = num - q * d;
            q += rest < 0 ? -1 : rest >= d ? 1 : 0;
            v[i] = (v[i] < 0 ? -q : q) * (kEncode ? 1 : d >> 3);
        }
        if (!kEncode) idct8<CONST_BITS - PASS1_BITS>(v);
#pragma unroll
        for (int i = 0; i < 8; ++i) cb[i * CSTRIDE + c] = v[i];
    }
    __syncthreads();

    if (kEncode) {
        // ---- zigzag positions 8r .. 8r+7 of block b: one 16-byte store.  jccoefct.c compress_data: a luma block past the
        // last real block column ceil(W/8) or row ceil(H/8) is a dummy -- AC all zero, DC that of the block coded just
        // before it in its MCU (itself possibly a dummy; the first block of an MCU is always real).
        const int u = b < 16 ? (b & 7) >> 1 : (b - 16) & 3;            // MCU of the tile
        const int mx = x0 / 16 + u;
        if (mx >= g.mw) return;
        const int k = b < 16 ? (b >> 3) * 2 + (b & 1) : 4 + ((b - 16) >> 2);
        const int bh = (g.H + 7) >> 3, bw = (g.W + 7) >> 3;
        int src = k;
        if (b < 16)
            while (src > 0 && (2 * m + (src >> 1) >= bh || 2 * mx + (src & 1) >= bw)) --src;
        const int* sb = src == k ? cb : coef + ((src >> 1) * 8 + 2 * u + (src & 1)) * CBLOCK;
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int nat = kNaturalOrder[8 * r + j];
            int c = sb[(nat >> 3) * CSTRIDE + (nat & 7)];
            if (src != k && 8 * r + j > 0) c = 0;
            if (j & 1) w[j >> 1] |= (uint32_t)(c & 0xffff) << 16;
            else w[j >> 1] = (uint32_t)(c & 0xffff);
        }
        int16_t* dst = reinterpret_cast<int16_t*>(scratch) +
                       ((((size_t)f * g.mh + m) * g.mw + mx) * 6 + k) * 64 + 8 * r;
        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    // ---- row r of block b: IDCT pass 2, range limit, 8 samples to the scratch plane.
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = cb[r * CSTRIDE + i];
    idct8<CONST_BITS + PASS1_BITS + 3>(v);
    uint2 o;
    o.x = range_limit(v[0]) | range_limit(v[1]) << 8 | range_limit(v[2]) << 16 | range_limit(v[3]) << 24;
    o.y = range_limit(v[4]) | range_limit(v[5]) << 8 | range_limit(v[6]) << 16 | range_limit(v[7]) << 24;
    uint8_t* fs = scratch + (size_t)f * g.frame_scratch();
    if (b < 16) {
        const int col = x0 + (b & 7) * 8, ys = 16 * g.mw;
        if (col < ys) *reinterpret_cast<uint2*>(fs + (size_t)(y0 + (b >> 3) * 8 + r) * ys + col) = o;
    } else {
        const int u = b - 16, col = x0 / 2 + (u & 3) * 8, cs = 8 * g.mw;
        uint8_t* plane = fs + (size_t)256 * g.mh * g.mw + (size_t)(u >> 2) * 64 * g.mh * g.mw;
        if (col < cs) *reinterpret_cast<uint2*>(plane + (size_t)(8 * m + r) * cs + col) = o;
    }
}

// The decoder's second half (jpeg_decode.hip calls it): the coefficient buffer of a decoded scan -- the layout
// jpeg_code_kernel<true, *> writes -- times the frame's own quantisation tables (jddctmgr.c: coef * quantval), through the
// same IDCT columns and rows, to the decoded planes.  Same grid and thread roles as jpeg_code_kernel.
__global__ void __launch_bounds__(THREADS) jpeg_idct_kernel(const int16_t* __restrict__ coef,
                                                            const vlfm_jpeg_frame* __restrict__ frames,
                                                            const vlfm_jpeg_table_set* __restrict__ sets, int n_sets,
                                                            Geometry g, uint8_t* __restrict__ planes) {
    __shared__ int cblk[BLOCKS * CBLOCK];
    const int t = threadIdx.x;
    const int per_frame = g.mh * g.tiles_x;
    const int f = blockIdx.x / per_frame;
    const int rem = blockIdx.x - f * per_frame;
    const int m = rem / g.tiles_x;
    const int x0 = (rem - m * g.tiles_x) * TILE_W;
    const int b = t >> 3, r = t & 7;
    const int u = b < 16 ? (b & 7) >> 1 : (b - 16) & 3;            // MCU of the tile
    const int mx = x0 / 16 + u;
    const int k = b < 16 ? (b >> 3) * 2 + (b & 1) : 4 + ((b - 16) >> 2);
    const int set = min(max(frames[f].table_set, 0), n_sets - 1);
    const uint16_t* q = sets[set].quant[b < 16 ? 0 : k - 3];
    int* cb = cblk + b * CBLOCK;
    // zigzag positions 8r .. 8r+7 of block b: one 16-byte load, dequantised into their natural places
    uint4 w = make_uint4(0, 0, 0, 0);
    if (mx < g.mw)
        w = *reinterpret_cast<const uint4*>(coef + ((((size_t)f * g.mh + m) * g.mw + mx) * 6 + k) * 64 + 8 * r);
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int nat = kNaturalOrder[8 * r + j];
        const int c = (int)(int16_t)(ww[j >> 1] >> (16 * (j & 1)));
        cb[(nat >> 3) * CSTRIDE + (nat & 7)] = c * (int)q[nat];
    }
    __syncthreads();
    int v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = cb[i * CSTRIDE + r];
    idct8<CONST_BITS - PASS1_BITS>(v);
#pragma unroll
    for (int i = 0; i < 8; ++i) cb[i * CSTRIDE + r] = v[i];
    __syncthreads();
    // row r of block b, as in jpeg_code_kernel: IDCT pass 2, range limit, 8 samples to the decoded planes
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = cb[r * CSTRIDE + i];
    idct8<CONST_BITS + PASS1_BITS + 3>(v);
    uint2 o;
    o.x = range_limit(v[0]) | range_limit(v[1]) << 8 | range_limit(v[2]) << 16 | range_limit(v[3]) << 24;
    o.y = range_limit(v[4]) | range_limit(v[5]) << 8 | range_limit(v[6]) << 16 | range_limit(v[7]) << 24;
    uint8_t* fs = planes + (size_t)f * g.frame_scratch();
    if (b < 16) {
        const int col = x0 + (b & 7) * 8, ys = 16 * g.mw;
        if (col < ys) *reinterpret_cast<uint2*>(fs + (size_t)(16 * m + (b >> 3) * 8 + r) * ys + col) = o;
    } else {
        const int col = x0 / 2 + u * 8, cs = 8 * g.mw;
        uint8_t* plane = fs + (size_t)256 * g.mh * g.mw + (size_t)(k - 4) * 64 * g.mh * g.mw;
        if (col < cs) *reinterpret_cast<uint2*>(plane + (size_t)(8 * m + r) * cs + col) = o;
    }
}

// Ten chroma samples, columns j0-1 .. j0+8 clamped to the real width [0, cw) (the clamp is how h2v2_fancy_upsample's
// first and last outputs treat the edge: the missing neighbour is the sample itself).
__device__ __forceinline__ void load10(const uint8_t* row, int j0, int cw, int* v) {
    if (j0 >= 1 && j0 + 9 <= cw) {
        const uint2 mid = *reinterpret_cast<const uint2*>(row + j0);
        v[0] = row[j0 - 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[1 + i] = (mid.x >> (8 * i)) & 0xff;
            v[5 + i] = (mid.y >> (8 * i)) & 0xff;
        }
        v[9] = row[j0 + 8];
    } else {
#pragma unroll
        for (int i = 0; i < 10; ++i) v[i] = row[min(max(j0 - 1 + i, 0), cw - 1)];
    }
}

// jdsample.c for output pixel p (0..15) of a run whose chroma columns start at j0: fancy (3*s + s_side + 8 or 7) >> 4 on
// the column sums s, or plain replication (h2v2_upsample) when the component is at most 2 samples wide.
__device__ __forceinline__ int upsample_px(const int* s, const int* raw, int p, bool fancy) {
    const int t = (p >> 1) + 1;
    if (!fancy) return raw[t];
    return (p & 1) ? (3 * s[t] + s[t + 1] + 7) >> 4 : (3 * s[t] + s[t - 1] + 8) >> 4;
}

// kRgb = false: slot 0 = B, 2 = R (the round trip's order, what cv2.imdecode returns); true: slot 0 = R.
template <bool kRgb>
__global__ void __launch_bounds__(256) jpeg_upsample_kernel(const uint8_t* __restrict__ scratch, Geometry g,
                                                            uint8_t* __restrict__ out) {
    const int runs = (g.W + 15) >> 4;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (size_t)g.n * g.H * runs) return;
    const int k = (int)(gid % runs);
    const size_t fy = gid / runs;
    const int y = (int)(fy % g.H), f = (int)(fy / g.H);
    const int x0 = 16 * k, j0 = 8 * k;
    const uint8_t* fs = scratch + (size_t)f * g.frame_scratch();
    const int ys = 16 * g.mw, cs = 8 * g.mw;
    const uint4 yv = *reinterpret_cast<const uint4*>(fs + (size_t)y * ys + x0);
    const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};

    const int i = y >> 1, i2 = (y & 1) ? min(i + 1, g.ch - 1) : max(i - 1, 0);
    const bool fancy = g.cw > 2;   // jdsample.c jinit_upsampler: do_fancy && downsampled_width > 2
    int cbs[10], crs[10], cb0[10], cr0[10];
    {
        const uint8_t* cbp = fs + (size_t)256 * g.mh * g.mw;
        const uint8_t* crp = cbp + (size_t)64 * g.mh * g.mw;
        int nb[10];
        load10(cbp + (size_t)i * cs, j0, g.cw, cb0);
        load10(cbp + (size_t)i2 * cs, j0, g.cw, nb);
#pragma unroll
        for (int q = 0; q < 10; ++q) cbs[q] = 3 * cb0[q] + nb[q];
        load10(crp + (size_t)i * cs, j0, g.cw, cr0);
        load10(crp + (size_t)i2 * cs, j0, g.cw, nb);
#pragma unroll
        for (int q = 0; q < 10; ++q) crs[q] = 3 * cr0[q] + nb[q];
    }
    uint32_t ow[12] = {};
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        // jdcolor.c ycc_rgb_convert, clamped (range_limit of the simple table)
        const int Y = (yw[p >> 2] >> (8 * (p & 3))) & 0xff;
        const int xcb = upsample_px(cbs, cb0, p, fancy) - 128, xcr = upsample_px(crs, cr0, p, fancy) - 128;
        const int R = min(max(Y + ((fix16(1.402) * xcr + ONE_HALF) >> 16), 0), 255);
        const int B = min(max(Y + ((fix16(1.772) * xcb + ONE_HALF) >> 16), 0), 255);
        const int G = min(max(Y + ((-fix16(0.34414) * xcb + ONE_HALF - fix16(0.71414) * xcr) >> 16), 0), 255);
        const int e = 3 * p;   // slot 0 = B, 1 = G, 2 = R (kRgb: 0 = R, 2 = B)
        ow[e >> 2] |= (uint32_t)(kRgb ? R : B) << (8 * (e & 3));
        ow[(e + 1) >> 2] |= (uint32_t)G << (8 * ((e + 1) & 3));
        ow[(e + 2) >> 2] |= (uint32_t)(kRgb ? B : R) << (8 * ((e + 2) & 3));
    }
    uint8_t* dst = out + ((size_t)f * g.H + y) * 3 * g.W + 3 * x0;
    if (g.vec_out && x0 + 16 <= g.W) {
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        d4[0] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        d4[1] = make_uint4(ow[4], ow[5], ow[6], ow[7]);
        d4[2] = make_uint4(ow[8], ow[9], ow[10], ow[11]);
    } else {
        const int nb = 3 * min(16, g.W - x0);
#pragma unroll
        for (int e = 0; e < 48; ++e)
            if (e < nb) dst[e] = (uint8_t)(ow[e >> 2] >> (8 * (e & 3)));
    }
}

// The encoder's coefficient pass (jpeg_entropy.hip calls it): 768 bytes per MCU to d_coef.
int launch_coefficients(const uint8_t* d_in, int n, int H, int W, int rgb_order, const QuantTables& qt, int16_t* d_coef,
                        hipStream_t st) {
    Geometry g;
    if (!geometry(n, H, W, &g, d_in) || g.code_grid() > 0x7fffffff)   // (the entry point has validated the size)
        return fail(VLFM_ERR_INVALID, "jpeg_encode_batched: batch too large for one launch");
    auto kernel = rgb_order ? jpeg_code_kernel<true, true> : jpeg_code_kernel<true, false>;
    {
        VLFM_TIMED("jpeg_coef_kernel", st);
        VLFM_KLAUNCH(kernel, dim3((unsigned)g.code_grid()), dim3(THREADS), 0, st, d_in, qt, g,
                     reinterpret_cast<uint8_t*>(d_coef));
    }
    return check_launch("jpeg_coef_kernel");
}

// The decoder's pixel half (jpeg_decode.hip calls it): coefficients -> decoded planes -> frames.
int launch_pixels(const int16_t* d_coef, const vlfm_jpeg_frame* d_frames, const vlfm_jpeg_table_set* d_sets, int n_sets, int n,
                  int H, int W, int rgb_order, uint8_t* d_planes, uint8_t* d_out, hipStream_t st) {
    Geometry g;
    // (the entry point has validated the size)
    if (!geometry(n, H, W, &g, nullptr, d_out) || g.code_grid() > 0x7fffffff || g.upsample_grid() > 0x7fffffff)
        return fail(VLFM_ERR_INVALID, "jpeg_decode_batched: batch too large for one launch");
    {
        VLFM_TIMED("jpeg_idct_kernel", st);
        VLFM_KLAUNCH(jpeg_idct_kernel, dim3((unsigned)g.code_grid()), dim3(THREADS), 0, st, d_coef, d_frames, d_sets, n_sets,
                     g, d_planes);
    }
    if (int rc = check_launch("jpeg_idct_kernel")) return rc;
    {
        VLFM_TIMED("jpeg_upsample_kernel", st);
        auto kernel = rgb_order ? jpeg_upsample_kernel<true> : jpeg_upsample_kernel<false>;
        VLFM_KLAUNCH(kernel, dim3((unsigned)g.upsample_grid()), dim3(256), 0, st, d_planes, g, d_out);
    }
    return check_launch("jpeg_upsample_kernel");
}

}  // namespace jpeg
}  // namespace vlfm

// ================================================================================================ C ABI
using namespace vlfm;
using namespace vlfm::jpeg;

namespace {
const uint16_t kStdLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
                               14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint16_t kStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
}  // namespace

extern "C" int vlfm_jpeg_quant_tables_host(int quality, uint16_t* h_tables) {
    if (!h_tables || quality < 1 || quality > 100) return fail(VLFM_ERR_INVALID, "jpeg_quant_tables_host: bad argument");
    // jcparam.c jpeg_quality_scaling, jpeg_add_quant_table(force_baseline = TRUE)
    const long s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const long l = (kStdLuma[i] * s + 50) / 100, c = (kStdChroma[i] * s + 50) / 100;
        h_tables[i] = (uint16_t)(l < 1 ? 1 : l > 255 ? 255 : l);
        h_tables[64 + i] = (uint16_t)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
    return VLFM_OK;
}

extern "C" size_t vlfm_jpeg_scratch_bytes(int n, int H, int W) {
    Geometry g;
    return geometry(n, H, W, &g) ? (size_t)n * g.frame_scratch() : 0;
}

extern "C" int vlfm_jpeg_roundtrip_batched(const uint8_t* d_in, uint8_t* d_out, int n, int H, int W,
                                           const uint16_t* h_tables, void* d_scratch, size_t scratch_bytes,
                                           void* stream) {
    Geometry g;
    if (!d_in || !d_out || !h_tables || !geometry(n, H, W, &g))
        return fail(VLFM_ERR_INVALID, "jpeg_roundtrip_batched: bad argument");
    QuantTables qt;
    for (int i = 0; i < 128; ++i) {
        if (h_tables[i] < 1 || h_tables[i] > 255)
            return fail(VLFM_ERR_INVALID, "jpeg_roundtrip_batched: quantisation table entries must be 1..255");
        qt.q[i >> 6][i & 63] = h_tables[i];
    }
    if (!d_scratch || (reinterpret_cast<uintptr_t>(d_scratch) & 15))
        return fail(VLFM_ERR_INVALID, "jpeg_roundtrip_batched: scratch must be a 16-byte aligned device buffer");
    if (scratch_bytes < (size_t)n * g.frame_scratch())
        return fail(VLFM_ERR_CAPACITY, "jpeg_roundtrip_batched: scratch too small");
    const size_t code_blocks = (size_t)n * g.mh * g.tiles_x;
    const size_t up_blocks = ((size_t)n * H * ((W + 15) / 16) + 255) / 256;
    if (code_blocks > 0x7fffffff || up_blocks > 0x7fffffff)
        return fail(VLFM_ERR_INVALID, "jpeg_roundtrip_batched: batch too large for one launch");
    const bool rows16 = (3 * (size_t)W) % 16 == 0;
    g.vec_in = rows16 && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
    g.vec_out = rows16 && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0;
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    hipStream_t st = (hipStream_t)stream;
    {
        VLFM_TIMED("jpeg_code_kernel", st);
        auto kernel = jpeg_code_kernel<false, false>;
        VLFM_KLAUNCH(kernel, dim3((unsigned)code_blocks), dim3(THREADS), 0, st, d_in, qt, g, scratch);
    }
    if (int rc = check_launch("jpeg_code_kernel")) return rc;
    {
        VLFM_TIMED("jpeg_upsample_kernel", st);
        auto kernel = jpeg_upsample_kernel<false>;
        VLFM_KLAUNCH(kernel, dim3((unsigned)up_blocks), dim3(256), 0, st, scratch, g, d_out);
    }
    return check_launch("jpeg_upsample_kernel");
}
