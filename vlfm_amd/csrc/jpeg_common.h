// jpeg_common.h -- what more than one of jpeg_codec.hip (round trip, pixel kernels), jpeg_entropy.hip (encoder) and
// jpeg_decode.hip (decoder) uses: frame geometry, the zigzag table, the quantisation-table loader, the launches one file
// makes for another, and the wavefront scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vlfm_amd.h"
#include "status.h"

namespace vlfm {
namespace jpeg {

constexpr int kMaxDim = 65500;               // libjpeg's JPEG_MAX_DIMENSION: the largest frame side a JPEG can carry

constexpr int TILE_MCUS = 4;                 // MCUs per workgroup of the coding and IDCT kernels, side by side
constexpr int TILE_W = 16 * TILE_MCUS;       // 64 pixels
constexpr int TILE_ROW_BYTES = 3 * TILE_W;   // 192 bytes of interleaved samples per tile row
constexpr int BLOCKS = 6 * TILE_MCUS;        // 16 Y + 4 Cb + 4 Cr
constexpr int THREADS = 8 * BLOCKS;          // one thread per block row (then per block column): 192

// jutils.c jpeg_natural_order: the natural (row-major) index of the k-th coefficient in zigzag order.  (A constexpr table
// with a constant initialiser: the host reads it as it stands, device code that indexes it gets a constant-memory copy.)
constexpr uint8_t kNaturalOrder[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                       12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                       35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                       58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct QuantTables {
    uint16_t q[2][64];   // luma, chroma quantval in natural order (jcparam.c jpeg_add_quant_table), 1..255
};

struct Geometry {
    int n, H, W;
    int mh, mw;          // MCU rows / columns: ceil(H/16), ceil(W/16)
    int tiles_x;         // ceil(mw / TILE_MCUS)
    int ch, cw;          // real chroma size: ceil(H/2), ceil(W/2)
    int vec_in, vec_out; // 16-byte global access allowed for the frame rows (3W % 16 == 0 and the pointer is aligned)
    // decoded planes per frame: Y [16 mh][16 mw], Cb and Cr [8 mh][8 mw]
    __host__ __device__ size_t frame_scratch() const { return (size_t)384 * mh * mw; }
    size_t mcus() const { return (size_t)mh * mw; }   // per frame; the coefficient layout has 768 B (6 blocks) per MCU
    size_t code_grid() const { return (size_t)n * mh * tiles_x; }                              // coding / IDCT kernel
    size_t upsample_grid() const { return ((size_t)n * H * ((W + 15) / 16) + 255) / 256; }     // upsampling kernel
};

// The geometry of n frames of H x W read from d_in and written to d_out (either may be null: no vector access there);
// false for a size no JPEG has.
inline bool geometry(int n, int H, int W, Geometry* g, const void* d_in = nullptr, const void* d_out = nullptr) {
    if (n <= 0 || H <= 0 || W <= 0 || H > kMaxDim || W > kMaxDim) return false;
    g->n = n; g->H = H; g->W = W;
    g->mh = (H + 15) / 16; g->mw = (W + 15) / 16;
    g->tiles_x = (g->mw + TILE_MCUS - 1) / TILE_MCUS;
    g->ch = (H + 1) / 2; g->cw = (W + 1) / 2;
    const bool rows16 = (3 * (size_t)W) % 16 == 0;
    g->vec_in = d_in && rows16 && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
    g->vec_out = d_out && rows16 && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0;
    return true;
}

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// h_tables [2][64] into *qt; false if an entry is not 1..255.
inline bool load_quant_tables(const uint16_t* h_tables, QuantTables* qt) {
    for (int i = 0; i < 128; ++i) {
        if (h_tables[i] < 1 || h_tables[i] > 255) return false;
        qt->q[i >> 6][i & 63] = h_tables[i];
    }
    return true;
}

// jpeg_codec.hip, for the encoder: frames -> the quantised coefficients of every block of the scan, 768 bytes per MCU.
int launch_coefficients(const uint8_t* d_in, int n, int H, int W, int rgb_order, const QuantTables& qt, int16_t* d_coef,
                        hipStream_t st);
// jpeg_codec.hip, for the decoder: coefficients -> decoded planes -> frames.
int launch_pixels(const int16_t* d_coef, const vlfm_jpeg_frame* d_frames, const vlfm_jpeg_table_set* d_sets, int n_sets, int n,
                  int H, int W, int rgb_order, uint8_t* d_planes, uint8_t* d_out, hipStream_t st);

template <typename T>
__device__ __forceinline__ T wave_inclusive_sum(T x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

}  // namespace jpeg
}  // namespace vlfm
