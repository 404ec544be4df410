// depth_filter.hip -- the hole filling that stands between the depth camera and every reader of its frames: a pixel that is not
// kept (zero, NaN, negative; with recover_nonzero off also a clipped one) becomes the maximum ("far") or the minimum ("near") of
// the nearest source pixels to its left, right, above and below, for n frames in TWO launches (and the memset of the counts);
// synthetic.depth_filter_numpy bit for bit.  Values are only selected, never computed: nothing here rounds.  The rule is stated
// with the entry point at the end of the file and in include/vlfm_amd.h.
//
// A candidate is always > 0 (a source is), so 0.0f stands for "no candidate" wherever a candidate travels: in the carries, and
// in d_out between the passes.
//
// Row pass (depth_filter_rows_kernel): grid (rows / 4, frames), 256 threads, ONE WAVEFRONT PER ROW, no LDS, no barrier.  A row goes
// in chunks of 256 columns, a lane owns four adjacent ones.  The nearest source to the left of a lane's columns is that of the
// nearest lower lane which holds one -- one ballot of "my columns hold a source", the highest set bit below the lane, one
// cross-lane read of that lane's last source (value, column) -- or else the carry from the chunks before; the lane then scans its
// four pixels.  The walk goes left to right, writing kept pixels with their own bits and every hole with its left candidate or 0,
// then right to left over the chunks from the last one down to the first that holds a hole, where the lanes that own holes combine
// the right candidate into what they wrote themselves (a lane re-reads its own stores: program order).  A chunk without a hole
// (one compare per pixel, one ballot) is copied and only feeds the carry; a row without a hole is never walked back.
// Column pass (depth_filter_cols_kernel): grid (row bands, frames), 256 threads; a lane owns four adjacent columns (16 bytes per
// lane and row: whole rows coalesce) and walks them down its band carrying the last source (value, row) of each, then up.  It
// reads d_in for sources and hole tests and touches d_out at hole pixels only, where it combines its candidate with what the row
// pass left; a column of a band belongs to one lane, so the read-modify-write needs no atomics.  Before a walk the carry is warmed
// outside the band: from the band's edge outwards until each column has met a source, reach_px rows are behind it or the frame
// ends, so every band_rows gives the same result.  Lanes whose columns hold no hole in the band skip the second walk.  The second
// walk finishes a pixel: it counts filled / left (register, wave reduction with shuffles, ONE atomicAdd per wave and counter) and
// writes black_value.
// With W a multiple of 4 and both planes 16-byte aligned a lane's four columns arrive in one 16-byte load (the row pass also
// stores 16 bytes); any other width or alignment takes scalar loads and stores, and columns past W - 1 are never touched.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vlfm_amd.h"
#include "profile.h"
#include "row_bands.h"
#include "status.h"

namespace vlfm {
namespace dfilter {

constexpr int THREADS = 256;
constexpr int CHUNK = 256;                    // columns a wavefront holds at once in the row pass
constexpr int MAX_BAND_ROWS = 32;             // planned bands of the column pass: a hole costs its lane a dependent load and store,
                                              // which more, shorter walks hide (measured at 256 frames of 640 x 480 with 1 % holes:
                                              // 703 us a call at the ray caster's 120 rows, 512 / 500 / 491 / 507 / 586 at 60 / 30 / 16 / 8 / 4)

struct Params {
    float clip, black;
    int near, reach, clip_on, recover, set_black;      // reach 0: no limit
};

__device__ __forceinline__ bool is_source(float v, const Params& a) { return v > 0.0f && !(a.clip_on && v > a.clip); }
__device__ __forceinline__ bool is_kept(float v, const Params& a) { return a.recover ? v > 0.0f : is_source(v, a); }
// candidates a, b (0: none) -> the farther / nearer of the two
__device__ __forceinline__ float combine(float x, float y, int near) {
    if (x == 0.0f) return y;
    if (y == 0.0f) return x;
    return near ? (y < x ? y : x) : (y > x ? y : x);
}
__device__ __forceinline__ bool within(int steps, int reach) { return reach == 0 || steps <= reach; }

// the four columns u .. u + 3 of a row (u < W); scalar path: a column past W - 1 reads as 0.0f (no source) and is never stored
template <bool VEC4>
__device__ __forceinline__ void load4(const float* __restrict__ row, int u, int W, float (&v)[4]) {
    if constexpr (VEC4) {
        const float4 q = *reinterpret_cast<const float4*>(row + u);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = u + j < W ? row[u + j] : 0.0f;
    }
}

template <bool VEC4>
__global__ __launch_bounds__(THREADS) void depth_filter_rows_kernel(const float* __restrict__ in, float* out, int H, int W,
                                                                    const Params a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (r >= H) return;                                    // (uniform for the wavefront)
    const size_t off = ((size_t)blockIdx.y * (size_t)H + (size_t)r) * (size_t)W;
    const float* __restrict__ src = in + off;
    float* dst = out + off;
    const int chunks = (W + CHUNK - 1) / CHUNK;
    const unsigned long long below = (1ull << lane) - 1ull, above = lane == 63 ? 0ull : ~0ull << (lane + 1);
    float cv = 0.0f;                                       // the carry: the last source before the chunk (0: none) ...
    int cc = 0, first_hole = chunks;                       // ... and its column; the first chunk that holds a hole
    for (int k = 0; k < chunks; ++k) {
        const int u = k * CHUNK + 4 * lane;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (u < W) load4<VEC4>(src, u, W, v);
        float lv = 0.0f;                                   // this lane's last source
        int lc = 0;
        bool hole = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (is_source(v[j], a)) lv = v[j], lc = u + j;
            hole |= u + j < W && !is_kept(v[j], a);
        }
        const unsigned long long m = __ballot(lv != 0.0f);
        if (__ballot(hole) == 0ull) {                      // (uniform) nothing to fill: a copy
            if (u < W) {
                if constexpr (VEC4) {
                    *reinterpret_cast<float4*>(dst + u) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (u + j < W) dst[u + j] = v[j];
                }
            }
        } else {
            first_hole = min(first_hole, k);
            const unsigned long long prev = m & below;
            const int p = prev ? 63 - __clzll((long long)prev) : lane;
            float rv = __shfl(lv, p);
            int rc = __shfl(lc, p);
            if (!prev) rv = cv, rc = cc;
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = v[j];
                if (!is_kept(v[j], a)) o[j] = (rv != 0.0f && within(u + j - rc, a.reach)) ? rv : 0.0f;
                if (is_source(v[j], a)) rv = v[j], rc = u + j;
            }
            if (u < W) {
                if constexpr (VEC4) {
                    *reinterpret_cast<float4*>(dst + u) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (u + j < W) dst[u + j] = o[j];
                }
            }
        }
        if (m) {                                           // (uniform)
            const int top = 63 - __clzll((long long)m);
            cv = __shfl(lv, top), cc = __shfl(lc, top);
        }
    }
    cv = 0.0f, cc = 0;                                     // now the first source after the chunk
    for (int k = chunks - 1; k >= first_hole; --k) {
        const int u = k * CHUNK + 4 * lane;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (u < W) load4<VEC4>(src, u, W, v);
        float fv = 0.0f;                                   // this lane's first source
        int fc = 0;
        bool hole = false;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            if (is_source(v[j], a)) fv = v[j], fc = u + j;
            hole |= u + j < W && !is_kept(v[j], a);
        }
        const unsigned long long m = __ballot(fv != 0.0f);
        if (__ballot(hole) != 0ull) {                      // (uniform)
            const unsigned long long next = m & above;
            const int p = next ? __ffsll((long long)next) - 1 : lane;
            float rv = __shfl(fv, p);
            int rc = __shfl(fc, p);
            if (!next) rv = cv, rc = cc;
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                if (u + j < W && !is_kept(v[j], a) && rv != 0.0f && within(rc - (u + j), a.reach))
                    dst[u + j] = combine(dst[u + j], rv, a.near);
                if (is_source(v[j], a)) rv = v[j], rc = u + j;
            }
        }
        if (m) {                                           // (uniform)
            const int low = __ffsll((long long)m) - 1;
            cv = __shfl(fv, low), cc = __shfl(fc, low);
        }
    }
}

// the nearest source of each of the four columns at u, walking from row `from` in steps of `step` over at most `rows` rows
template <bool VEC4>
__device__ __forceinline__ void warm(const float* __restrict__ src, int u, int W, int from, int step, int rows, const Params& a,
                                     float (&cv)[4], int (&cr)[4]) {
    int missing = min(4, W - u);                           // (columns past W - 1 hold nothing to wait for)
    for (int i = 0, r = from; i < rows && missing > 0; ++i, r += step) {
        float v[4];
        load4<VEC4>(src + (size_t)r * W, u, W, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (cv[j] == 0.0f && is_source(v[j], a)) cv[j] = v[j], cr[j] = r, --missing;
    }
}

template <bool VEC4>
__global__ __launch_bounds__(THREADS) void depth_filter_cols_kernel(const float* __restrict__ in, float* out, int H, int W,
                                                                    int band, const Params a, int32_t* __restrict__ counts) {
    const int r0 = blockIdx.x * band;
    if (r0 >= H) return;                                   // (uniform for the workgroup)
    const int r1 = min(r0 + band, H);
    const int frame = blockIdx.y;
    const size_t base = (size_t)frame * (size_t)H * (size_t)W;
    const float* __restrict__ src = in + base;
    float* dst = out + base;
    const int ng = (W + 3) >> 2;
    int filled = 0, left = 0;
    for (int it = threadIdx.x; it < ng; it += THREADS) {
        const int u = 4 * it;
        float cv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v[4];      // the carry of each column: its last source (0: none) ...
        int cr[4] = {0, 0, 0, 0};                          // ... and that source's row
        warm<VEC4>(src, u, W, r0 - 1, -1, a.reach ? min(a.reach, r0) : r0, a, cv, cr);
        bool hole = false;
        for (int r = r0; r < r1; ++r) {                    // down: the candidates from above
            load4<VEC4>(src + (size_t)r * W, u, W, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (u + j < W && !is_kept(v[j], a)) {
                    hole = true;
                    if (cv[j] != 0.0f && within(r - cr[j], a.reach)) {
                        float* p = dst + (size_t)r * W + u + j;
                        *p = combine(*p, cv[j], a.near);
                    }
                }
                if (is_source(v[j], a)) cv[j] = v[j], cr[j] = r;
            }
        }
        if (!hole) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) cv[j] = 0.0f, cr[j] = 0;
        warm<VEC4>(src, u, W, r1, 1, a.reach ? min(a.reach, H - r1) : H - r1, a, cv, cr);
        for (int r = r1 - 1; r >= r0; --r) {               // up: the candidates from below; this walk finishes the pixel
            load4<VEC4>(src + (size_t)r * W, u, W, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (u + j < W && !is_kept(v[j], a)) {
                    float* p = dst + (size_t)r * W + u + j;
                    const float have = *p;
                    const float got = (cv[j] != 0.0f && within(cr[j] - r, a.reach)) ? combine(have, cv[j], a.near) : have;
                    if (got == 0.0f) {
                        ++left;
                        if (a.set_black) *p = a.black;
                    } else {
                        ++filled;
                        if (got != have) *p = got;
                    }
                }
                if (is_source(v[j], a)) cv[j] = v[j], cr[j] = r;
            }
        }
    }
    if (counts != nullptr) {                               // (uniform: every lane of the wave takes part in the shuffles)
        for (int off = 32; off > 0; off >>= 1) filled += __shfl_down(filled, off), left += __shfl_down(left, off);
        if ((threadIdx.x & 63) == 0) {
            if (filled != 0) atomicAdd(counts + 2 * frame, filled);
            if (left != 0) atomicAdd(counts + 2 * frame + 1, left);
        }
    }
}

}  // namespace dfilter
}  // namespace vlfm

using namespace vlfm;
using namespace vlfm::dfilter;

// ------------------------------------------------------------------------------------------------------------ the entry
// vlfm_depth_filter: per frame and pixel d,
//   positive   d > 0 (NaN, +0.0, -0.0 and negatives are not)
//   source     positive, and with clip_far > 0 not (d > clip_far)
//   kept       recover_nonzero ? positive : source -- leaves with its input bits; every other pixel is a hole
//   candidate  per direction left, right, up, down the value of the nearest source of d_in inside the frame, if reach_px == 0 or
//              it is at most reach_px steps away
//   hole       the maximum (fill 0) or minimum (fill 1) of its candidates; none: set_black ? black_value : 0.0f
//   counts     d_counts[i] = {holes of frame i with a candidate, holes without}
extern "C" int vlfm_depth_filter(const float* d_in, float* d_out, int n, int H, int W, int fill, int reach_px, float clip_far,
                                 int recover_nonzero, int set_black, float black_value, int32_t* d_counts, int band_rows,
                                 void* stream) {
    if (n < 0 || n > 65535 || H < 1 || W < 1 || (long long)H * W >= (1LL << 31) || band_rows < 0)
        return fail(VLFM_ERR_INVALID, "depth_filter: n in [0, 65535], H, W >= 1 with H * W < 2^31, band_rows >= 0");
    if ((fill != 0 && fill != 1) || reach_px < 0 || reach_px > 65535)
        return fail(VLFM_ERR_INVALID, "depth_filter: fill is 0 (far) or 1 (near), reach_px in [0, 65535] (0: no limit)");
    if (!(clip_far >= 0.0f) || isinf(clip_far) || isnan(black_value) || isinf(black_value))
        return fail(VLFM_ERR_INVALID, "depth_filter: clip_far must be finite and not negative, black_value finite");
    if (n > 0 && (!d_in || !d_out)) return fail(VLFM_ERR_INVALID, "depth_filter: missing array");
    if (n == 0) return VLFM_OK;
    const uintptr_t bytes = (uintptr_t)n * (uintptr_t)H * (uintptr_t)W * sizeof(float);
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(d_in), o0 = reinterpret_cast<uintptr_t>(d_out);
    if (i0 < o0 + bytes && o0 < i0 + bytes)
        return fail(VLFM_ERR_INVALID, "depth_filter: d_out overlaps d_in (the candidates are input pixels)");
    int band = band_rows == 0 ? plan_bands(n, H, MAX_BAND_ROWS).band : band_rows;
    band = band > H ? H : band;
    hipStream_t st = (hipStream_t)stream;
    Params a;
    a.clip = clip_far, a.black = black_value, a.near = fill, a.reach = reach_px, a.clip_on = clip_far > 0.0f;
    a.recover = recover_nonzero != 0, a.set_black = set_black != 0;
    if (d_counts != nullptr && hipMemsetAsync(d_counts, 0, (size_t)n * 2 * sizeof(int32_t), st) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VLFM_ERR_HIP, "depth_filter: the memset of d_counts failed");
    }
    const bool vec4 = (W % 4 == 0) && (i0 % 16 == 0) && (o0 % 16 == 0);
    {
        const dim3 grid((H + THREADS / 64 - 1) / (THREADS / 64), n);
        VLFM_TIMED("depth_filter_rows_kernel", st);
        const auto kernel = vec4 ? depth_filter_rows_kernel<true> : depth_filter_rows_kernel<false>;
        VLFM_KLAUNCH(kernel, grid, dim3(THREADS), 0, st, d_in, d_out, H, W, a);
        if (check_launch("depth_filter_rows_kernel") != VLFM_OK) return VLFM_ERR_HIP;
    }
    const dim3 grid((H + band - 1) / band, n);
    VLFM_TIMED("depth_filter_cols_kernel", st);
    const auto kernel = vec4 ? depth_filter_cols_kernel<true> : depth_filter_cols_kernel<false>;
    VLFM_KLAUNCH(kernel, grid, dim3(THREADS), 0, st, d_in, d_out, H, W, band, a, d_counts);
    return check_launch("depth_filter_cols_kernel");
}
