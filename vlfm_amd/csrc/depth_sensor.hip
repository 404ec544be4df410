// depth_sensor.hip -- what a depth CAMERA makes of the exact frames the ray caster writes (world_render.hip): axial noise,
// disparity quantisation and holes, for n frames in ONE launch; the arithmetic of synthetic.depth_sensor_numpy, bit for bit (f32,
// one rounding per operation: the library is built with -ffp-contract=off and the expressions below go through __fmul_rn /
// __fadd_rn / __fsub_rn / __fdiv_rn, which are never fused; rintf rounds half to even).  The rule is stated with the entry point
// at the end of the file and in include/vlfm_amd.h.
//
// Layout: grid (row bands, frames), 256 threads, no LDS.  A lane owns four adjacent columns and walks them down the rows of one
// 8-row block line (rows 8k .. 8k + 7, cut to the band): the patch hash of its 8 x 8 block is evaluated once for those rows, not
// per pixel.  With W a multiple of 4 and both planes 16-byte aligned the four columns arrive in one 16-byte load and leave in one
// 16-byte store; any other width or alignment takes the scalar loads and stores (columns past W - 1 repeat column W - 1 and are
// never stored).
// Edge stage: the rows above and below come straight from global memory through the cache, and a lane keeps them in registers
// while it walks down (the row below becomes the current row, the current row the row above): per row one 16-byte load of the
// next row and two scalar loads left and right of its four columns, all of lines this workgroup or its neighbour has just read.
// No halo in LDS: there is no barrier, a band's seam needs no case of its own (the row above a band is a row of d_clean like
// any other; d_out never aliases it), and the only redundant traffic is two rows per 8-row walk, served by the cache.  A
// neighbour outside the frame is replaced by the pixel itself: the difference is 0 (or NaN), never greater than edge_m.
// The edge stage and the 16-byte path are template parameters, every other stage a branch on a kernel argument (uniform: an SGPR
// compare): a stage that is off costs no hash and no load.
// Invalid count: a lane counts in a register, a wave adds its 64 counts with shuffles, and its first lane issues ONE atomicAdd.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vlfm_amd.h"
#include "profile.h"
#include "row_bands.h"
#include "status.h"

namespace vlfm {
namespace sensor {

constexpr int THREADS = 256;
constexpr int BLOCK = 8;                      // synthetic.DEPTH_SENSOR_BLOCK
constexpr float NOISE_SCALE = 0x1.bb67aep-16f;   // f32(1 / sqrt(1431655765)), bits 0x37ddb3d7: synthetic.DEPTH_SENSOR_NOISE_SCALE

struct Params {
    float sigma0, sigma2, k, edge, zmin, zmax;
    uint32_t t_drop, t_patch;
    int noise, quant, range;                  // stages that are on
};

__device__ __forceinline__ uint32_t mix32(uint32_t a, uint32_t b, uint32_t salt) {      // synthetic._mix32
    uint32_t h = a * 2654435761u + b * 40503u + salt * 97u + 0x9E3779B9u;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

__device__ __forceinline__ float metres(float d, float lo, float span) { return __fadd_rn(lo, __fmul_rn(d, span)); }

// the four columns u .. u + 3 of a row; scalar path: a column past W - 1 repeats column W - 1
template <bool VEC4>
__device__ __forceinline__ void load4(const float* __restrict__ row, int u, int W, float (&v)[4]) {
    if constexpr (VEC4) {
        const float4 q = *reinterpret_cast<const float4*>(row + u);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = row[min(u + j, W - 1)];
    }
}

__device__ __forceinline__ bool steps(float zn, float z, float edge) { return fabsf(__fsub_rn(zn, z)) > edge; }

// one pixel: clean value d, its metres z (read only by the stages that need it), `inv` from the patch and edge stages
__device__ __forceinline__ float sense(float d, float z, bool inv, uint32_t p, uint32_t kf, const Params& a, float lo, float span,
                                       int& count) {
    if (a.range) inv |= !(z >= a.zmin && z <= a.zmax);
    if (a.t_drop) inv |= mix32(kf, p, 55u) < a.t_drop;
    float v = d;
    if (a.noise | a.quant) {
        float z1 = z;
        if (a.noise) {
            const uint32_t h1 = mix32(kf, p, 53u), h2 = mix32(kf, p, 54u);
            const int n = (int)((h1 & 0xFFFFu) + (h1 >> 16) + (h2 & 0xFFFFu) + (h2 >> 16)) - 131070;
            const float nf = __fmul_rn((float)n, NOISE_SCALE);
            const float sg = __fadd_rn(a.sigma0, __fmul_rn(a.sigma2, __fmul_rn(z, z)));
            z1 = __fadd_rn(z, __fmul_rn(sg, nf));
        }
        if (a.quant) {
            z1 = z1 < 1e-3f ? 1e-3f : z1;                  // (selects, not fmaxf: a NaN stays a NaN, as in the statement)
            float m = rintf(__fdiv_rn(a.k, z1));
            m = m < 1.0f ? 1.0f : m;
            z1 = __fdiv_rn(a.k, m);
        }
        v = __fdiv_rn(__fsub_rn(z1, lo), span);
        v = v < 1e-3f ? 1e-3f : (v > 1.0f ? 1.0f : v);
    }
    if (inv) {
        v = 0.0f;
        ++count;
    }
    return v;
}

template <bool VEC4, bool EDGE>
__global__ __launch_bounds__(THREADS) void depth_sensor_kernel(const float* __restrict__ clean, float* __restrict__ out, int H,
                                                               int W, int band, const uint32_t* __restrict__ keys,
                                                               const float* __restrict__ range, const Params a,
                                                               int32_t* __restrict__ invalid) {
    const int r0 = blockIdx.x * band;
    if (r0 >= H) return;                                   // (uniform for the workgroup)
    const int r1 = min(r0 + band, H);
    const int frame = blockIdx.y;
    const uint32_t kf = keys[frame];
    const float lo = range[2 * frame], span = __fsub_rn(range[2 * frame + 1], lo);
    const size_t base = (size_t)frame * (size_t)H * (size_t)W;
    const float* __restrict__ src = clean + base;
    float* __restrict__ dst = out + base;
    const int ng = (W + 3) >> 2, bw = (W + BLOCK - 1) / BLOCK;
    const int line0 = r0 / BLOCK, lines = (r1 - 1) / BLOCK - line0 + 1;      // the 8-row block lines this band touches
    const int items = lines * ng;
    const bool need_z = EDGE || a.range || a.noise || a.quant;
    int count = 0;
    for (int it = threadIdx.x; it < items; it += THREADS) {
        const int line = line0 + it / ng, u = 4 * (it % ng);
        const int ra = max(line * BLOCK, r0), rb = min(line * BLOCK + BLOCK, r1);
        const bool patch = a.t_patch != 0 && mix32(kf, (uint32_t)(line * bw + u / BLOCK), 56u) < a.t_patch;
        float dc[4], zc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, zu[4], zd[4], dn[4];
        if constexpr (EDGE) {
            load4<VEC4>(src + (size_t)ra * W, u, W, dc);
#pragma unroll
            for (int j = 0; j < 4; ++j) zc[j] = metres(dc[j], lo, span);
            if (ra > 0) {
                load4<VEC4>(src + (size_t)(ra - 1) * W, u, W, zu);
#pragma unroll
                for (int j = 0; j < 4; ++j) zu[j] = metres(zu[j], lo, span);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) zu[j] = zc[j];
            }
        }
        for (int r = ra; r < rb; ++r) {
            const float* __restrict__ row = src + (size_t)r * W;
            bool inv[4] = {patch, patch, patch, patch};
            if constexpr (EDGE) {
                if (r + 1 < H) {
                    load4<VEC4>(row + W, u, W, dn);
#pragma unroll
                    for (int j = 0; j < 4; ++j) zd[j] = metres(dn[j], lo, span);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) dn[j] = dc[j], zd[j] = zc[j];
                }
                const float zl = u > 0 ? metres(row[u - 1], lo, span) : zc[0];
                const float zr = u + 4 < W ? metres(row[u + 4], lo, span) : zc[3];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float left = j == 0 ? zl : zc[j > 0 ? j - 1 : 0], right = j == 3 ? zr : zc[j < 3 ? j + 1 : 3];
                    inv[j] |= steps(zu[j], zc[j], a.edge) || steps(zd[j], zc[j], a.edge) || steps(left, zc[j], a.edge) ||
                              steps(right, zc[j], a.edge);
                }
            } else {
                load4<VEC4>(row, u, W, dc);
                if (need_z) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) zc[j] = metres(dc[j], lo, span);
                }
            }
            const uint32_t p = (uint32_t)r * (uint32_t)W + (uint32_t)u;
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int one = 0;
                o[j] = sense(dc[j], zc[j], inv[j], p + (uint32_t)j, kf, a, lo, span, one);
                if (VEC4 || u + j < W) count += one;
            }
            if constexpr (VEC4) {
                *reinterpret_cast<float4*>(dst + (size_t)r * W + u) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (u + j < W) dst[(size_t)r * W + u + j] = o[j];
            }
            if constexpr (EDGE) {
#pragma unroll
                for (int j = 0; j < 4; ++j) zu[j] = zc[j], zc[j] = zd[j], dc[j] = dn[j];
            }
        }
    }
    if (invalid != nullptr) {                              // (uniform: every lane of the wave takes part in the shuffles)
        for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off);
        if ((threadIdx.x & 63) == 0 && count != 0) atomicAdd(invalid + frame, count);
    }
}

}  // namespace sensor
}  // namespace vlfm

using namespace vlfm;
using namespace vlfm::sensor;

// ------------------------------------------------------------------------------------------------------------ the entry
// vlfm_depth_sensor: per frame i, kf = d_keys[i], lo = d_range[i][0], span = d_range[i][1] - lo, p = r * W + u:
//   metres    z = lo + d * span
//   invalid   range stage on (min_range_m > 0 or max_range_m < inf) and not (z >= min and z <= max);  edge stage on and
//             |z_n - z| > edge_m for a 4-neighbour inside the frame;  mix32(kf, p, 55) < drop_threshold;
//             mix32(kf, (r >> 3) * ((W + 7) >> 3) + (u >> 3), 56) < patch_threshold.  Invalid: 0.0f
//   noise     nf = f32(sum of the four 16-bit halves of mix32(kf, p, 53) and mix32(kf, p, 54), minus 131070) * NOISE_SCALE,
//             z1 = z + (sigma0 + sigma2 * (z * z)) * nf
//   quantise  z1 = z1 < 1e-3f ? 1e-3f : z1;  m = rint(k / z1);  m = m < 1 ? 1 : m;  z1 = k / m
//   output    v = (z1 - lo) / span clipped to [1e-3f, 1]; with noise and quantisation off the input value itself
extern "C" int vlfm_depth_sensor(const float* d_clean, float* d_out, int n, int H, int W, const uint32_t* d_keys,
                                 const float* d_range, float sigma0_m, float sigma2_per_m, float disparity_k,
                                 uint32_t drop_threshold, uint32_t patch_threshold, float edge_m, float min_range_m,
                                 float max_range_m, int32_t* d_invalid, int band_rows, void* stream) {
    if (n < 0 || n > 65535 || H < 1 || W < 1 || (long long)H * W >= (1LL << 31) || band_rows < 0)
        return fail(VLFM_ERR_INVALID, "depth_sensor: n in [0, 65535], H, W >= 1 with H * W < 2^31, band_rows >= 0");
    if (!(sigma0_m >= 0.0f) || !(sigma2_per_m >= 0.0f) || !(disparity_k >= 0.0f) || !(edge_m >= 0.0f) || !(min_range_m >= 0.0f) ||
        !(max_range_m >= 0.0f) || isinf(sigma0_m) || isinf(sigma2_per_m) || isinf(disparity_k) || isinf(edge_m) || isinf(min_range_m))
        return fail(VLFM_ERR_INVALID, "depth_sensor: the sensor's scalars must be finite and not negative (max_range_m may be inf)");
    if (n > 0 && (!d_clean || !d_out || !d_keys || !d_range)) return fail(VLFM_ERR_INVALID, "depth_sensor: missing array");
    if (n == 0) return VLFM_OK;
    const uintptr_t bytes = (uintptr_t)n * (uintptr_t)H * (uintptr_t)W * sizeof(float);
    const uintptr_t c0 = reinterpret_cast<uintptr_t>(d_clean), o0 = reinterpret_cast<uintptr_t>(d_out);
    if (c0 < o0 + bytes && o0 < c0 + bytes)
        return fail(VLFM_ERR_INVALID, "depth_sensor: d_out overlaps d_clean (the edge stage reads clean neighbours)");
    int band = band_rows;
    if (band == 0) {                                       // the ray caster's plan, in whole block lines
        band = plan_bands(n, H, H).band;
        band = (band + BLOCK - 1) / BLOCK * BLOCK;
    }
    band = band > H ? H : band;
    const dim3 grid((H + band - 1) / band, n);
    hipStream_t st = (hipStream_t)stream;
    Params a;
    a.sigma0 = sigma0_m, a.sigma2 = sigma2_per_m, a.k = disparity_k, a.edge = edge_m, a.zmin = min_range_m, a.zmax = max_range_m;
    a.t_drop = drop_threshold, a.t_patch = patch_threshold;
    a.noise = sigma0_m != 0.0f || sigma2_per_m != 0.0f;
    a.quant = disparity_k > 0.0f;
    a.range = min_range_m > 0.0f || !isinf(max_range_m);
    if (d_invalid != nullptr && hipMemsetAsync(d_invalid, 0, (size_t)n * sizeof(int32_t), st) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VLFM_ERR_HIP, "depth_sensor: the memset of d_invalid failed");
    }
    const bool vec4 = (W % 4 == 0) && (c0 % 16 == 0) && (o0 % 16 == 0), edge = edge_m > 0.0f;
    const auto kernel = vec4 ? (edge ? depth_sensor_kernel<true, true> : depth_sensor_kernel<true, false>)
                             : (edge ? depth_sensor_kernel<false, true> : depth_sensor_kernel<false, false>);
    VLFM_TIMED("depth_sensor_kernel", st);
    VLFM_KLAUNCH(kernel, grid, dim3(THREADS), 0, st, d_clean, d_out, H, W, band, d_keys, d_range, a, d_invalid);
    return check_launch("depth_sensor_kernel");
}
