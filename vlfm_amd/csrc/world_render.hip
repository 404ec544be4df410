// world_render.hip -- depth frames of the rooms-and-pillars world (vlfm_amd/synthetic.py) ray-cast for n cameras at arbitrary
// poses in ONE launch: the arithmetic of synthetic.wall_profile / depth_from_profile and of harness.RoomsRenderer._cast, bit for
// bit (f64, true divisions, no contraction: the library is built with -ffp-contract=off and the two-rounding expressions below
// go through __dmul_rn / __dadd_rn / __dsub_rn, which are never fused).
//
//   column u:  m = -(u - W/2) / fx;  dx = c - s*m;  dy = s + c*m;  |dx| < 1e-12 -> 1e-12 (same for dy)
//              slab test against every box; hit when tmax >= max(tmin, 0) and tmin > 0 (a box around the camera is transparent)
//              wall(u) = f32(min over the hit boxes of tmin), inf when nothing is hit
//   row r:     floor(r) = r - H/2 > 0 ? height * fx / (r - H/2) : inf
//   pixel:     f32(clamp((min(wall, floor) - lo) / (hi - lo), 1e-3, 1))
//
// Every step of the normalisation (subtract lo, divide by hi - lo > 0, clamp, round to f32) is monotone non-decreasing, so
// norm(min(wall, floor)) == min(norm(wall), norm(floor)) exactly: the kernel normalises once per column and once per row and
// the per-pixel work is one f32 min and the store.
//
// Layout: grid (row bands, cameras), 256 threads.  A workgroup holds the boxes, the normalised column profile [W] and the
// normalised floor values of its band of rows in LDS; the column profile is recomputed per band (W * B * 4 divisions) so that a
// handful of cameras still spreads over the chip.  With W a multiple of 4 and a 16-byte aligned output every lane owns 4
// adjacent columns and a band leaves as consecutive 16-byte stores; any other W takes the scalar store loop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vlfm_amd.h"
#include "profile.h"
#include "status.h"

namespace vlfm {
namespace world {

constexpr int THREADS = 256;
constexpr int MIN_BAND_ROWS = 4;

struct CameraRec {      // 64 bytes, vlfm_amd.h
    double x, y, c, s, height, fx, lo, hi;
};

__device__ __forceinline__ float normalise(double d, double lo, double span) {
    double v = (d - lo) / span;
    v = v < 1e-3 ? 1e-3 : v;
    v = v > 1.0 ? 1.0 : v;
    return (float)v;
}

__global__ __launch_bounds__(THREADS) void rooms_raycast_kernel(const CameraRec* __restrict__ cameras,
                                                                const double* __restrict__ boxes, int n_boxes, int H, int W,
                                                                int band, int vec4, float* __restrict__ out) {
    extern __shared__ double smem[];
    const int r0 = blockIdx.x * band;
    if (r0 >= H) return;                                   // (uniform for the workgroup: before any barrier)
    const int rows = min(band, H - r0);
    const int tid = threadIdx.x;
    double* sbox = smem;                                   // [n_boxes][4]
    float* ncol = reinterpret_cast<float*>(smem + 4 * n_boxes);   // [W rounded up to 4]: 16-byte aligned (32 * n_boxes bytes in)
    float* nrow = ncol + ((W + 3) & ~3);                   // [band]
    const CameraRec cam = cameras[blockIdx.y];
    for (int i = tid; i < 4 * n_boxes; i += THREADS) sbox[i] = boxes[i];
    const double span = cam.hi - cam.lo;
    const double inf = __builtin_inf();
    for (int i = tid; i < rows; i += THREADS) {
        const int rr = r0 + i - H / 2;
        const double floor_d = rr > 0 ? __dmul_rn(cam.height, cam.fx) / (double)rr : inf;
        nrow[i] = normalise(floor_d, cam.lo, span);
    }
    __syncthreads();
    for (int u = tid; u < W; u += THREADS) {
        const double m = -(double)(u - W / 2) / cam.fx;
        double dx = __dsub_rn(cam.c, __dmul_rn(cam.s, m));
        double dy = __dadd_rn(cam.s, __dmul_rn(cam.c, m));
        if (fabs(dx) < 1e-12) dx = 1e-12;
        if (fabs(dy) < 1e-12) dy = 1e-12;
        double best = inf;
        for (int b = 0; b < n_boxes; ++b) {
            const double tx0 = (sbox[4 * b + 0] - cam.x) / dx, tx1 = (sbox[4 * b + 2] - cam.x) / dx;
            const double ty0 = (sbox[4 * b + 1] - cam.y) / dy, ty1 = (sbox[4 * b + 3] - cam.y) / dy;
            const double tmin = fmax(fmin(tx0, tx1), fmin(ty0, ty1));
            const double tmax = fmin(fmax(tx0, tx1), fmax(ty0, ty1));
            if (tmax >= fmax(tmin, 0.0) && tmin > 0.0) best = fmin(best, tmin);
        }
        const float wall = (float)best;                    // the host path keeps the profile in f32
        ncol[u] = normalise((double)wall, cam.lo, span);
    }
    __syncthreads();
    float* dst = out + ((size_t)blockIdx.y * H + r0) * (size_t)W;      // the band's rows are contiguous
    if (vec4) {
        const int ng = W >> 2, total = rows * ng;
        const int dr = THREADS / ng, dg = THREADS % ng;
        int r = tid / ng, g = tid % ng;
        float4* dst4 = reinterpret_cast<float4*>(dst);
        const float4* ncol4 = reinterpret_cast<const float4*>(ncol);
        for (int idx = tid; idx < total; idx += THREADS) {
            const float4 cv = ncol4[g];
            const float rv = nrow[r];
            dst4[idx] = make_float4(fminf(cv.x, rv), fminf(cv.y, rv), fminf(cv.z, rv), fminf(cv.w, rv));
            r += dr;
            g += dg;
            if (g >= ng) {
                g -= ng;
                ++r;
            }
        }
    } else {
        const int total = rows * W;
        const int dr = THREADS / W, dc = THREADS % W;
        int r = tid / W, c = tid % W;
        for (int idx = tid; idx < total; idx += THREADS) {
            dst[idx] = fminf(ncol[c], nrow[r]);
            r += dr;
            c += dc;
            if (c >= W) {
                c -= W;
                ++r;
            }
        }
    }
}

}  // namespace world
}  // namespace vlfm

using namespace vlfm;
using namespace vlfm::world;

extern "C" int vlfm_rooms_raycast(const double* d_cameras, int n, const double* d_boxes, int n_boxes, int H, int W,
                                  float* d_out, void* stream) {
    static_assert(sizeof(CameraRec) == 64, "camera record layout");
    if (n < 0 || n > 65535 || n_boxes < 0 || H <= 0 || W <= 0 || (n > 0 && (!d_cameras || !d_out)) || (n_boxes > 0 && !d_boxes))
        return fail(VLFM_ERR_INVALID, "rooms_raycast: bad argument");
    if (n == 0) return VLFM_OK;
    // row bands: enough workgroups for four per compute unit, never fewer than MIN_BAND_ROWS rows each
    const long long want = 4LL * device_cu_count();
    long long bands = (want + n - 1) / n;
    const long long most = (H + MIN_BAND_ROWS - 1) / MIN_BAND_ROWS;
    bands = bands < 1 ? 1 : (bands > most ? most : bands);
    const int band = (int)((H + bands - 1) / bands);
    const int grid_x = (H + band - 1) / band;
    const size_t lds = (size_t)n_boxes * 32 + (size_t)((W + 3) & ~3) * 4 + (size_t)band * 4;
    if (lds > 64 * 1024) return fail(VLFM_ERR_INVALID, "rooms_raycast: boxes + one image row + one row band exceed 64 KB of LDS");
    const int vec4 = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(d_out) % 16 == 0);
    hipStream_t st = (hipStream_t)stream;
    VLFM_TIMED("rooms_raycast_kernel", st);
    VLFM_KLAUNCH(rooms_raycast_kernel, dim3(grid_x, n), dim3(THREADS), lds, st,
                 reinterpret_cast<const CameraRec*>(d_cameras), d_boxes, n_boxes, H, W, band, vec4, d_out);
    return check_launch("rooms_raycast_kernel");
}
