// map_render.hip -- gfx950 kernels that render ValueMap.visualize / ObstacleMap.visualize frames for a batch of slots
// (reference: vlfm/mapping/value_map.py:189-219, obstacle_map.py:171-192, traj_visualizer.py, img_utils.py:64-85).
//
// Per call, over the frames k = 0..n-1 of the requested slots env_ids[k], into uint8 [n][S][S][3] (BGR, or RGB):
//
//   value_partials_kernel   reduce channels -> explored mask -> per 8-row tile: max, min over non-zero cells, any zero
//   value_color_kernel      flip, min-max normalise in the slot's dtype, inferno LUT, zeros white, path cells green
//   obstacle_color_kernel   white / explored / non-navigable / obstacle colours, flip, path cells green
//   primitive_kernel        one workgroup per frame walks that frame's primitives (frontier circles, agent disc, heading,
//                           markers) in order: runs of primitives with one colour are painted concurrently (painting one
//                           colour is idempotent), a barrier separates runs, so overlaps come out as sequential drawing
//   traj_append_kernel      ORs new trajectory segments (cv2.line thickness 3) into a per-slot path bit-plane
//
// The rasteriser below restates OpenCV 4.5.5 drawing.cpp (Line2, FillConvexPoly, ThickLine, Circle, PolyLine) over a
// "painter": one instance writes colour bytes, one ORs bits into the path plane.  Normalising is NumPy's arithmetic:
// round-to-nearest sub / div / mul in f32 or f64 (the build passes -ffp-contract=off), then truncation to uint8.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vlfm_amd.h"
#include "profile.h"
#include "raster.h"
#include "status.h"

namespace vlfm {
namespace render {

// cv::COLORMAP_INFERNO as OpenCV 4.5.5 builds it: saturate_cast<uchar>(255 * f32(matplotlib "inferno" data)), B, G, R.
// (The data is matplotlib's, CC0; tests/test_map_render_cpu.py recomputes this table.)
__device__ inline const unsigned char* inferno_bgr(int i) {
    static constexpr unsigned char kInfernoBGR[256][3] = {
        {4, 0, 0}, {5, 0, 1}, {6, 1, 1}, {8, 1, 1}, {10, 1, 2}, {12, 2, 2}, {14, 2, 2}, {16, 2, 3},
        {18, 3, 4}, {20, 3, 4}, {23, 4, 5}, {25, 4, 6}, {27, 5, 7}, {29, 5, 8}, {31, 6, 9}, {34, 7, 10},
        {36, 7, 11}, {38, 8, 12}, {41, 8, 13}, {43, 9, 14}, {45, 9, 16}, {48, 10, 17}, {50, 10, 18}, {52, 11, 20},
        {55, 11, 21}, {57, 11, 22}, {60, 12, 24}, {62, 12, 25}, {65, 12, 27}, {67, 12, 28}, {69, 12, 30}, {72, 12, 31},
        {74, 12, 33}, {76, 12, 35}, {79, 12, 36}, {81, 12, 38}, {83, 11, 40}, {85, 11, 41}, {87, 11, 43}, {89, 11, 45},
        {91, 10, 47}, {92, 10, 49}, {94, 10, 50}, {95, 10, 52}, {97, 9, 54}, {98, 9, 56}, {99, 9, 57}, {100, 9, 59},
        {101, 9, 61}, {102, 9, 62}, {103, 10, 64}, {104, 10, 66}, {104, 10, 68}, {105, 10, 69}, {106, 11, 71}, {106, 11, 73},
        {107, 12, 74}, {107, 12, 76}, {108, 13, 77}, {108, 13, 79}, {108, 14, 81}, {109, 14, 82}, {109, 15, 84}, {109, 15, 85},
        {110, 16, 87}, {110, 16, 89}, {110, 17, 90}, {110, 18, 92}, {110, 18, 93}, {110, 19, 95}, {110, 19, 97}, {110, 20, 98},
        {110, 21, 100}, {110, 21, 101}, {110, 22, 103}, {110, 22, 105}, {110, 23, 106}, {110, 24, 108}, {110, 24, 109}, {110, 25, 111},
        {110, 25, 113}, {110, 26, 114}, {110, 26, 116}, {110, 27, 117}, {109, 28, 119}, {109, 28, 120}, {109, 29, 122}, {109, 29, 124},
        {109, 30, 125}, {108, 30, 127}, {108, 31, 128}, {108, 32, 130}, {107, 32, 132}, {107, 33, 133}, {107, 33, 135}, {106, 34, 136},
        {106, 34, 138}, {105, 35, 140}, {105, 35, 141}, {105, 36, 143}, {104, 37, 144}, {104, 37, 146}, {103, 38, 147}, {103, 38, 149},
        {102, 39, 151}, {102, 39, 152}, {101, 40, 154}, {100, 41, 155}, {100, 41, 157}, {99, 42, 159}, {99, 42, 160}, {98, 43, 162},
        {97, 44, 163}, {96, 44, 165}, {96, 45, 166}, {95, 46, 168}, {94, 46, 169}, {94, 47, 171}, {93, 48, 173}, {92, 48, 174},
        {91, 49, 176}, {90, 50, 177}, {90, 50, 179}, {89, 51, 180}, {88, 52, 182}, {87, 53, 183}, {86, 53, 185}, {85, 54, 186},
        {84, 55, 188}, {83, 56, 189}, {82, 57, 191}, {81, 58, 192}, {80, 58, 193}, {79, 59, 195}, {78, 60, 196}, {77, 61, 198},
        {76, 62, 199}, {75, 63, 200}, {74, 64, 202}, {73, 65, 203}, {72, 66, 204}, {71, 67, 206}, {70, 68, 207}, {69, 69, 208},
        {68, 70, 210}, {67, 71, 211}, {66, 72, 212}, {65, 74, 213}, {63, 75, 215}, {62, 76, 216}, {61, 77, 217}, {60, 78, 218},
        {59, 80, 219}, {58, 81, 221}, {56, 82, 222}, {55, 83, 223}, {54, 85, 224}, {53, 86, 225}, {52, 87, 226}, {51, 89, 227},
        {49, 90, 228}, {48, 92, 229}, {47, 93, 230}, {46, 94, 231}, {45, 96, 232}, {43, 97, 233}, {42, 99, 234}, {41, 100, 235},
        {40, 102, 235}, {38, 103, 236}, {37, 105, 237}, {36, 106, 238}, {35, 108, 239}, {33, 110, 239}, {32, 111, 240}, {31, 113, 241},
        {29, 115, 241}, {28, 116, 242}, {27, 118, 243}, {25, 120, 243}, {24, 121, 244}, {23, 123, 245}, {21, 125, 245}, {20, 126, 246},
        {19, 128, 246}, {18, 130, 247}, {16, 132, 247}, {15, 133, 248}, {14, 135, 248}, {12, 137, 248}, {11, 139, 249}, {10, 140, 249},
        {9, 142, 249}, {8, 144, 250}, {7, 146, 250}, {7, 148, 250}, {6, 150, 251}, {6, 151, 251}, {6, 153, 251}, {6, 155, 251},
        {7, 157, 251}, {7, 159, 252}, {8, 161, 252}, {9, 163, 252}, {10, 165, 252}, {12, 166, 252}, {13, 168, 252}, {15, 170, 252},
        {17, 172, 252}, {18, 174, 252}, {20, 176, 252}, {22, 178, 252}, {24, 180, 252}, {26, 182, 251}, {29, 184, 251}, {31, 186, 251},
        {33, 188, 251}, {35, 190, 251}, {38, 192, 250}, {40, 194, 250}, {42, 196, 250}, {45, 198, 250}, {47, 199, 249}, {50, 201, 249},
        {53, 203, 249}, {55, 205, 248}, {58, 207, 248}, {61, 209, 247}, {64, 211, 247}, {67, 213, 246}, {70, 215, 246}, {73, 217, 245},
        {76, 219, 245}, {79, 221, 244}, {83, 223, 244}, {86, 225, 244}, {90, 227, 243}, {93, 229, 243}, {97, 230, 242}, {101, 232, 242},
        {105, 234, 242}, {109, 236, 241}, {113, 237, 241}, {117, 239, 241}, {121, 241, 241}, {125, 242, 242}, {130, 244, 242}, {134, 245, 243},
        {138, 246, 243}, {142, 248, 244}, {146, 249, 245}, {150, 250, 246}, {154, 251, 248}, {157, 252, 249}, {161, 253, 250}, {164, 255, 252},
    };
    return kInfernoBGR[i];
}

constexpr int TILE_ROWS = 8;          // rows per min/max partial
constexpr int COLOR_ROWS = 4;         // rows per colour workgroup
constexpr int PX = 4;                 // pixels per thread in the colour passes

struct FrameHdr {                     // one per frame, uploaded with the primitives
    int env, f32, explored, pad;
};

// ------------------------------------------------------------------------------------------------ value reduction
struct Reduce {
    const double* value;   // [n_envs][S][S][C]
    const double* plane;   // [n][S][S] host-reduced planes (mode VLFM_REDUCE_PLANE)
    const uint32_t* explored;
    int S, C, stride, mode;
    double thresh;
    __device__ double cell(int k, const FrameHdr& h, int r, int x) const {
        double v;
        if (mode == VLFM_REDUCE_PLANE) {
            v = plane[((size_t)k * S + r) * S + x];
        } else {
            const double* c = value + (((size_t)h.env * S + r) * S + x) * C;
            double mx = c[0];
            for (int i = 1; i < C; i++) mx = c[i] > mx ? c[i] : mx;   // f32 slots hold f32 values: max is exact either way
            v = mx;
            if (mode == VLFM_REDUCE_EXPLORE) {
                // np.where(arr[..., 0] > t, arr[..., 0], max): the comparison runs in the array's dtype (t cast to it)
                const bool above = h.f32 ? ((float)c[0] > (float)thresh) : (c[0] > thresh);
                v = above ? c[0] : mx;
            }
        }
        if (h.explored >= 0 && !((explored[((size_t)h.explored * S + r) * stride + (x >> 5)] >> (x & 31)) & 1u)) v = 0.0;
        return v;
    }
};

__global__ __launch_bounds__(256) void value_partials_kernel(Reduce R, const FrameHdr* __restrict__ hdr,
                                                             double* __restrict__ partials, int tiles) {
    const int k = blockIdx.y, tile = blockIdx.x;
    const FrameHdr h = hdr[k];
    double mx = -INFINITY, mn = INFINITY;
    int zero = 0;
    const int r0 = tile * TILE_ROWS, r1 = min(R.S, r0 + TILE_ROWS);
    for (int i = threadIdx.x; i < (r1 - r0) * R.S; i += blockDim.x) {
        const int r = r0 + i / R.S, x = i % R.S;
        const double v = R.cell(k, h, r, x);
        mx = v > mx ? v : mx;
        if (v == 0.0) zero = 1;
        else mn = v < mn ? v : mn;
    }
    __shared__ double smx[256], smn[256];
    __shared__ int sz[256];
    smx[threadIdx.x] = mx; smn[threadIdx.x] = mn; sz[threadIdx.x] = zero;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            smx[threadIdx.x] = fmax(smx[threadIdx.x], smx[threadIdx.x + s]);
            smn[threadIdx.x] = fmin(smn[threadIdx.x], smn[threadIdx.x + s]);
            sz[threadIdx.x] |= sz[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* p = partials + ((size_t)k * tiles + tile) * 3;
        p[0] = smx[0]; p[1] = smn[0]; p[2] = sz[0];
    }
}

__device__ inline void put3(unsigned char* p, const unsigned char* bgr, int rgb) {
    p[0] = bgr[rgb ? 2 : 0]; p[1] = bgr[1]; p[2] = bgr[rgb ? 0 : 2];
}

// stores PX pixels (3 bytes each) at pixel x of a row: three dword stores when the row start is 4-byte aligned
__device__ inline void store_px(unsigned char* row, int x, int S, const unsigned char (*c)[3]) {
    if (x + PX <= S && ((S * 3) & 3) == 0 && ((uintptr_t)row & 3) == 0) {
        unsigned w[3] = {0u, 0u, 0u};
        for (int b = 0; b < 3 * PX; b++) w[b >> 2] |= (unsigned)c[b / 3][b % 3] << (8 * (b & 3));
        unsigned* d = reinterpret_cast<unsigned*>(row + 3 * x);
        d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
    } else {
        for (int j = 0; j < PX && x + j < S; j++)
            for (int b = 0; b < 3; b++) row[3 * (x + j) + b] = c[j][b];
    }
}

__global__ __launch_bounds__(256) void value_color_kernel(Reduce R, const FrameHdr* __restrict__ hdr,
                                                          const double* __restrict__ partials, int tiles,
                                                          const uint32_t* __restrict__ path, int rgb,
                                                          unsigned char* __restrict__ out) {
    const int k = blockIdx.y, S = R.S;
    const FrameHdr h = hdr[k];
    __shared__ double smx[256], smn[256];
    __shared__ int sz[256];
    double mx = -INFINITY, mn = INFINITY;
    int zero = 0;
    for (int t = threadIdx.x; t < tiles; t += blockDim.x) {
        const double* p = partials + ((size_t)k * tiles + t) * 3;
        mx = fmax(mx, p[0]); mn = fmin(mn, p[1]); zero |= p[2] != 0.0;
    }
    smx[threadIdx.x] = mx; smn[threadIdx.x] = mn; sz[threadIdx.x] = zero;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            smx[threadIdx.x] = fmax(smx[threadIdx.x], smx[threadIdx.x + s]);
            smn[threadIdx.x] = fmin(smn[threadIdx.x], smn[threadIdx.x + s]);
            sz[threadIdx.x] |= sz[threadIdx.x + s];
        }
        __syncthreads();
    }
    // img_utils.py:75-80 after value_map.py:203-205: zeros were replaced by the max, so the min is the min over the
    // non-zero cells, or the max itself when a zero lies below every non-zero cell
    const double M = smx[0];
    const double m = sz[0] ? fmin(smn[0], M) : smn[0];
    const double ptp = __dsub_rn(M, m);
    const float Mf = (float)M, mf = (float)m, ptpf = __fsub_rn(Mf, mf);
    const unsigned char white[3] = {255, 255, 255}, green[3] = {0, 255, 0};
    const int stride = (S + 31) >> 5;
    const int xs = (blockIdx.x * blockDim.x + threadIdx.x) * PX;
    if (xs >= S) return;
    for (int rr = 0; rr < COLOR_ROWS; rr++) {
        const int y = blockIdx.z * COLOR_ROWS + rr;
        if (y >= S) break;
        const int r = S - 1 - y;   // np.flipud
        unsigned char c[PX][3];
        const uint32_t pw = path ? path[((size_t)h.env * S + y) * stride + (xs >> 5)] : 0u;
        for (int j = 0; j < PX; j++) {
            const int x = xs + j;
            if (x >= S) break;
            const unsigned char* col;
            if ((pw >> (x & 31)) & 1u) {
                col = green;
            } else {
                const double v = R.cell(k, h, r, x);
                if (v == 0.0) {
                    col = white;
                } else {
                    int idx;
                    if (h.f32) idx = ptpf == 0.0f ? 0 : (int)__fmul_rn(__fdiv_rn(__fsub_rn((float)v, mf), ptpf), 255.0f);
                    else idx = ptp == 0.0 ? 0 : (int)__dmul_rn(__ddiv_rn(__dsub_rn(v, m), ptp), 255.0);
                    col = inferno_bgr(idx & 255);
                }
            }
            c[j][0] = col[rgb ? 2 : 0]; c[j][1] = col[1]; c[j][2] = col[rgb ? 0 : 2];
        }
        store_px(out + ((size_t)k * S + y) * S * 3, xs, S, c);
    }
}

// ------------------------------------------------------------------------------------------------ obstacle colours
__global__ __launch_bounds__(256) void obstacle_color_kernel(const uint32_t* __restrict__ obstacle,
                                                             const uint32_t* __restrict__ navigable,
                                                             const uint32_t* __restrict__ explored,
                                                             const FrameHdr* __restrict__ hdr, int S,
                                                             const uint32_t* __restrict__ path, unsigned pad_bgr,
                                                             int rgb, unsigned char* __restrict__ out) {
    const int k = blockIdx.y;
    const FrameHdr h = hdr[k];
    const int stride = (S + 31) >> 5;
    const int xs = (blockIdx.x * blockDim.x + threadIdx.x) * PX;
    if (xs >= S) return;
    const unsigned char white[3] = {255, 255, 255}, light[3] = {200, 255, 200}, black[3] = {0, 0, 0},
                        green[3] = {0, 255, 0};
    const unsigned char pad[3] = {(unsigned char)(pad_bgr & 255), (unsigned char)((pad_bgr >> 8) & 255),
                                  (unsigned char)((pad_bgr >> 16) & 255)};
    for (int rr = 0; rr < COLOR_ROWS; rr++) {
        const int y = blockIdx.z * COLOR_ROWS + rr;
        if (y >= S) break;
        const int r = S - 1 - y;   // cv2.flip(vis_img, 0)
        const size_t src = ((size_t)h.env * S + r) * stride + (xs >> 5);
        const uint32_t ow = obstacle[src], nw = navigable[src], ew = explored[src];
        const uint32_t pw = path ? path[((size_t)h.env * S + y) * stride + (xs >> 5)] : 0u;
        unsigned char c[PX][3];
        for (int j = 0; j < PX; j++) {
            const int b = (xs + j) & 31;
            const unsigned char* col = white;                       // obstacle_map.py:173-180, in drawing order
            if ((ew >> b) & 1u) col = light;
            if (!((nw >> b) & 1u)) col = pad;
            if ((ow >> b) & 1u) col = black;
            if ((pw >> b) & 1u) col = green;                         // traj_visualizer.py:53, after the flip
            c[j][0] = col[rgb ? 2 : 0]; c[j][1] = col[1]; c[j][2] = col[rgb ? 0 : 2];
        }
        store_px(out + ((size_t)k * S + y) * S * 3, xs, S, c);
    }
}

// ------------------------------------------------------------------------------------------------ rasteriser
// Painters: put(x, y) for a pixel already known to lie in the image, span(y, x1, x2) for a clipped span.
struct ImagePainter {
    unsigned char* img;      // one frame [S][S][3]
    const uint32_t* path;    // this slot's path plane: primitives drawn before the trajectory leave its pixels alone
    int S, stride, flip;
    unsigned char c[3];
    __device__ void put(int x, int y) const {
        const int yy = flip ? S - 1 - y : y;
        if (path && ((path[(size_t)yy * stride + (x >> 5)] >> (x & 31)) & 1u)) return;
        unsigned char* p = img + ((size_t)yy * S + x) * 3;
        p[0] = c[0]; p[1] = c[1]; p[2] = c[2];
    }
    __device__ void span(int y, int x1, int x2) const {
        for (int x = x1; x <= x2; x++) put(x, y);
    }
};

struct BitPainter {
    uint32_t* plane;   // [S][stride]
    int S, stride;
    __device__ void put(int x, int y) const { atomicOr(&plane[(size_t)y * stride + (x >> 5)], 1u << (x & 31)); }
    __device__ void span(int y, int x1, int x2) const {
        for (int x = x1; x <= x2;) {
            const int w = x >> 5, e = min(x2, (w << 5) + 31);
            const unsigned hi = (e & 31) == 31 ? 0xFFFFFFFFu : ((1u << ((e & 31) + 1)) - 1u);
            atomicOr(&plane[(size_t)y * stride + w], hi & ~((1u << (x & 31)) - 1u));
            x = e + 1;
        }
    }
};

// cv Line2: 16.16 end points, clipped to the image, every point bounds-checked
template <class P>
__device__ void line2(const P& p, long long x1, long long y1, long long x2, long long y2) {
    const int S = p.S;
    if (!clip_line((long long)S << XY_SHIFT, (long long)S << XY_SHIFT, x1, y1, x2, y2)) return;
    long long dx = x2 - x1, dy = y2 - y1;
    const long long j = dx < 0 ? -1 : 0, i = dy < 0 ? -1 : 0;
    const long long ax = (dx ^ j) - j, ay = (dy ^ i) - i;
    long long x_step, y_step;
    int ecount;
    if (ax > ay) {
        dy = (dy ^ j) - j;
        if (j) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
        x_step = XY_ONE;
        y_step = (dy << XY_SHIFT) / (ax | 1);
        ecount = (int)((x2 - x1) >> XY_SHIFT);
    } else {
        dx = (dx ^ i) - i;
        if (i) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
        x_step = (dx << XY_SHIFT) / (ay | 1);
        y_step = XY_ONE;
        ecount = (int)((y2 - y1) >> XY_SHIFT);
    }
    x1 += XY_ONE >> 1;
    y1 += XY_ONE >> 1;
    auto put = [&](long long x, long long y) {
        if (x >= 0 && y >= 0 && x < S && y < S) p.put((int)x, (int)y);
    };
    put((x2 + (XY_ONE >> 1)) >> XY_SHIFT, (y2 + (XY_ONE >> 1)) >> XY_SHIFT);
    if (ax > ay) {
        x1 >>= XY_SHIFT;
        for (; ecount >= 0; ecount--) { put(x1, y1 >> XY_SHIFT); x1++; y1 += y_step; }
    } else {
        y1 >>= XY_SHIFT;
        for (; ecount >= 0; ecount--) { put(x1 >> XY_SHIFT, y1); x1 += x_step; y1++; }
    }
}

// cv FillConvexPoly, shift = XY_SHIFT (what ThickLine hands it), LINE_8
template <class P>
__device__ void fill_convex_poly(const P& p, const long long* vx, const long long* vy, int npts) {
    const int S = p.S, shift = XY_SHIFT;
    const long long delta = 1LL << shift >> 1;
    struct { int idx, di; long long x, dx; int ye; } edge[2];
    int imin = 0, edges = npts, y;
    long long xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0];
    long long p0x = vx[npts - 1], p0y = vy[npts - 1];
    for (int i = 0; i < npts; i++) {
        if (vy[i] < ymin) { ymin = vy[i]; imin = i; }
        if (vy[i] > ymax) ymax = vy[i];
        if (vx[i] > xmax) xmax = vx[i];
        if (vx[i] < xmin) xmin = vx[i];
        line2(p, p0x, p0y, vx[i], vy[i]);
        p0x = vx[i]; p0y = vy[i];
    }
    xmin = (xmin + delta) >> shift; xmax = (xmax + delta) >> shift;
    ymin = (ymin + delta) >> shift; ymax = (ymax + delta) >> shift;
    if (npts < 3 || (int)xmax < 0 || (int)ymax < 0 || (int)xmin >= S || (int)ymin >= S) return;
    if (ymax > S - 1) ymax = S - 1;
    edge[0].idx = edge[1].idx = imin;
    edge[0].ye = edge[1].ye = y = (int)ymin;
    edge[0].di = 1; edge[1].di = npts - 1;
    edge[0].x = edge[1].x = -XY_ONE;
    edge[0].dx = edge[1].dx = 0;
    do {
        for (int i = 0; i < 2; i++) {
            if (y >= edge[i].ye) {
                int idx0 = edge[i].idx, di = edge[i].di;
                int idx = idx0 + di;
                if (idx >= npts) idx -= npts;
                for (; edges-- > 0;) {
                    const int ty = (int)((vy[idx] + delta) >> shift);
                    if (ty > y) {
                        const long long xs = vx[idx0], xe = vx[idx];
                        edge[i].ye = ty;
                        edge[i].dx = ((xe - xs) * 2 + (ty - y)) / (2 * (ty - y));
                        edge[i].x = xs;
                        edge[i].idx = idx;
                        break;
                    }
                    idx0 = idx;
                    idx += di;
                    if (idx >= npts) idx -= npts;
                }
            }
        }
        if (edges < 0) break;
        if (y < 0) {   // rows above the image paint nothing: on to the next edge event or to row 0 (the edges are linear
                       // in between, so stepping k rows at once is the same integer arithmetic as k single steps)
            int ny = 0;
            if (edge[0].ye < ny) ny = edge[0].ye;
            if (edge[1].ye < ny) ny = edge[1].ye;
            if (ny <= y) ny = y + 1;
            const long long k = ny - y;
            edge[0].x += edge[0].dx * k;
            edge[1].x += edge[1].dx * k;
            y = ny - 1;
            continue;
        }
        {
            int left = 0, right = 1;
            if (edge[0].x > edge[1].x) { left = 1; right = 0; }
            int xx1 = (int)((edge[left].x + (XY_ONE >> 1)) >> XY_SHIFT);
            int xx2 = (int)((edge[right].x + (XY_ONE >> 1)) >> XY_SHIFT);
            if (xx2 >= 0 && xx1 < S) {
                if (xx1 < 0) xx1 = 0;
                if (xx2 >= S) xx2 = S - 1;
                p.span(y, xx1, xx2);
            }
        }
        edge[0].x += edge[0].dx;
        edge[1].x += edge[1].dx;
    } while (++y <= (int)ymax);
}

// cv Circle (midpoint): fill != 0 -> clipped spans, else the eight symmetric points that lie in the image
template <class P>
__device__ void circle(const P& p, int cx, int cy, int radius, int fill) {
    const int S = p.S;
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    auto span = [&](int y, int x1, int x2) {
        if ((unsigned)y >= (unsigned)S) return;
        if (x1 < 0) x1 = 0;
        if (x2 > S - 1) x2 = S - 1;
        if (x1 <= x2) p.span(y, x1, x2);
    };
    auto pt = [&](int x, int y) {
        if ((unsigned)x < (unsigned)S && (unsigned)y < (unsigned)S) p.put(x, y);
    };
    while (dx >= dy) {
        const int y11 = cy - dy, y12 = cy + dy, y21 = cy - dx, y22 = cy + dx;
        const int x11 = cx - dx, x12 = cx + dx, x21 = cx - dy, x22 = cx + dy;
        if (fill) {
            span(y11, x11, x12); span(y12, x11, x12); span(y21, x21, x22); span(y22, x21, x22);
        } else {
            pt(x11, y11); pt(x12, y11); pt(x11, y12); pt(x12, y12);
            pt(x21, y21); pt(x22, y21); pt(x21, y22); pt(x22, y22);
        }
        dy++;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= 2 & mask;
    }
}

// cv ThickLine, thickness > 1, LINE_8, end points in 16.16; flags bit 0 / bit 1: round cap at p0 / p1
template <class P>
__device__ void thick_line(const P& p, long long p0x, long long p0y, long long p1x, long long p1y, int thickness,
                           int flags) {
    const double INV = 1. / XY_ONE;
    const double dx = (double)(p0x - p1x) * INV, dy = (double)(p1y - p0y) * INV;
    double r = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
    const int odd = thickness & 1;
    const long long th = (long long)thickness << (XY_SHIFT - 1);
    if (fabs(r) > 2.220446049250313e-16) {
        r = __ddiv_rn(__dadd_rn((double)th, (double)odd * (double)XY_ONE * 0.5), sqrt(r));
        const long long dpx = __double2ll_rn(__dmul_rn(dy, r)), dpy = __double2ll_rn(__dmul_rn(dx, r));
        const long long vx[4] = {p0x + dpx, p0x - dpx, p1x - dpx, p1x + dpx};
        const long long vy[4] = {p0y + dpy, p0y - dpy, p1y - dpy, p1y + dpy};
        fill_convex_poly(p, vx, vy, 4);
    }
    const int rad = (int)((th + (XY_ONE >> 1)) >> XY_SHIFT);
    for (int i = 0; i < 2; i++) {
        if (flags & (i + 1))
            circle(p, (int)((p0x + (XY_ONE >> 1)) >> XY_SHIFT), (int)((p0y + (XY_ONE >> 1)) >> XY_SHIFT), rad, 1);
        p0x = p1x; p0y = p1y;
    }
}

__device__ inline int prim_tasks(const vlfm_render_prim& q) {
    return q.kind == VLFM_PRIM_POLYLINE ? (q.n_vtx > 1 ? q.n_vtx - 1 : 0) : 1;
}

template <class P>
__device__ void prim_task(const P& p, const vlfm_render_prim& q, const long long* vtx, int t) {
    switch (q.kind) {
        case VLFM_PRIM_CIRCLE_FILL: circle(p, q.x0, q.y0, q.x1, 1); break;
        case VLFM_PRIM_CIRCLE: circle(p, q.x0, q.y0, q.x1, 0); break;
        case VLFM_PRIM_LINE:
            thick_line(p, (long long)q.x0 << XY_SHIFT, (long long)q.y0 << XY_SHIFT, (long long)q.x1 << XY_SHIFT,
                       (long long)q.y1 << XY_SHIFT, q.thickness, 3);
            break;
        case VLFM_PRIM_POLYLINE: {   // PolyLine(is_closed = false): segment t + 1 from v[t] to v[t + 1]
            const long long* a = vtx + 2 * ((size_t)q.vtx_off + t);
            thick_line(p, a[0], a[1], a[2], a[3], q.thickness, t == 0 ? 3 : 2);
            break;
        }
        default: break;
    }
}

// one workgroup per frame; a run = consecutive primitives with the same colour and flags
__global__ __launch_bounds__(256) void primitive_kernel(const FrameHdr* __restrict__ hdr,
                                                        const int32_t* __restrict__ prim_off,
                                                        const vlfm_render_prim* __restrict__ prims,
                                                        const long long* __restrict__ vtx, int S,
                                                        const uint32_t* __restrict__ path, int rgb,
                                                        unsigned char* __restrict__ out) {
    const int k = blockIdx.x, lane = threadIdx.x, nl = blockDim.x;
    const int stride = (S + 31) >> 5;
    const int a = prim_off[k], b = prim_off[k + 1];
    const uint32_t* plane = path ? path + (size_t)hdr[k].env * S * stride : nullptr;
    for (int i = a; i < b;) {
        const vlfm_render_prim& q0 = prims[i];
        int j = i + 1;
        while (j < b && prims[j].flags == q0.flags && prims[j].bgr[0] == q0.bgr[0] && prims[j].bgr[1] == q0.bgr[1] &&
               prims[j].bgr[2] == q0.bgr[2])
            j++;
        ImagePainter p;
        p.img = out + (size_t)k * S * S * 3;
        p.path = (q0.flags & VLFM_RENDER_UNDER_PATH) ? plane : nullptr;
        p.S = S; p.stride = stride; p.flip = q0.flags & VLFM_RENDER_FLIP_ROWS;
        p.c[0] = q0.bgr[rgb ? 2 : 0]; p.c[1] = q0.bgr[1]; p.c[2] = q0.bgr[rgb ? 0 : 2];
        int g0 = 0;   // task index of the run's first task of primitive m, modulo the lane count
        for (int m = i; m < j; m++) {
            const int nt = prim_tasks(prims[m]);
            for (int t = ((lane - g0) % nl + nl) % nl; t < nt; t += nl) prim_task(p, prims[m], vtx, t);
            g0 = (g0 + nt) % nl;
        }
        __syncthreads();   // the next run paints over this one
        i = j;
    }
}

// one thread per new segment: cv2.line(path_mask, p0, p1, 255, thickness) == ThickLine(flags = 3)
__global__ __launch_bounds__(64) void traj_append_kernel(uint32_t* __restrict__ path, int n_envs, int S,
                                                         const int32_t* __restrict__ segs, int m, int thickness) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= m) return;
    const int32_t* q = segs + 5 * s;
    if ((unsigned)q[0] >= (unsigned)n_envs) return;
    const int stride = (S + 31) >> 5;
    BitPainter p{path + (size_t)q[0] * S * stride, S, stride};
    thick_line(p, (long long)q[1] << XY_SHIFT, (long long)q[2] << XY_SHIFT, (long long)q[3] << XY_SHIFT,
               (long long)q[4] << XY_SHIFT, thickness, 3);
}

}  // namespace render
}  // namespace vlfm

// ================================================================================================ C ABI
using namespace vlfm;
using namespace vlfm::render;

extern "C" size_t vlfm_value_render_scratch_bytes(int n, int map_size) {
    if (n <= 0 || map_size <= 0) return 0;
    return (size_t)n * ((map_size + TILE_ROWS - 1) / TILE_ROWS) * 3 * sizeof(double);
}

extern "C" int vlfm_value_map_render(const double* d_value, int n_envs, int map_size, int channels,
                                     const int32_t* d_frames, int n, int reduce_mode, double explore_thresh,
                                     const double* d_plane, const uint32_t* d_explored, const uint32_t* d_path,
                                     const int32_t* d_prim_off, const vlfm_render_prim* d_prims, const int64_t* d_vtx,
                                     int rgb, void* d_scratch, size_t scratch_bytes, uint8_t* d_out, void* stream) {
    if (n < 0 || n_envs <= 0 || map_size <= 0 || channels <= 0 || !d_frames || !d_out || !d_prim_off || !d_scratch)
        return fail(VLFM_ERR_INVALID, "value_map_render: bad argument");
    if (reduce_mode == VLFM_REDUCE_PLANE ? !d_plane : (!d_value || (reduce_mode != VLFM_REDUCE_MAX &&
                                                                    reduce_mode != VLFM_REDUCE_EXPLORE)))
        return fail(VLFM_ERR_INVALID, "value_map_render: bad reduce mode / input");
    if (reduce_mode == VLFM_REDUCE_EXPLORE && channels < 1)
        return fail(VLFM_ERR_INVALID, "value_map_render: explore reducer needs channel 0");
    if (n == 0) return VLFM_OK;
    if (scratch_bytes < vlfm_value_render_scratch_bytes(n, map_size))
        return fail(VLFM_ERR_CAPACITY, "value_map_render: scratch too small");
    const int S = map_size, tiles = (S + TILE_ROWS - 1) / TILE_ROWS;
    const FrameHdr* hdr = reinterpret_cast<const FrameHdr*>(d_frames);
    Reduce R{d_value, d_plane, d_explored, S, channels, (S + 31) >> 5, reduce_mode, explore_thresh};
    double* partials = static_cast<double*>(d_scratch);
    hipStream_t st = (hipStream_t)stream;
    {
        VLFM_TIMED("value_partials_kernel", st);
        VLFM_KLAUNCH(value_partials_kernel, dim3(tiles, n), dim3(256), 0, st, R, hdr, partials, tiles);
    }
    if (int rc = check_launch("value_partials_kernel")) return rc;
    {
        VLFM_TIMED("value_color_kernel", st);
        VLFM_KLAUNCH(value_color_kernel, dim3((S + 256 * PX - 1) / (256 * PX), n, (S + COLOR_ROWS - 1) / COLOR_ROWS),
                     dim3(256), 0, st, R, hdr, partials, tiles, d_path, rgb, d_out);
    }
    if (int rc = check_launch("value_color_kernel")) return rc;
    if (d_prims) {
        VLFM_TIMED("primitive_kernel", st);
        VLFM_KLAUNCH(primitive_kernel, dim3(n), dim3(256), 0, st, hdr, d_prim_off, d_prims,
                     reinterpret_cast<const long long*>(d_vtx), S, d_path, rgb, d_out);
        if (int rc = check_launch("primitive_kernel")) return rc;
    }
    return VLFM_OK;
}

extern "C" int vlfm_obstacle_map_render(const uint32_t* d_obstacle, const uint32_t* d_navigable,
                                        const uint32_t* d_explored, int n_envs, int map_size, const int32_t* d_frames,
                                        int n, uint32_t pad_bgr, const uint32_t* d_path, const int32_t* d_prim_off,
                                        const vlfm_render_prim* d_prims, const int64_t* d_vtx, int rgb, uint8_t* d_out,
                                        void* stream) {
    if (n < 0 || n_envs <= 0 || map_size <= 0 || !d_obstacle || !d_navigable || !d_explored || !d_frames || !d_out ||
        !d_prim_off)
        return fail(VLFM_ERR_INVALID, "obstacle_map_render: bad argument");
    if (n == 0) return VLFM_OK;
    const int S = map_size;
    const FrameHdr* hdr = reinterpret_cast<const FrameHdr*>(d_frames);
    hipStream_t st = (hipStream_t)stream;
    {
        VLFM_TIMED("obstacle_color_kernel", st);
        VLFM_KLAUNCH(obstacle_color_kernel,
                     dim3((S + 256 * PX - 1) / (256 * PX), n, (S + COLOR_ROWS - 1) / COLOR_ROWS), dim3(256), 0, st,
                     d_obstacle, d_navigable, d_explored, hdr, S, d_path, pad_bgr, rgb, d_out);
    }
    if (int rc = check_launch("obstacle_color_kernel")) return rc;
    if (d_prims) {
        VLFM_TIMED("primitive_kernel", st);
        VLFM_KLAUNCH(primitive_kernel, dim3(n), dim3(256), 0, st, hdr, d_prim_off, d_prims,
                     reinterpret_cast<const long long*>(d_vtx), S, d_path, rgb, d_out);
        if (int rc = check_launch("primitive_kernel")) return rc;
    }
    return VLFM_OK;
}

extern "C" int vlfm_traj_append(uint32_t* d_path, int n_envs, int map_size, const int32_t* d_segs, int m,
                                int thickness, void* stream) {
    if (!d_path || n_envs <= 0 || map_size <= 0 || m < 0 || (m > 0 && !d_segs) || thickness < 2)
        return fail(VLFM_ERR_INVALID, "traj_append: bad argument");
    if (m == 0) return VLFM_OK;
    hipStream_t st = (hipStream_t)stream;
    VLFM_TIMED("traj_append_kernel", st);
    VLFM_KLAUNCH(traj_append_kernel, dim3((m + 63) / 64), dim3(64), 0, st, d_path, n_envs, map_size, d_segs, m,
                 thickness);
    return check_launch("traj_append_kernel");
}
