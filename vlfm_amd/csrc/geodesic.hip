// geodesic.hip -- shortest collision-free path lengths in the rooms world, for the ObjectNav metrics (SPL, SoftSPL,
// distance_to_goal): the geodesic fields of n environments in ONE launch and the distances of m points in ONE launch, bit for
// bit vlfm_amd.synthetic.geodesic_field_numpy / geodesic_query_numpy (f64, one rounding per operation: the library is built with
// -ffp-contract=off and the expressions below go through __dadd_rn / __dsub_rn / __dmul_rn / __dsqrt_rn and true divisions).
//
//   rectangles  the wall boxes of the field's world, then the environment's valid object footprints in slot order, each inflated to
//               (x0 - m, y0 - m, x1 + m, y1 + m); OPEN sets
//   blocked     p -> q is blocked by a rectangle iff max(enter_x, enter_y, 0) < min(exit_x, exit_y, 1), where per axis, with
//               d = q - p:  d == 0: (-inf, inf) if lo < p < hi, else empty;  otherwise t0 = (lo - p) / d, t1 = (hi - p) / d and
//               (enter, exit) = (min(t0, t1), max(t0, t1)).  Evaluated FROM p TO q: source -> corner, corner of lower index ->
//               corner of higher index (one verdict per pair), query point -> source or corner
//   nodes       the corners (x0,y0) (x1,y0) (x1,y1) (x0,y1) of every rectangle, in order, without those strictly inside a rectangle
//   w(a, b)     sqrt(dx*dx + dy*dy)
//   field       the least dist with dist[c] = min(min over the sources s that see c of w(s, c),
//                                                 min over the corners u that see c of fl(dist[u] + w(u, c)))
//   query       d(p) = min(min over the sources p sees of w(p, s), min over the corners p sees of fl(w(p, c) + dist[c]))
//
// Field kernel: one 1024-thread workgroup per environment.  Rectangles, nodes, the node-to-node visibility bitmap and two copies
// of dist sit in LDS.  The pair tests are spread over the lanes (a pair's verdict is OR-ed into both rows of the bitmap, the
// source distances are min-ed into dist as unsigned 64-bit integers -- non-negative doubles order like their bit patterns;
// OR and min commute, so the result does not depend on the order).  Then Jacobi rounds: every node takes the minimum over the
// nodes it sees of the PREVIOUS round's dist plus the edge, rounds separated by barriers, until a workgroup-uniform "changed"
// flag stays clear.  Adding a non-negative weight never decreases a value, so every intermediate value is the length of a real
// path (never below the least fixed point) and the state the rounds stop in is that fixed point: what Dijkstra returns.  A
// shortest path visits no node twice, so N rounds suffice; the loop is capped there.
// The work is chains of f64 divisions and roots with little to overlap inside a lane, and a 256-environment launch puts ONE
// workgroup on each CU, so the workgroup is made as large as it can be: measured at 256 environments of the rooms world, 905 us
// with 256 threads, 581 us with 512, 433 us with 1024 ("ObjectNav metrics").
// Query kernel: one 256-thread workgroup per point; sources and nodes spread over the lanes, an LDS min-reduction at the end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vlfm_amd.h"
#include "profile.h"
#include "status.h"
#include "world_table.h"

namespace vlfm {
namespace geodesic {

constexpr int THREADS = 256;            // query kernel
constexpr int FIELD_THREADS = 1024;     // field kernel: 16 waves, the one workgroup a CU gets (see the note above)
constexpr int MAX_OBJECTS = 8;                // vlfm_amd.h: objects per environment
constexpr int OBJ_REC = 8;                    // doubles per object record: x0 y0 x1 y1 z0 z1 valid pad

// one axis of the blocked test: narrows (enter, leave) by the parameter interval in which p + t d lies strictly inside (lo, hi)
__device__ __forceinline__ void axis_interval(double p, double q, double lo, double hi, double& enter, double& leave) {
    const double d = __dsub_rn(q, p);
    double a, b;
    if (d == 0.0) {
        const bool inside = lo < p && p < hi;
        a = inside ? -__builtin_inf() : __builtin_inf();
        b = inside ? __builtin_inf() : -__builtin_inf();
    } else {
        const double t0 = __dsub_rn(lo, p) / d, t1 = __dsub_rn(hi, p) / d;
        a = fmin(t0, t1);
        b = fmax(t0, t1);
    }
    enter = fmax(enter, a);
    leave = fmin(leave, b);
}

// is the segment (px, py) -> (qx, qy) blocked by one of the n_rects open rectangles in `rects` (LDS)
// A rectangle whose open interval on one axis does not meet the segment's extent there is skipped without the divisions; the
// verdict is the rule's own.  Say both ends are <= lo (>= hi mirrors it), d = fl(q - p):  d == 0: p is not inside, the interval
// is empty;  d > 0: rounding is monotone, so q <= lo gives d <= fl(lo - p), t0 >= 1, enter >= 1 >= exit;  d < 0: lo - p >= 0 and
// hi - p > 0 give t0 <= 0 and t1 < 0, exit <= 0 <= enter.
__device__ __forceinline__ bool blocked(double px, double py, double qx, double qy, const double* rects, int n_rects) {
    const double xmin = fmin(px, qx), xmax = fmax(px, qx), ymin = fmin(py, qy), ymax = fmax(py, qy);
    for (int r = 0; r < n_rects; ++r) {
        const double x0 = rects[4 * r + 0], y0 = rects[4 * r + 1], x1 = rects[4 * r + 2], y1 = rects[4 * r + 3];
        if (xmax <= x0 || xmin >= x1 || ymax <= y0 || ymin >= y1) continue;
        double enter = 0.0, leave = 1.0;
        axis_interval(px, qx, x0, x1, enter, leave);
        axis_interval(py, qy, y0, y1, enter, leave);
        if (enter < leave) return true;
    }
    return false;
}

__device__ __forceinline__ double weight(double ax, double ay, double bx, double by) {
    const double dx = __dsub_rn(ax, bx), dy = __dsub_rn(ay, by);
    return __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
}

// LDS of the field kernel for `max_rects` rectangles: rectangles, nodes, two dist arrays, keep flags, the bitmap
__host__ __device__ inline size_t field_lds_bytes(int max_rects) {
    const size_t nn = 4 * (size_t)max_rects, wpr = (nn + 31) / 32;
    return (size_t)max_rects * 32 + nn * 16 + 2 * nn * 8 + nn * 4 + nn * wpr * 4;
}

// A field finds its wall boxes in the row of its world in the table (world_table.h).  walls.capacity() + 8 is R, the stride of
// the outputs; the field's own count varies below it.
__global__ __launch_bounds__(FIELD_THREADS) void geodesic_fields_kernel(
    const WorldBoxes walls, double margin, const double* __restrict__ objects,
    const double* __restrict__ sources, const int32_t* __restrict__ source_counts, int max_sources, double* __restrict__ out_rects,
    double* __restrict__ out_nodes, double* __restrict__ out_dist, int32_t* __restrict__ out_counts) {
    extern __shared__ double smem[];
    const int env = blockIdx.x, tid = threadIdx.x;
    int n_boxes;
    const double* __restrict__ boxes = walls.find(env, n_boxes);
    const int max_rects = walls.capacity() + MAX_OBJECTS, max_nodes = 4 * max_rects, wpr = (max_nodes + 31) / 32;
    double* rects = smem;                                   // [max_rects][4]
    double* nodes = rects + 4 * max_rects;                  // [max_nodes][2]
    double* dist_a = nodes + 2 * max_nodes;                 // [max_nodes]
    double* dist_b = dist_a + max_nodes;                    // [max_nodes]
    int* keep = reinterpret_cast<int*>(dist_b + max_nodes); // [max_nodes]: is the candidate corner a node
    uint32_t* sees = reinterpret_cast<uint32_t*>(keep + max_nodes);   // [max_nodes][wpr]
    const double inf = __builtin_inf();

    // ---- rectangles: the walls, then the valid object slots in slot order (every lane counts the 8 slots itself)
    const double* obj = objects + (size_t)env * MAX_OBJECTS * OBJ_REC;
    int n_rects = n_boxes;
    for (int k = 0; k < MAX_OBJECTS; ++k) n_rects += obj[OBJ_REC * k + 6] != 0.0 ? 1 : 0;
    for (int r = tid; r < max_rects; r += FIELD_THREADS) {
        const double* b = nullptr;
        if (r < n_boxes) {
            b = boxes + 4 * r;
        } else {
            int seen = n_boxes;
            for (int k = 0; k < MAX_OBJECTS && !b; ++k)
                if (obj[OBJ_REC * k + 6] != 0.0 && seen++ == r) b = obj + OBJ_REC * k;
        }
        rects[4 * r + 0] = b ? __dsub_rn(b[0], margin) : 0.0;
        rects[4 * r + 1] = b ? __dsub_rn(b[1], margin) : 0.0;
        rects[4 * r + 2] = b ? __dadd_rn(b[2], margin) : 0.0;
        rects[4 * r + 3] = b ? __dadd_rn(b[3], margin) : 0.0;
    }
    __syncthreads();
    // ---- nodes: the corners that are strictly inside no rectangle, compacted in order
    const int n_cand = 4 * n_rects;
    for (int i = tid; i < n_cand; i += FIELD_THREADS) {
        const int r = i >> 2, c = i & 3;
        const double x = rects[4 * r + ((c == 1 || c == 2) ? 2 : 0)], y = rects[4 * r + (c >= 2 ? 3 : 1)];
        bool in = false;
        for (int k = 0; k < n_rects && !in; ++k)
            in = rects[4 * k + 0] < x && x < rects[4 * k + 2] && rects[4 * k + 1] < y && y < rects[4 * k + 3];
        keep[i] = in ? 0 : 1;
    }
    __syncthreads();
    int n_nodes = 0;                                        // (every lane counts all flags: uniform without another barrier)
    for (int i = 0; i < n_cand; ++i) n_nodes += keep[i];
    for (int i = tid; i < n_cand; i += FIELD_THREADS) {
        if (!keep[i]) continue;
        int at = 0;
        for (int j = 0; j < i; ++j) at += keep[j];
        const int r = i >> 2, c = i & 3;
        nodes[2 * at + 0] = rects[4 * r + ((c == 1 || c == 2) ? 2 : 0)];
        nodes[2 * at + 1] = rects[4 * r + (c >= 2 ? 3 : 1)];
    }
    for (int i = tid; i < max_nodes; i += FIELD_THREADS) dist_a[i] = inf;
    for (int i = tid; i < max_nodes * wpr; i += FIELD_THREADS) sees[i] = 0u;
    __syncthreads();
    // ---- the sources' direct distances (min as unsigned 64-bit integers: all values are non-negative doubles)
    int n_src = source_counts[env];
    n_src = n_src < 0 ? 0 : (n_src > max_sources ? max_sources : n_src);
    const double* src = sources + (size_t)env * max_sources * 2;
    for (int idx = tid; idx < n_nodes * n_src; idx += FIELD_THREADS) {
        const int c = idx / n_src, s = idx - c * n_src;
        const double sx = src[2 * s], sy = src[2 * s + 1], cx = nodes[2 * c], cy = nodes[2 * c + 1];
        if (blocked(sx, sy, cx, cy, rects, n_rects)) continue;
        atomicMin(reinterpret_cast<unsigned long long*>(dist_a + c), (unsigned long long)__double_as_longlong(weight(sx, sy, cx, cy)));
    }
    // ---- which corner sees which: the pair (a, b), a < b, is tested once, from a to b
    for (int idx = tid; idx < n_nodes * n_nodes; idx += FIELD_THREADS) {
        const int a = idx / n_nodes, b = idx - a * n_nodes;
        if (a >= b) continue;
        if (blocked(nodes[2 * a], nodes[2 * a + 1], nodes[2 * b], nodes[2 * b + 1], rects, n_rects)) continue;
        atomicOr(sees + a * wpr + (b >> 5), 1u << (b & 31));
        atomicOr(sees + b * wpr + (a >> 5), 1u << (a & 31));
    }
    __syncthreads();
    // ---- Jacobi rounds from the goal outwards
    double* cur = dist_a;
    double* nxt = dist_b;
    for (int round = 0; round < n_nodes; ++round) {
        int changed = 0;
        for (int c = tid; c < n_nodes; c += FIELD_THREADS) {
            const double cx = nodes[2 * c], cy = nodes[2 * c + 1], old = cur[c];
            double best = old;
            for (int wd = 0; wd < wpr; ++wd) {
                uint32_t bits = sees[c * wpr + wd];
                while (bits) {
                    const int u = 32 * wd + __ffs(bits) - 1;
                    bits &= bits - 1;
                    const double du = cur[u];
                    if (du < best) best = fmin(best, __dadd_rn(du, weight(nodes[2 * u], nodes[2 * u + 1], cx, cy)));
                }
            }
            nxt[c] = best;
            changed |= best != old;
        }
        const int any = __syncthreads_or(changed);          // (also the barrier between the rounds)
        double* t = cur;
        cur = nxt;
        nxt = t;
        if (!any) break;
    }
    // ---- out: the tables' unused tails are zero nodes / rectangles at infinite distance
    double* g_rects = out_rects + (size_t)env * max_rects * 4;
    double* g_nodes = out_nodes + (size_t)env * max_nodes * 2;
    double* g_dist = out_dist + (size_t)env * max_nodes;
    for (int i = tid; i < 4 * max_rects; i += FIELD_THREADS) g_rects[i] = i < 4 * n_rects ? rects[i] : 0.0;
    for (int i = tid; i < 2 * max_nodes; i += FIELD_THREADS) g_nodes[i] = i < 2 * n_nodes ? nodes[i] : 0.0;
    for (int i = tid; i < max_nodes; i += FIELD_THREADS) g_dist[i] = i < n_nodes ? cur[i] : inf;
    if (tid == 0) {
        out_counts[2 * env + 0] = n_rects;
        out_counts[2 * env + 1] = n_nodes;
    }
}

__global__ __launch_bounds__(THREADS) void geodesic_query_kernel(
    const double* __restrict__ points, const int32_t* __restrict__ field_of, int n_fields, int max_rects,
    const double* __restrict__ f_rects, const double* __restrict__ f_nodes, const double* __restrict__ f_dist,
    const int32_t* __restrict__ f_counts, const double* __restrict__ sources, const int32_t* __restrict__ source_counts,
    int max_sources, double* __restrict__ out) {
    extern __shared__ double smem[];
    double* rects = smem;                                   // [max_rects][4]
    double* red = rects + 4 * max_rects;                    // [THREADS]
    const int tid = threadIdx.x, max_nodes = 4 * max_rects;
    const int f = field_of[blockIdx.x];
    if (f < 0 || f >= n_fields) {                           // (uniform for the workgroup: before any barrier) no field: NaN
        if (tid == 0) out[blockIdx.x] = __builtin_nan("");
        return;
    }
    int n_rects = f_counts[2 * f], n_nodes = f_counts[2 * f + 1], n_src = source_counts[f];
    n_rects = n_rects < 0 ? 0 : (n_rects > max_rects ? max_rects : n_rects);
    n_nodes = n_nodes < 0 ? 0 : (n_nodes > max_nodes ? max_nodes : n_nodes);
    n_src = n_src < 0 ? 0 : (n_src > max_sources ? max_sources : n_src);
    for (int i = tid; i < 4 * n_rects; i += THREADS) rects[i] = f_rects[(size_t)f * max_rects * 4 + i];
    __syncthreads();
    const double px = points[2 * blockIdx.x], py = points[2 * blockIdx.x + 1];
    const double* src = sources + (size_t)f * max_sources * 2;
    const double* nodes = f_nodes + (size_t)f * max_nodes * 2;
    const double* dist = f_dist + (size_t)f * max_nodes;
    double best = __builtin_inf();
    for (int i = tid; i < n_src + n_nodes; i += THREADS) {
        const bool is_src = i < n_src;
        const int c = is_src ? i : i - n_src;
        const double qx = is_src ? src[2 * c] : nodes[2 * c], qy = is_src ? src[2 * c + 1] : nodes[2 * c + 1];
        const double far = is_src ? 0.0 : dist[c];
        if (!(far < best)) continue;                        // (w >= 0: cannot improve; also skips unreachable corners)
        if (blocked(px, py, qx, qy, rects, n_rects)) continue;
        const double w = weight(px, py, qx, qy);
        best = fmin(best, is_src ? w : __dadd_rn(w, far));
    }
    red[tid] = best;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmin(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = red[0];
}

}  // namespace geodesic
}  // namespace vlfm

using namespace vlfm;
using namespace vlfm::geodesic;

extern "C" int vlfm_geodesic_fields(const double* d_world_boxes, const int32_t* d_box_counts, int n_worlds, int max_boxes,
                                    const int32_t* d_world_of, double margin, const double* d_objects, const double* d_sources,
                                    const int32_t* d_source_counts, int n, int max_sources, double* d_rects, double* d_nodes,
                                    double* d_dist, int32_t* d_counts, void* stream) {
    if (n < 0 || n_worlds < 0 || max_boxes < 0 || max_boxes > 16384 || max_sources < 0 || !(margin == margin) ||
        (n_worlds > 0 && (!d_box_counts || (max_boxes > 0 && !d_world_boxes))) ||
        (n > 0 && (!d_world_of || !d_objects || !d_source_counts || !d_rects || !d_nodes || !d_dist || !d_counts)) ||
        (n > 0 && max_sources > 0 && !d_sources))
        return fail(VLFM_ERR_INVALID, "geodesic_fields: bad argument");
    if (n == 0) return VLFM_OK;
    const size_t lds = field_lds_bytes(max_boxes + MAX_OBJECTS);
    if (lds > 64 * 1024)
        return fail(VLFM_ERR_INVALID, "geodesic_fields: rectangles, nodes and the visibility bitmap exceed 64 KB of LDS");
    hipStream_t st = (hipStream_t)stream;
    VLFM_TIMED("geodesic_fields_kernel", st);
    VLFM_KLAUNCH(geodesic_fields_kernel, dim3(n), dim3(FIELD_THREADS), lds, st,
                 WorldBoxes{d_world_boxes, d_box_counts, d_world_of, n_worlds, max_boxes}, margin, d_objects, d_sources,
                 d_source_counts, max_sources, d_rects, d_nodes, d_dist, d_counts);
    return check_launch("geodesic_fields_kernel");
}

extern "C" int vlfm_geodesic_query(const double* d_points, const int32_t* d_field_of, int m, int n_fields, int n_boxes,
                                   const double* d_rects, const double* d_nodes, const double* d_dist, const int32_t* d_counts,
                                   const double* d_sources, const int32_t* d_source_counts, int max_sources, double* d_out,
                                   void* stream) {
    if (m < 0 || n_fields < 0 || n_boxes < 0 || n_boxes > 16384 || max_sources < 0 ||
        (m > 0 && (!d_points || !d_field_of || !d_out)) ||
        (m > 0 && n_fields > 0 && (!d_rects || !d_nodes || !d_dist || !d_counts || !d_source_counts)) ||
        (m > 0 && n_fields > 0 && max_sources > 0 && !d_sources))
        return fail(VLFM_ERR_INVALID, "geodesic_query: bad argument");
    if (m == 0) return VLFM_OK;
    const int max_rects = n_boxes + MAX_OBJECTS;
    const size_t lds = (size_t)max_rects * 32 + THREADS * 8;
    if (lds > 64 * 1024) return fail(VLFM_ERR_INVALID, "geodesic_query: the rectangles exceed 64 KB of LDS");
    hipStream_t st = (hipStream_t)stream;
    VLFM_TIMED("geodesic_query_kernel", st);
    VLFM_KLAUNCH(geodesic_query_kernel, dim3(m), dim3(THREADS), lds, st, d_points, d_field_of, n_fields, max_rects, d_rects,
                 d_nodes, d_dist, d_counts, d_sources, d_source_counts, max_sources, d_out);
    return check_launch("geodesic_query_kernel");
}
