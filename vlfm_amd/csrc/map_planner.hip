// map_planner.hip -- shortest paths over the navigable planes of ObstacleMapBatch (bit-packed, bitmap.h), n jobs in ONE launch,
// bit for bit vlfm_amd.synthetic.plan_paths_numpy (integers only).  The contract -- jobs, free cells, moves, field, descent,
// statuses -- is stated in full in include/vlfm_amd.h ("Map planner"); this comment is about the layout.
//
// One 1024-thread workgroup per job.  With costs 2 (E/N/W/S) and 3 (diagonals) the field is a sequence of level sets,
//     L[d] = (orthogonal step from L[d-2]  |  diagonal step from L[d-3])  &  free  &  not yet settled,
// swept level by level in this kernel's loop; the moves on bit-packed rows, the bands (here a ring of eight, sweeps widened by
// one row), the order of a level and why its one barrier is enough are stated once, in level_sets.h.
// Six planes per job: `free`, `open` (free and not yet settled) and a ring of four level planes -- level d writes slot d & 3
// while it reads d - 2 and d - 3, and d - 1 must survive for the next level.  Each plane covers the job's window, word-aligned
// to the map's words (no bit shifting on the way in), with one zero word left and right of every row and one zero row above and
// below: no bounds test anywhere, in the sweep or in the descent.  The planes live in LDS when six planes of the call's
// field_h x field_w bound fit 160 KB (a 400 x 400 window: 151 KB), else in a per-job global scratch (L2-resident); the code is
// the same template over the two pointer kinds.
// dist: a uint16 plane in global memory (the caller's field, else scratch), preset to 0xFFFF by a memset node in front of the
// kernel; each cell is stored once, by the level that settles it.  The descent is a single-lane walk behind a release fence, a
// workgroup barrier and an acquire fence.
// Early exit (no fields asked): the sweep stops after the level that settles `start`; every cell with a smaller cost is settled
// by then, and the descent only ever moves to smaller costs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vlfm_amd.h"
#include "bitmap.h"
#include "level_sets.h"
#include "profile.h"
#include "status.h"

namespace vlfm {
namespace planner {
using namespace levels;

constexpr int PLANES = 6;               // free, open, four level planes
constexpr int MAX_RADIUS = 4096;        // vlfm_amd.h: free radii

// words of one plane that holds any window of at most field_h x field_w cells: a run of w columns touches at most
// (w + 30) / 32 + 1 words, plus the two zero words; field_h + 2 rows
__host__ __device__ inline size_t plane_words(int field_h, int field_w) {
    return (size_t)(((field_w + 30) >> 5) + 3) * (size_t)(field_h + 2);
}
inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

template <bool IN_LDS>
__global__ __launch_bounds__(THREADS) void plan_paths_kernel(
    const unsigned* __restrict__ nav, int n_envs, int size, const VlfmPlanJob* __restrict__ jobs, int lookahead, int max_cost,
    uint16_t* fields, int field_h, int field_w, int early, VlfmPlanResult* __restrict__ results, unsigned* g_planes,
    size_t plane_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned smem[];
    int* b_lo = reinterpret_cast<int*>(smem);       // [8] first row of level d, slot d & 7 (NONE: empty)
    int* b_hi = b_lo + 8;                           // [8] last row (-1: empty)
    int* s_start = b_lo + 16;                       // the level that settled `start` (-1: none yet)
    unsigned* planes = IN_LDS ? smem + HEADER_WORDS : g_planes + (size_t)blockIdx.x * PLANES * plane_cap;
    const int tid = threadIdx.x;
    const VlfmPlanJob j = jobs[blockIdx.x];

    // ---- a bad job is answered by its status (uniform for the workgroup: before any barrier)
    bool ok = j.env >= 0 && j.env < n_envs && j.y0 >= 0 && j.x0 >= 0 && j.y1 < size && j.x1 < size && j.y0 <= j.y1 &&
              j.x0 <= j.x1;
    ok = ok && j.y1 - j.y0 + 1 <= field_h && j.x1 - j.x0 + 1 <= field_w;
    ok = ok && j.sx >= j.x0 && j.sx <= j.x1 && j.sy >= j.y0 && j.sy <= j.y1 && j.gx >= j.x0 && j.gx <= j.x1 && j.gy >= j.y0 &&
         j.gy <= j.y1;
    ok = ok && j.start_free >= 0 && j.start_free <= MAX_RADIUS && j.goal_free >= 0 && j.goal_free <= MAX_RADIUS;
    if (!ok) {
        if (tid == 0) {
            VlfmPlanResult r = {};
            r.status = VLFM_PLAN_INVALID; r.cost = 0xFFFF; r.waypoint_x = j.sx; r.waypoint_y = j.sy;
            results[blockIdx.x] = r;
        }
        return;
    }
    const int stride = (size + 31) >> 5;
    const int h = j.y1 - j.y0 + 1;
    const int wx0 = j.x0 >> 5, ws = (j.x1 >> 5) - wx0 + 1;      // the window's words of a map row
    const int P = ws + 2, R = h + 2;                            // plane pitch and rows with the zero border
    unsigned* F = planes;                                       // free
    unsigned* U = planes + plane_cap;                           // open: free and not yet settled
    unsigned* L0 = planes + 2 * plane_cap;                      // level ring: slot s at L0 + s * plane_cap
    uint16_t* dist = fields + (size_t)blockIdx.x * field_h * field_w;
    auto cell = [&](int x, int y) { return (y - j.y0 + 1) * P + (x >> 5) - wx0 + 1; };     // (also for the border cells)

    for (int i = tid; i < P * R; i += THREADS)
        for (int p = 0; p < PLANES; ++p) planes[p * plane_cap + i] = 0u;
    if (tid < 8) { b_lo[tid] = NONE; b_hi[tid] = -1; }
    if (tid == 0) *s_start = -1;
    __syncthreads();
    // ---- free: the navigable bits and the two discs (per row a run of columns cx - hw .. cx + hw, hw = floor(sqrt(r*r - dy*dy))),
    // inside the window; every word is built by one lane, no atomics
    const unsigned* nv = nav + (size_t)j.env * size * stride;
    for (int i = tid; i < h * ws; i += THREADS) {
        const int r = i / ws, k = i - r * ws;
        const int xb = (wx0 + k) * 32, y = j.y0 + r;            // column of the word's bit 0
        unsigned v = nv[(size_t)y * stride + wx0 + k];
        for (int which = 0; which < 2; ++which) {
            const int cx = which ? j.gx : j.sx, dy = y - (which ? j.gy : j.sy), rad = which ? j.goal_free : j.start_free;
            const int rest = rad * rad - dy * dy;
            if (rest < 0) continue;
            int hw = (int)sqrtf((float)rest);
            while ((hw + 1) * (hw + 1) <= rest) ++hw;
            while (hw * hw > rest) --hw;
            const int lo = max(cx - hw, xb) - xb, hi = min(cx + hw, xb + 31) - xb;
            if (lo <= hi) v |= (~0u << lo) & (~0u >> (31 - hi));
        }
        unsigned m = ~0u;
        if (xb < j.x0) m &= ~0u << (j.x0 - xb);
        if (xb + 31 > j.x1) m &= ~0u >> (xb + 31 - j.x1);
        F[(r + 1) * P + k + 1] = v & m;
    }
    __syncthreads();
    for (int i = tid; i < P * R; i += THREADS) U[i] = F[i];
    __syncthreads();
    const int si = cell(j.sx, j.sy), gi = cell(j.gx, j.gy);
    const unsigned sb = 1u << (j.sx & 31), gb = 1u << (j.gx & 31);
    if (tid == 0) {                                             // level 0: the goal
        U[gi] &= ~gb;
        L0[gi] = gb;
        b_lo[0] = b_hi[0] = j.gy - j.y0;
        dist[(size_t)(j.gy - j.y0) * field_w + (j.gx - j.x0)] = 0;
        if (si == gi && sb == gb) *s_start = 0;
    }
    __syncthreads();

    // ---- levels (the order of a level: level_sets.h)
    int too_long = 0;
    const int last = max_cost + 3;      // a cell beyond max_cost shows in one of the three levels after it
    for (int d = 1;; ++d) {
        const int hi1 = b_hi[(d + 7) & 7];
        const int lo2 = b_lo[(d + 6) & 7], hi2 = b_hi[(d + 6) & 7];
        const int lo3 = b_lo[(d + 5) & 7], hi3 = b_hi[(d + 5) & 7];
        const int lo4 = b_lo[(d + 4) & 7], hi4 = b_hi[(d + 4) & 7];      // what the slot this level writes still holds
        // (a lane that is already inside level d may store d here while another still reads: a value >= d is "not yet")
        const int seen = *s_start, settled = seen < d ? seen : -1;
        if (d - 1 > max_cost && hi1 >= 0) { too_long = 1; break; }
        if (settled >= 0 && (early || d > max_cost)) break;
        if (d > last) break;
        if (hi1 < 0 && hi2 < 0 && hi3 < 0) break;                        // ran dry
        const bool have = hi2 >= 0 || hi3 >= 0;
        int n0 = 1, n1 = 0;                                              // rows this level can set
        if (have) {
            n0 = max(min(hi2 >= 0 ? lo2 : NONE, hi3 >= 0 ? lo3 : NONE) - 1, 0);
            n1 = min(max(hi2, hi3) + 1, h - 1);
        }
        int s0 = n0, s1 = n1;                                            // rows to write: those, and the slot's stale ones
        if (hi4 >= 0) {
            s0 = have ? min(n0, lo4) : lo4;
            s1 = have ? max(n1, hi4) : hi4;
        }
        unsigned* Ld = L0 + (size_t)(d & 3) * plane_cap;
        const unsigned* A = L0 + (size_t)((d + 2) & 3) * plane_cap;      // L[d-2]
        const unsigned* B = L0 + (size_t)((d + 1) & 3) * plane_cap;      // L[d-3]
        int my_lo = NONE, my_hi = -1;
        const int total = (s1 - s0 + 1) * ws;
        for (int i = tid; i < total; i += THREADS) {
            const int q = i / ws, r = s0 + q, k = i - q * ws;
            const int c = (r + 1) * P + k + 1;
            unsigned out = 0u, u = 0u;
            if (r >= n0 && r <= n1 && (u = U[c]) != 0u) {
                out = (straight_into(A, c, P) | diagonal_into(B, F, c, -P) | diagonal_into(B, F, c, P)) & u;
            }
            Ld[c] = out;
            if (out) {
                U[c] = u & ~out;
                my_lo = min(my_lo, r);
                my_hi = max(my_hi, r);
                if (c == si && (out & sb)) *s_start = d;
                if (d <= max_cost) {
                    uint16_t* row = dist + (size_t)r * field_w + ((wx0 + k) * 32 - j.x0);
                    for (unsigned m = out; m; m &= m - 1) row[__ffs(m) - 1] = (uint16_t)d;
                }
            }
        }
        if (my_hi >= 0) {
            atomicMin(&b_lo[d & 7], my_lo);
            atomicMax(&b_hi[d & 7], my_hi);
        }
        if (tid == 0) { b_lo[(d + 1) & 7] = NONE; b_hi[(d + 1) & 7] = -1; }   // (last read as level d - 7)
        __syncthreads();
    }

    // ---- the descent: one lane, after every lane's cell stores are visible to it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (tid != 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int settled = *s_start;
    VlfmPlanResult res = {};
    res.cost = 0xFFFF; res.waypoint_x = j.sx; res.waypoint_y = j.sy;
    if (settled < 0 || settled > max_cost) {
        res.status = (too_long || settled > max_cost) ? VLFM_PLAN_TOO_LONG : VLFM_PLAN_UNREACHABLE;
        results[blockIdx.x] = res;
        return;
    }
    auto is_free = [&](int x, int y) { return (F[cell(x, y)] >> (x & 31)) & 1u; };
    auto dist_at = [&](int x, int y) { return (int)dist[(size_t)(y - j.y0) * field_w + (x - j.x0)]; };
    int cx = j.sx, cy = j.sy, dc = dist_at(cx, cy), steps = 0;
    res.cost = dc;
    while (dc > 0 && steps < lookahead) {
        int s = 0;
        for (; s < 8; ++s) {
            const int dx = code_dx(s), dy = code_dy(s), nx = cx + dx, ny = cy + dy;
            if (!is_free(nx, ny)) continue;                              // (the zero border: never outside the window)
            if ((s & 1) && !(is_free(nx, cy) && is_free(cx, ny))) continue;
            if (dist_at(nx, ny) + ((s & 1) ? 3 : 2) != dc) continue;
            cx = nx; cy = ny;
            dc -= (s & 1) ? 3 : 2;
            ++steps;
            break;
        }
        if (s == 8) break;                                               // (cannot happen: a settled cell has a predecessor)
    }
    res.status = VLFM_PLAN_OK;
    res.waypoint_x = cx; res.waypoint_y = cy; res.steps = steps;
    results[blockIdx.x] = res;
}

}  // namespace planner
}  // namespace vlfm

using namespace vlfm;
using namespace vlfm::planner;

extern "C" size_t vlfm_plan_scratch_bytes(int n_jobs, int size) {
    if (n_jobs <= 0 || size <= 0 || size > 2048) return 0;
    return align16((size_t)n_jobs * size * size * sizeof(uint16_t)) +
           (size_t)n_jobs * PLANES * plane_words(size, size) * sizeof(unsigned);
}

extern "C" int vlfm_plan_paths(const int32_t* d_navigable, int n_envs, int size, const VlfmPlanJob* d_jobs, int n_jobs,
                               int lookahead, int max_cost, uint16_t* d_fields, int field_h, int field_w,
                               VlfmPlanResult* d_results, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (n_envs < 1 || size < 1 || size > 2048 || n_jobs < 0 || lookahead < 0 || max_cost < 0 || max_cost > 65534 ||
        field_h < 1 || field_w < 1 || field_h > size || field_w > size || !d_navigable ||
        (n_jobs > 0 && (!d_jobs || !d_results || !d_scratch)))
        return fail(VLFM_ERR_INVALID, "plan_paths: bad argument (size <= 2048, max_cost <= 65534, 1 <= field <= size)");
    if (n_jobs == 0) return VLFM_OK;
    if (scratch_bytes < vlfm_plan_scratch_bytes(n_jobs, size))
        return fail(VLFM_ERR_CAPACITY, "plan_paths: scratch smaller than vlfm_plan_scratch_bytes(n_jobs, size)");
    hipStream_t st = (hipStream_t)stream;
    // scratch: [the dist planes of a call without fields][PLANES planes per job for the global residence]
    uint16_t* dist = d_fields ? d_fields : reinterpret_cast<uint16_t*>(d_scratch);
    unsigned* g_planes = reinterpret_cast<unsigned*>(static_cast<char*>(d_scratch) +
                                                     align16((size_t)n_jobs * size * size * sizeof(uint16_t)));
    if (hipMemsetAsync(dist, 0xFF, (size_t)n_jobs * field_h * field_w * sizeof(uint16_t), st) != hipSuccess)
        return fail(VLFM_ERR_HIP, "plan_paths: cannot preset the dist planes");
    const size_t lds = HEADER_WORDS * sizeof(unsigned) + PLANES * plane_words(field_h, field_w) * sizeof(unsigned);
    const unsigned* nav = reinterpret_cast<const unsigned*>(d_navigable);
    const int early = d_fields ? 0 : 1;
    VLFM_TIMED("plan_paths_kernel", st);
    if (lds <= LDS_BYTES_MAX) {
        static LdsOptIn opt;
        if (lds > 64 * 1024 && !opt.ensure(reinterpret_cast<const void*>(plan_paths_kernel<true>), lds))
            return fail(VLFM_ERR_HIP, "plan_paths: cannot opt in to the LDS size");
        VLFM_KLAUNCH(plan_paths_kernel<true>, dim3(n_jobs), dim3(THREADS), lds, st, nav, n_envs, size, d_jobs, lookahead,
                     max_cost, dist, field_h, field_w, early, d_results, (unsigned*)nullptr, plane_words(field_h, field_w));
        const int rc = check_launch("plan_paths_kernel");
        return rc == VLFM_OK ? VLFM_PLAN_IN_LDS : rc;
    }
    VLFM_KLAUNCH(plan_paths_kernel<false>, dim3(n_jobs), dim3(THREADS), HEADER_WORDS * sizeof(unsigned), st, nav, n_envs, size,
                 d_jobs, lookahead, max_cost, dist, field_h, field_w, early, d_results, g_planes, plane_words(size, size));
    const int rc = check_launch("plan_paths_kernel");
    return rc == VLFM_OK ? VLFM_PLAN_IN_SCRATCH : rc;
}
