// lattice_geodesic.hip -- the ObjectNav metrics' geodesic on a metric lattice with integer costs, for worlds the visibility graph
// (geodesic.hip) cannot hold: grid worlds and box worlds beyond 141 rectangles.  Bit for bit vlfm_amd.synthetic's "Lattice
// geodesic" section (lattice_free_numpy / lattice_field_numpy / lattice_query_numpy); the rule -- lattice, free nodes, the 16
// moves with costs 5 / 7 / 11 and their intermediate nodes, sources, field, query -- is stated in full in include/vlfm_amd.h
// ("Lattice geodesic").  This comment is about the layout.
//
// lattice_free_kernel: one lane per node, a wave per run of 64 nodes of a row; the lanes' verdicts are packed by a ballot and
// stored by lane 0 as two words.  Boxes, object records, grid edges and grid bits are read from global memory (wave-uniform or
// neighbouring addresses), as the ray caster reads them.  Grid cells: two strict binary searches per axis bound the block of
// cells whose inflated boxes hold the node; the block's bits are ORed row by row.
//
// lattice_fields_kernel: one 1024-thread workgroup per field.  With integer costs the field is a sequence of level sets,
//     L[d] = (straight(L[d-5]) | diagonal(L[d-7]) | knight(L[d-11])) & free & ~settled,
// swept level by level in this kernel's loop; the straight and diagonal moves on bit-packed rows, the bands (here a ring of
// sixteen, sweeps widened by two rows), the order of a level and why its one barrier is enough are stated once, in level_sets.h.
// The knight moves are this file's own:
//     knight 2s,t  source (x - 2s, y - t): both intermediate nodes stand in column x - s, in the source's and in the target's
//                  row: shift by one, AND with both rows of `free`, shift by one more.  Two bits cross a word boundary: the
//                  second shift's carry is the top (bottom) bit of the neighbouring word's intermediate, built from that word
//     knight s,2t  source (x - s, y - 2t): AND with the row between at the source's column, shift, AND with it at the target's
// Fourteen planes per field: `free`, `open` (free and not yet settled) and a ring of twelve level planes -- level d writes slot
// d % 12 while it reads d - 5, d - 7 and d - 11, and d - 1 .. d - 4 must survive for the levels to come.  A plane has one zero
// word left and right of every row and two zero rows above and below: no bounds test anywhere in the sweep.  The planes live
// in LDS when fourteen planes of the call's max_nb x max_na bound fit 160 KB (e.g. 256 x 256: 142 KB); else `free` and `open`
// stay in LDS while two planes fit (up to about 780 x 780; the rooms world's 449 x 449: 62 KB) and the ring goes to a per-field
// global scratch (L2-resident): a word's first question -- has it an open bit -- is then answered without a trip to L2, and the
// level loads go out together; beyond that all fourteen live in the scratch.  One template over the three layouts.
// A level whose three source levels are empty only clears the slot it overwrites.  The search ends after eleven empty levels in
// a row (level_sets.h) or past max_cost.
// dist: uint16 [max_nb][max_na] per field in global memory, preset to 0xFFFF by a memset in front of the kernel; each node is
// stored once, by the level that settles it, with ordinary vector stores.
// lattice_query_kernel: one lane per point, four nodes each; f64, one rounding per operation (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vlfm_amd.h"
#include "level_sets.h"
#include "profile.h"
#include "status.h"
#include "world_table.h"

namespace vlfm {
namespace lattice {
using namespace levels;                 // (THREADS: the fields kernel's)

constexpr int SMALL_THREADS = 256;      // free and query kernels
constexpr int PLANES = 14;              // free, open, twelve level planes
constexpr int RING = 12;
constexpr int MAX_NODES = VLFM_LATTICE_MAX_NODES;
constexpr int MAX_OBJECTS = 8;          // vlfm_amd.h: objects per environment
constexpr int OBJ_REC = 8;              // doubles per object record: x0 y0 x1 y1 z0 z1 valid pad

// words of one plane that holds any lattice of at most max_nb x max_na nodes: the row's words and the two zero words, nb + 4 rows
__host__ __device__ inline size_t plane_words(int max_nb, int max_na) {
    return (size_t)(((max_na + 31) >> 5) + 2) * (size_t)(max_nb + 4);
}
// Where the planes of a call live (the same for every field of it): everything in LDS; `free` and `open` in LDS and the level ring
// in the scratch; everything in the scratch.
enum Residence { ALL_LDS = 0, RING_IN_SCRATCH = 1, ALL_IN_SCRATCH = 2 };
inline size_t lds_bytes(int lds_planes, int max_nb, int max_na) {
    return (HEADER_WORDS + lds_planes * plane_words(max_nb, max_na)) * sizeof(unsigned);
}
inline Residence residence_of(int max_nb, int max_na) {
    if (lds_bytes(PLANES, max_nb, max_na) <= LDS_BYTES_MAX) return ALL_LDS;
    return lds_bytes(2, max_nb, max_na) <= LDS_BYTES_MAX ? RING_IN_SCRATCH : ALL_IN_SCRATCH;
}
inline int scratch_planes(Residence r) { return r == ALL_LDS ? 0 : (r == RING_IN_SCRATCH ? RING : PLANES); }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- free ---------------------------------------------------------------------------------------------------------------------
// the cells i of an axis with edges[i] - m < v < edges[i + 1] + m are [first, last): both sides are monotone in i
__device__ __forceinline__ void strict_run(const double* __restrict__ edges, int n, double m, double v, int& first, int& last) {
    int lo = 0, hi = n;
    while (lo < hi) {                                   // how many cells have edges[i + 1] + m <= v
        const int mid = (lo + hi) >> 1;
        if (__dadd_rn(edges[mid + 1], m) <= v) lo = mid + 1; else hi = mid;
    }
    first = lo;
    lo = 0, hi = n;
    while (lo < hi) {                                   // how many cells have edges[i] - m < v
        const int mid = (lo + hi) >> 1;
        if (__dsub_rn(edges[mid], m) < v) lo = mid + 1; else hi = mid;
    }
    last = lo;
}

__global__ __launch_bounds__(SMALL_THREADS) void lattice_free_kernel(
    const WorldBoxes table, const WorldGrids grids, double margin, const double* __restrict__ objects,
    const int32_t* __restrict__ dims, int cells_per_metre, int max_nb, int max_na, unsigned* __restrict__ out) {
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    const int segs = (max_na + 63) >> 6, words = (max_na + 31) >> 5;
    const int item = blockIdx.x * (SMALL_THREADS / 64) + (threadIdx.x >> 6);
    const int r = item / segs, seg = item - r * segs;
    if (r >= max_nb) return;                            // (the whole wave)
    const int a0 = dims[4 * f], b0 = dims[4 * f + 1];
    const int na = clampi(dims[4 * f + 2], 0, max_na), nb = clampi(dims[4 * f + 3], 0, max_nb);
    const int i = seg * 64 + lane;
    bool is_free = false;
    if (r < nb && i < na) {
        const double n = (double)cells_per_metre;
        const double x = (double)((long long)a0 + i) / n, y = (double)((long long)b0 + r) / n;
        int n_boxes;
        const double* __restrict__ boxes = table.find(f, n_boxes);
        bool hit = false;
        for (int k = 0; k < n_boxes && !hit; ++k) {
            const double* b = boxes + 4 * k;
            hit = __dsub_rn(b[0], margin) < x && x < __dadd_rn(b[2], margin) && __dsub_rn(b[1], margin) < y &&
                  y < __dadd_rn(b[3], margin);
        }
        if (objects) {
            const double* obj = objects + (size_t)f * MAX_OBJECTS * OBJ_REC;
            for (int k = 0; k < MAX_OBJECTS && !hit; ++k) {
                const double* b = obj + OBJ_REC * k;
                hit = b[6] != 0.0 && __dsub_rn(b[0], margin) < x && x < __dadd_rn(b[2], margin) &&
                      __dsub_rn(b[1], margin) < y && y < __dadd_rn(b[3], margin);
            }
        }
        const GridView g = grids.find(table, f);
        if (!hit && g.nx > 0) {
            int i0, i1, j0, j1;
            strict_run(g.xs, g.nx, margin, x, i0, i1);
            strict_run(g.ys, g.ny, margin, y, j0, j1);
            if (i0 < i1) {
                const int w0 = i0 >> 5, w1 = (i1 - 1) >> 5;
                for (int j = j0; j < j1 && !hit; ++j) {
                    const uint32_t* row = g.bits + (size_t)j * g.words;
                    for (int w = w0; w <= w1; ++w) {
                        unsigned mask = ~0u;
                        if (w == w0) mask &= ~0u << (i0 & 31);
                        if (w == w1) mask &= ~0u >> (31 - ((i1 - 1) & 31));
                        hit = hit || (row[w] & mask) != 0u;
                    }
                }
            }
        }
        is_free = !hit;
    }
    const unsigned long long verdicts = __ballot(is_free);
    if (lane == 0) {
        unsigned* row = out + ((size_t)f * max_nb + r) * words;
        row[2 * seg] = (unsigned)verdicts;
        if (2 * seg + 1 < words) row[2 * seg + 1] = (unsigned)(verdicts >> 32);
    }
}

// ---- fields -------------------------------------------------------------------------------------------------------------------
// knight moves (2s, t) out of the source row at c + S (S = -P: the row above, +P: below): two columns along the row
__device__ __forceinline__ unsigned knight_wide_into(const unsigned* C, const unsigned* F, int c, int S) {
    const unsigned cl = C[c + S - 1], cm = C[c + S], cr = C[c + S + 1];
    const unsigned gl = F[c + S - 1] & F[c - 1], gm = F[c + S] & F[c], gr = F[c + S + 1] & F[c + 1];
    const unsigned from_left = ((cm << 1) | (cl >> 31)) & gm, left_top = ((cl << 1) & gl) >> 31;
    const unsigned from_right = ((cm >> 1) | (cr << 31)) & gm, right_low = ((cr >> 1) & gr) & 1u;
    return (from_left << 1) | left_top | (from_right >> 1) | (right_low << 31);
}

// knight moves (s, 2t) out of the source row at c + 2S, through the row between at c + S
__device__ __forceinline__ unsigned knight_tall_into(const unsigned* C, const unsigned* F, int c, int S) {
    const unsigned l = C[c + 2 * S - 1] & F[c + S - 1], m = C[c + 2 * S] & F[c + S], r = C[c + 2 * S + 1] & F[c + S + 1];
    return ((m << 1) | (l >> 31) | (m >> 1) | (r << 31)) & F[c + S];
}

template <int WHERE>
__global__ __launch_bounds__(THREADS) void lattice_fields_kernel(
    const unsigned* __restrict__ free_bits, const int32_t* __restrict__ dims, int max_nb, int max_na,
    const int32_t* __restrict__ sources, const int32_t* __restrict__ source_counts, int max_sources, int max_cost,
    uint16_t* __restrict__ dist_all, unsigned* g_planes, size_t plane_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned smem[];
    int* b_lo = reinterpret_cast<int*>(smem);       // [16] first row of level d, slot d & 15 (NONE: empty)
    int* b_hi = b_lo + 16;                          // [16] last row (-1: empty)
    unsigned* mine = WHERE == ALL_LDS ? nullptr : g_planes + (size_t)blockIdx.x * (WHERE == RING_IN_SCRATCH ? RING : PLANES) * plane_cap;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int a0 = dims[4 * f], b0 = dims[4 * f + 1];
    const int na = clampi(dims[4 * f + 2], 0, max_na), nb = clampi(dims[4 * f + 3], 0, max_nb);
    if (na == 0 || nb == 0) return;                 // (uniform for the workgroup: before any barrier) no nodes, nothing to settle
    const int words = (max_na + 31) >> 5;           // the pitch of the caller's free planes
    const int W = (na + 31) >> 5, P = W + 2, R = nb + 4;
    unsigned* F = WHERE == ALL_IN_SCRATCH ? mine : smem + HEADER_WORDS;        // free
    unsigned* U = F + plane_cap;                                                // open: free and not yet settled
    unsigned* L0 = WHERE == ALL_LDS ? U + plane_cap : (WHERE == RING_IN_SCRATCH ? mine : mine + 2 * plane_cap);   // level ring
    uint16_t* dist = dist_all + (size_t)f * max_nb * max_na;

    for (int i = tid; i < P * R; i += THREADS) {
        F[i] = U[i] = 0u;
        for (int p = 0; p < RING; ++p) L0[p * plane_cap + i] = 0u;
    }
    if (tid < 16) { b_lo[tid] = NONE; b_hi[tid] = -1; }
    __syncthreads();
    // ---- free: the caller's words, without the bits beyond na (whatever the plane's tail holds)
    const unsigned* fb = free_bits + (size_t)f * max_nb * words;
    for (int i = tid; i < nb * W; i += THREADS) {
        const int r = i / W, k = i - r * W;
        unsigned v = fb[(size_t)r * words + k];
        if (k == W - 1 && (na & 31)) v &= ~0u >> (32 - (na & 31));
        F[(r + 2) * P + k + 1] = v;
        U[(r + 2) * P + k + 1] = v;
    }
    __syncthreads();
    // ---- level 0: the sources that are nodes of this lattice and free
    const int n_src = clampi(source_counts[f], 0, max_sources);
    const int32_t* src = sources + (size_t)f * max_sources * 2;
    for (int s = tid; s < n_src; s += THREADS) {
        const long long la = (long long)src[2 * s] - a0, lb = (long long)src[2 * s + 1] - b0;
        if (la < 0 || la >= na || lb < 0 || lb >= nb) continue;
        const int c = ((int)lb + 2) * P + ((int)la >> 5) + 1;
        const unsigned bit = 1u << ((int)la & 31);
        if (!(F[c] & bit)) continue;
        if (atomicOr(&L0[c], bit) & bit) continue;  // (the same node twice: the first lane settles it)
        atomicAnd(&U[c], ~bit);
        dist[(size_t)lb * max_na + la] = 0;
        atomicMin(&b_lo[0], (int)lb);
        atomicMax(&b_hi[0], (int)lb);
    }
    __syncthreads();

    // ---- levels (the order of a level: level_sets.h)
    int run = 0, sd = 0;                            // empty levels in a row; d % 12
    for (int d = 1; d <= max_cost; ++d) {
        sd = sd == RING - 1 ? 0 : sd + 1;
        run = b_hi[(d - 1) & 15] < 0 ? run + 1 : 0;
        if (run >= RING - 1) break;                 // levels d - 11 .. d - 1 are empty: so is every level from here on
        const int lo5 = b_lo[(d - 5) & 15], hi5 = b_hi[(d - 5) & 15];
        const int lo7 = b_lo[(d - 7) & 15], hi7 = b_hi[(d - 7) & 15];
        const int lo11 = b_lo[(d - 11) & 15], hi11 = b_hi[(d - 11) & 15];
        const int lo12 = b_lo[(d - 12) & 15], hi12 = b_hi[(d - 12) & 15];   // what the slot this level writes still holds
        const bool have = hi5 >= 0 || hi7 >= 0 || hi11 >= 0;
        int n0 = 1, n1 = 0;                                                 // rows this level can set
        if (have) {
            n0 = max(min(min(hi5 >= 0 ? lo5 : NONE, hi7 >= 0 ? lo7 : NONE), hi11 >= 0 ? lo11 : NONE) - 2, 0);
            n1 = min(max(max(hi5, hi7), hi11) + 2, nb - 1);
        }
        int s0 = n0, s1 = n1;                                               // rows to write: those, and the slot's stale ones
        if (hi12 >= 0) {
            s0 = have ? min(n0, lo12) : lo12;
            s1 = have ? max(n1, hi12) : hi12;
        }
        unsigned* Ld = L0 + (size_t)sd * plane_cap;
        const unsigned* A = L0 + (size_t)((sd + 7) % RING) * plane_cap;     // L[d-5]
        const unsigned* B = L0 + (size_t)((sd + 5) % RING) * plane_cap;     // L[d-7]
        const unsigned* C = L0 + (size_t)((sd + 1) % RING) * plane_cap;     // L[d-11]
        int my_lo = NONE, my_hi = -1;
        const int total = (s1 - s0 + 1) * W;
        for (int i = tid; i < total; i += THREADS) {
            const int q = i / W, r = s0 + q, k = i - q * W;
            const int c = (r + 2) * P + k + 1;
            unsigned out = 0u, u = 0u;
            if (r >= n0 && r <= n1 && (u = U[c]) != 0u) {
                if (hi5 >= 0) out = straight_into(A, c, P);
                if (hi7 >= 0) out |= diagonal_into(B, F, c, -P) | diagonal_into(B, F, c, P);
                if (hi11 >= 0)
                    out |= knight_wide_into(C, F, c, -P) | knight_wide_into(C, F, c, P) | knight_tall_into(C, F, c, -P) |
                           knight_tall_into(C, F, c, P);
                out &= u;
            }
            if (out != 0u || (r >= lo12 && r <= hi12)) Ld[c] = out;            // (rows beyond the stale band hold zeros)
            if (out) {
                U[c] = u & ~out;
                my_lo = min(my_lo, r);
                my_hi = max(my_hi, r);
                uint16_t* row = dist + (size_t)r * max_na + k * 32;
                for (unsigned m = out; m; m &= m - 1) row[__ffs(m) - 1] = (uint16_t)d;
            }
        }
        if (my_hi >= 0) {
            atomicMin(&b_lo[d & 15], my_lo);
            atomicMax(&b_hi[d & 15], my_hi);
        }
        if (tid == 0) { b_lo[(d + 1) & 15] = NONE; b_hi[(d + 1) & 15] = -1; }   // (level d - 15's: last read three levels ago)
        __syncthreads();
    }
}

// ---- query --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SMALL_THREADS) void lattice_query_kernel(
    const double* __restrict__ points, const int32_t* __restrict__ field_of, int m, int n_fields,
    const uint16_t* __restrict__ dist_all, const int32_t* __restrict__ dims, int max_nb, int max_na, int cells_per_metre,
    double* __restrict__ out) {
    const int p = blockIdx.x * SMALL_THREADS + threadIdx.x;
    if (p >= m) return;
    const int f = field_of[p];
    if (f < 0 || f >= n_fields) {
        out[p] = __builtin_nan("");
        return;
    }
    const double a0 = (double)dims[4 * f], b0 = (double)dims[4 * f + 1];
    const int na = clampi(dims[4 * f + 2], 0, max_na), nb = clampi(dims[4 * f + 3], 0, max_nb);
    const uint16_t* dist = dist_all + (size_t)f * max_nb * max_na;
    const double n = (double)cells_per_metre, unit = __dmul_rn(5.0, n);
    const double x = points[2 * p], y = points[2 * p + 1];
    const double fa = floor(__dmul_rn(x, n)), fb = floor(__dmul_rn(y, n));
    double best = __builtin_inf();
    for (int ua = 0; ua < 2; ++ua)
        for (int ub = 0; ub < 2; ++ub) {
            const double a = __dadd_rn(fa, (double)ua), b = __dadd_rn(fb, (double)ub);
            // (false for a NaN; inside, a - a0 is an exact small integer)
            if (!(a >= a0 && a <= __dadd_rn(a0, (double)(na - 1)) && b >= b0 && b <= __dadd_rn(b0, (double)(nb - 1)))) continue;
            const unsigned cost = dist[(size_t)(int)__dsub_rn(b, b0) * max_na + (int)__dsub_rn(a, a0)];
            if (cost == 0xFFFFu) continue;
            const double dx = __dsub_rn(x, a / n), dy = __dsub_rn(y, b / n);
            const double d = __dadd_rn(__dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy))), (double)cost / unit);
            best = fmin(best, d);
        }
    out[p] = best;
}

}  // namespace lattice
}  // namespace vlfm

using namespace vlfm;
using namespace vlfm::lattice;

static bool bad_bound(int n, int max_nb, int max_na) {
    return n < 0 || n > 65535 || max_nb < 1 || max_na < 1 || max_nb > MAX_NODES || max_na > MAX_NODES;
}
static bool bad_spacing(int cells_per_metre) { return cells_per_metre < 4 || cells_per_metre % 4 != 0; }

extern "C" int vlfm_lattice_free(const double* d_world_boxes, const int32_t* d_box_counts, int n_worlds, int max_boxes,
                                 const uint32_t* d_grid_bits, const double* d_grid_edges, const int32_t* d_grid_dims, int max_nx,
                                 int max_ny, const int32_t* d_world_of, double margin, const double* d_objects,
                                 const int32_t* d_dims, int n, int cells_per_metre, int max_nb, int max_na, uint32_t* d_free,
                                 void* stream) {
    const bool with_grids = d_grid_bits || d_grid_edges || d_grid_dims;
    if (bad_bound(n, max_nb, max_na) || bad_spacing(cells_per_metre) || n_worlds < 0 || max_boxes < 0 || max_boxes > 16384 ||
        !(margin == margin) || (n_worlds > 0 && (!d_box_counts || (max_boxes > 0 && !d_world_boxes))) ||
        (with_grids && (!d_grid_bits || !d_grid_edges || !d_grid_dims || max_nx < 1 || max_ny < 1 ||
                        max_nx > VLFM_GRID_MAX_CELLS || max_ny > VLFM_GRID_MAX_CELLS)) ||
        (n > 0 && (!d_world_of || !d_dims || !d_free)))
        return fail(VLFM_ERR_INVALID, "lattice_free: bad argument (1 <= max_nb, max_na <= 1024; cells_per_metre a multiple of 4)");
    if (n == 0) return VLFM_OK;
    hipStream_t st = (hipStream_t)stream;
    const int items = max_nb * ((max_na + 63) >> 6), per_block = SMALL_THREADS / 64;
    VLFM_TIMED("lattice_free_kernel", st);
    VLFM_KLAUNCH(lattice_free_kernel, dim3((items + per_block - 1) / per_block, n), dim3(SMALL_THREADS), 0, st,
                 WorldBoxes{d_world_boxes, d_box_counts, d_world_of, n_worlds, max_boxes},
                 WorldGrids{d_grid_bits, d_grid_edges, d_grid_dims, with_grids ? max_nx : 0, with_grids ? max_ny : 0}, margin,
                 d_objects, d_dims, cells_per_metre, max_nb, max_na, d_free);
    return check_launch("lattice_free_kernel");
}

extern "C" size_t vlfm_lattice_scratch_bytes(int n, int max_nb, int max_na) {
    if (n <= 0 || bad_bound(n, max_nb, max_na)) return 0;
    return (size_t)n * scratch_planes(residence_of(max_nb, max_na)) * plane_words(max_nb, max_na) * sizeof(unsigned);
}

extern "C" int vlfm_lattice_fields(const uint32_t* d_free, const int32_t* d_dims, int n, int max_nb, int max_na,
                                   const int32_t* d_sources, const int32_t* d_source_counts, int max_sources, int max_cost,
                                   uint16_t* d_dist, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (bad_bound(n, max_nb, max_na) || max_sources < 0 || max_cost < 0 || max_cost > 65534 ||
        (n > 0 && (!d_free || !d_dims || !d_source_counts || !d_dist)) || (n > 0 && max_sources > 0 && !d_sources))
        return fail(VLFM_ERR_INVALID, "lattice_fields: bad argument (1 <= max_nb, max_na <= 1024; max_cost <= 65534)");
    if (n == 0) return VLFM_OK;
    const size_t need = vlfm_lattice_scratch_bytes(n, max_nb, max_na);
    if (need > 0 && (!d_scratch || scratch_bytes < need))
        return fail(VLFM_ERR_CAPACITY, "lattice_fields: scratch smaller than vlfm_lattice_scratch_bytes(n, max_nb, max_na)");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_dist, 0xFF, (size_t)n * max_nb * max_na * sizeof(uint16_t), st) != hipSuccess)
        return fail(VLFM_ERR_HIP, "lattice_fields: cannot preset the dist planes");
    const size_t cap = plane_words(max_nb, max_na);
    const Residence where = residence_of(max_nb, max_na);
    const size_t lds = lds_bytes(PLANES - scratch_planes(where), max_nb, max_na);
    unsigned* g_planes = reinterpret_cast<unsigned*>(d_scratch);
    VLFM_TIMED("lattice_fields_kernel", st);
#define VLFM_LATTICE_LAUNCH(WHERE)                                                                                            \
    do {                                                                                                                      \
        static LdsOptIn opt;                                                                                                  \
        if (lds > 64 * 1024 && !opt.ensure(reinterpret_cast<const void*>(lattice_fields_kernel<WHERE>), lds))                 \
            return fail(VLFM_ERR_HIP, "lattice_fields: cannot opt in to the LDS size");                                       \
        VLFM_KLAUNCH(lattice_fields_kernel<WHERE>, dim3(n), dim3(THREADS), lds, st, d_free, d_dims, max_nb, max_na, d_sources, \
                     d_source_counts, max_sources, max_cost, d_dist, g_planes, cap);                                          \
    } while (0)
    if (where == ALL_LDS) VLFM_LATTICE_LAUNCH(ALL_LDS);
    else if (where == RING_IN_SCRATCH) VLFM_LATTICE_LAUNCH(RING_IN_SCRATCH);
    else VLFM_LATTICE_LAUNCH(ALL_IN_SCRATCH);
#undef VLFM_LATTICE_LAUNCH
    const int rc = check_launch("lattice_fields_kernel");
    return rc == VLFM_OK ? (int)where : rc;
}

extern "C" int vlfm_lattice_query(const double* d_points, const int32_t* d_field_of, int m, int n_fields, const uint16_t* d_dist,
                                  const int32_t* d_dims, int max_nb, int max_na, int cells_per_metre, double* d_out,
                                  void* stream) {
    if (m < 0 || n_fields < 0 || bad_bound(0, max_nb, max_na) || bad_spacing(cells_per_metre) ||
        (m > 0 && (!d_points || !d_field_of || !d_out)) || (m > 0 && n_fields > 0 && (!d_dist || !d_dims)))
        return fail(VLFM_ERR_INVALID, "lattice_query: bad argument (1 <= max_nb, max_na <= 1024; cells_per_metre a multiple of 4)");
    if (m == 0) return VLFM_OK;
    hipStream_t st = (hipStream_t)stream;
    VLFM_TIMED("lattice_query_kernel", st);
    VLFM_KLAUNCH(lattice_query_kernel, dim3((m + SMALL_THREADS - 1) / SMALL_THREADS), dim3(SMALL_THREADS), 0, st, d_points,
                 d_field_of, m, n_fields, d_dist, d_dims, max_nb, max_na, cells_per_metre, d_out);
    return check_launch("lattice_query_kernel");
}
