// level_sets.h -- Dial's level sets over bit-packed rows, one 1024-thread workgroup per field: what map_planner.hip
// (8 moves, costs 2 / 3) and lattice_geodesic.hip (16 moves, costs 5 / 7 / 11) share.  With integer costs the field is a sequence
// of level sets,
//     L[d] = (OR over the costs k of  moves_k(L[d - k]))  &  free  &  not yet settled,
// and on bit-packed rows a move is word shifts with carries from the neighbouring words, ANDs and ORs (straight_into,
// diagonal_into below; the lattice adds its knight moves).  Each kernel keeps its own level loop; what differs between them:
//     RING     level planes (4 / 12): level d writes slot d % RING while it reads the slots of d - k; RING > every cost, so the
//              slot it overwrites (level d - RING's) is no source of this or any later level
//     BANDS    slots of the band ring (8 / 16), a power of two > RING + 1
//     REACH    the rows a move spans (1 / 2): the zero rows above and below every plane and the widening of a sweep
// Planes: `free`, `open` (free and not yet settled) and the ring, each of `rows` x W words with one zero word left and right of
// every row (pitch P = W + 2) and REACH zero rows above and below: nothing tests a bound.  Row r, word k is (r + REACH) * P + k + 1.
// The kernels choose where the planes live (LDS or a global scratch); the primitives take plain pointers and are inlined, so the
// address space is still the compiler's to see.
//
// Bands and the order of a level -- why one barrier per level is enough.
//   Every level records the first and last row it set in b_lo / b_hi[d & (BANDS - 1)] (LDS atomics); an empty level leaves
//   NONE / -1 (the loops test hi >= 0).  Level d can set only rows within REACH of a source level's band (n0 .. n1).
//   It must also leave slot d % RING holding exactly L[d]: the slot still holds L[d - RING] in the rows of that level's band, so
//   those rows are swept too (s0 .. s1) and get their zeros; every other row of the slot holds zeros already, by induction from
//   the cleared planes, which is why the lattice stores a zero word only inside the stale band (the planner stores every word it
//   sweeps; both are right).  An empty level's plane is all zeros for the same reason, so the lattice does not read a source level
//   with an empty band.
//   Everything level d reads at its top -- the bands of d - 1, of its source levels and of d - RING, and the source
//   planes -- was written before the barrier that ended level d - 1.  Inside the level a word of `open` and of the written slot
//   is touched by the one lane that sweeps it; the source planes and `free` are only read.  The band slot of d takes the atomics;
//   it was reset during level d - 1.  Lane 0 resets slot d + 1, which held level d + 1 - BANDS: older than d - RING, so no lane
//   still at the top of level d reads it.  Hence nothing written in level d is read in level d, and the one barrier at its end
//   orders it against level d + 1.
//   Running dry: RING - 1 empty levels in a row -- every source level of every later level is among them (the lattice counts
//   them; the planner tests its three).  dist: each cell is stored once, by the level that settles it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vlfm {
namespace levels {

constexpr int THREADS = 1024;           // 16 waves, the one workgroup a CU gets
constexpr int HEADER_WORDS = 32;        // LDS in front of the planes: the band ring (lo[BANDS], hi[BANDS]) and the kernel's own words
constexpr size_t LDS_BYTES_MAX = 160 * 1024;
constexpr int NONE = 0x7FFFFFFF;

// ---- what the moves of one cost reach in the target word c (pitch P), before `& open`
__device__ __forceinline__ unsigned straight_into(const unsigned* A, int c, int P) {
    const unsigned a = A[c];
    return A[c - P] | A[c + P] | (a << 1) | (A[c - 1] >> 31) | (a >> 1) | (A[c + 1] << 31);
}

// diagonals out of the source row at c + S (S = -P: the row above, +P: below), F the free plane.  Target (x, y), source
// (x - dx, y - dy): the source AND the side cell (x - dx, y) are one AND of the source's row of B with the target's row of `free`
// BEFORE the shift; the side cell (x, y - dy) is one AND with the source's row of `free` after it.  Shift-with-carry distributes
// over AND, so that is two ANDs per row.
__device__ __forceinline__ unsigned diagonal_into(const unsigned* B, const unsigned* F, int c, int S) {
    const unsigned l = B[c + S - 1] & F[c - 1], m = B[c + S] & F[c], r = B[c + S + 1] & F[c + 1];
    return ((m << 1) | (l >> 31) | (m >> 1) | (r << 31)) & F[c + S];
}

}  // namespace levels
}  // namespace vlfm
