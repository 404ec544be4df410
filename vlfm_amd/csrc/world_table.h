// world_table.h -- where a workgroup finds the wall boxes of ITS camera (world_render.hip) or field (geodesic.hip): a table of
// worlds [n_worlds][max_boxes][4] with a count per world and, per camera or field, the world it stands in.  The fixed rooms
// world is a table of one row.  A world outside [0, n_worlds) is EMPTY and is never dereferenced; a count is clamped to
// [0, max_boxes]; rows beyond a world's count are never read.
// `capacity()` is what a kernel's LDS layout and output strides reserve for the boxes -- the same for every workgroup of a
// launch --, `find(i, count)` the boxes of camera / field i and how many of them there are.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace vlfm {

struct WorldBoxes {
    const double* boxes;
    const int32_t* counts;
    const int32_t* world_of;
    int n_worlds, max_boxes;
    __device__ __forceinline__ int capacity() const { return max_boxes; }
    __device__ __forceinline__ const double* find(int i, int& count) const {
        const int w = world_of[i];
        const bool known = w >= 0 && w < n_worlds;
        const int c = known ? counts[w] : 0;
        count = c < 0 ? 0 : (c > max_boxes ? max_boxes : c);
        return boxes + (known ? (size_t)w * (size_t)max_boxes * 4 : 0);
    }
};

// The occupancy grids of the same table (world_render.hip only): per world bit-packed rows [max_ny][words] (bit i % 32 of word
// i / 32 of row j: cell (i, j) is a wall), the edges xs [max_nx + 1] then ys [max_ny + 1], and dims (ny, nx), clamped to
// [0, max_ny] x [0, max_nx]; a world whose clamped dims hold a zero, or that lies outside the table, has NO grid (nx = ny = 0
// in the view, nothing of it is ever read).  Cells beyond a world's dims are never read, whatever the table holds there.
struct GridView {
    const uint32_t* bits;
    const double *xs, *ys;
    int nx, ny, words;
};

struct WorldGrids {
    const uint32_t* bits;
    const double* edges;
    const int32_t* dims;
    int max_nx, max_ny;
    __device__ __forceinline__ int words() const { return (max_nx + 31) >> 5; }
    __device__ __forceinline__ GridView find(const WorldBoxes& table, int i) const {
        const int w = table.world_of[i];
        const bool known = bits != nullptr && w >= 0 && w < table.n_worlds;
        int ny = known ? dims[2 * w] : 0, nx = known ? dims[2 * w + 1] : 0;
        ny = ny < 0 ? 0 : (ny > max_ny ? max_ny : ny);
        nx = nx < 0 ? 0 : (nx > max_nx ? max_nx : nx);
        if (nx == 0 || ny == 0) nx = ny = 0;
        const size_t row = known ? (size_t)w : 0;
        const double* e = edges + row * (size_t)(max_nx + max_ny + 2);
        return GridView{bits + row * (size_t)max_ny * words(), e, e + max_nx + 1, nx, ny, words()};
    }
};

}  // namespace vlfm
