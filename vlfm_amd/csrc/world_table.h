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

}  // namespace vlfm
