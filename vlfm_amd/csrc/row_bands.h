// row_bands.h -- the launch geometry of the per-frame image kernels (world_render.hip, depth_sensor.hip): a grid of
// (row bands, frames), one workgroup per band.  Host only.
#pragma once
#include "status.h"

namespace vlfm {

constexpr int MIN_BAND_ROWS = 4;

struct Bands {
    int band, grid_x;                         // rows per workgroup, workgroups per frame
};

// row bands: enough workgroups for four per compute unit, never fewer than MIN_BAND_ROWS rows each and never more than `max_rows`
inline Bands plan_bands(int n, int H, int max_rows) {
    const long long want = 4LL * device_cu_count();
    long long bands = (want + n - 1) / n;
    const long long most = (H + MIN_BAND_ROWS - 1) / MIN_BAND_ROWS, least = ((long long)H + max_rows - 1) / max_rows;
    bands = bands < least ? least : (bands > most ? most : bands);
    const int band = (int)((H + bands - 1) / bands);
    return Bands{band, (H + band - 1) / band};
}

}  // namespace vlfm
