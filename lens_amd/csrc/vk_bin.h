// Bin-site arithmetic shared by vk_bin_sites (vk_lattice.hip) and the motility
// kernel (vk_motility.hip), so the bins a moved agent lands in are the ones
// vk_bin_sites would give its new location.
#pragma once

#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

// get_bin_site: floor(loc * n / bound) as int, then Python/numpy floor-mod n.
__device__ __forceinline__ int bin_axis(double loc, int n, double bound) {
    const double v = floor(loc * n / bound);
    if (!(fabs(v) < 9.0e15)) return 0;
    int64_t i = (int64_t)v % n;
    if (i < 0) i += n;
    return (int)i;
}

// local linear bin (ix - row_offset) * ny + iy of a location; *ix_out = ix
__device__ __forceinline__ int32_t bin_site_lin(double x, double y, int nx, int ny, double bx, double by,
                                                int row_offset, int *ix_out) {
    const int ix = bin_axis(x, nx, bx);
    const int iy = bin_axis(y, ny, by);
    *ix_out = ix;
    return (ix - row_offset) * ny + iy;
}
