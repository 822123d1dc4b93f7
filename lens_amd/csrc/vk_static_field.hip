// Analytic gradients on MI355X (gfx950): make_gradient on the device (vk_gradient_fill) and
// the StaticField deriver (vk_static_gather).  Both evaluate gradient_value (vk_gradient.h),
// the one statement of the reference's arithmetic; the motile kernels' static variants
// (vk_motility.hip, vk_flagella.hip) sense through the same function.
//
// Specs are few (<= VK_GRADIENT_MAX) and wave-uniform, so they travel by value in the kernel
// arguments: no device table to allocate, nothing a captured graph has to keep alive.
// Both kernels are streaming: one thread per cell / per agent, stores coalesced along the
// fastest axis (iy of a plane, the agent column of conc).

#include "vk_gradient.h"

struct gradient_specs {
    vk_gradient_spec g[VK_GRADIENT_MAX];
};

struct gather_map {
    vk_gradient_spec g[VK_GRADIENT_MAX];   // the spec of map entry j (already looked up)
    int32_t row[VK_GRADIENT_MAX];
};

// grid: (ceil(ny / 256), nx, n_specs); threadIdx.x runs along iy
__global__ __launch_bounds__(256) void k_gradient_fill(gradient_specs s, double *__restrict__ planes,
                                                       int64_t plane_stride, int64_t row_stride, int nx, int ny,
                                                       double bx, double by) {
    const int iy = blockIdx.x * blockDim.x + threadIdx.x;
    const int ix = blockIdx.y;
    const int f = blockIdx.z;
    if (iy >= ny) return;
    // the middle of the bin, parenthesised as the reference writes it
    const double x = (((double)ix + 0.5) * bx) / (double)nx;
    const double y = (((double)iy + 0.5) * by) / (double)ny;
    planes[(int64_t)f * plane_stride + (int64_t)ix * row_stride + iy] = gradient_value(s.g[f], x, y);
}

__global__ __launch_bounds__(256) void k_static_gather(gather_map m, int n_map, const double *__restrict__ loc,
                                                       int64_t ld, int64_t n, double *__restrict__ conc,
                                                       int64_t ld_conc) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const double x = loc[a], y = loc[ld + a];
    for (int j = 0; j < n_map; ++j) conc[(int64_t)m.row[j] * ld_conc + a] = gradient_value(m.g[j], x, y);
}

extern "C" int vk_gradient_fill(const vk_gradient_spec *specs, int32_t n_specs, double *planes, int64_t plane_stride,
                                int64_t row_stride, int32_t nx, int32_t ny, double bound_x, double bound_y,
                                vk_stream_t stream) {
    if (n_specs < 0 || n_specs > VK_GRADIENT_MAX || nx <= 0 || ny <= 0 || nx > 65535 || row_stride < ny ||
        !(bound_x > 0.0) || !(bound_y > 0.0) || (n_specs > 0 && (!specs || !planes)) ||
        (n_specs > 1 && plane_stride < (int64_t)(nx - 1) * row_stride + ny)) {
        vk::set_error("vk_gradient_fill: bad arguments");
        return VK_ERR_ARG;
    }
    gradient_specs s = {};
    for (int f = 0; f < n_specs; ++f) {
        if (!gradient_spec_ok(specs[f])) {
            vk::set_error("vk_gradient_fill: spec %d: unknown type, zero deviation or non-positive base", f);
            return VK_ERR_ARG;
        }
        s.g[f] = specs[f];
    }
    if (n_specs == 0) return VK_OK;
    hipLaunchKernelGGL(k_gradient_fill, dim3((unsigned)((ny + 255) / 256), (unsigned)nx, (unsigned)n_specs), dim3(256),
                       0, (hipStream_t)stream, s, planes, plane_stride, row_stride, nx, ny, bound_x, bound_y);
    return vk::launch_check("k_gradient_fill");
}

extern "C" int vk_static_gather(const vk_gradient_spec *specs, const int32_t *field_of, const int32_t *row_of,
                                int32_t n_map, const double *loc, int64_t ld, int64_t n, double *conc,
                                int64_t ld_conc, vk_stream_t stream) {
    if (n_map < 0 || n_map > VK_GRADIENT_MAX || n < 0 || ld < n || ld_conc < n ||
        (n_map > 0 && (!specs || !field_of || !row_of)) || (n > 0 && n_map > 0 && (!loc || !conc))) {
        vk::set_error("vk_static_gather: bad arguments");
        return VK_ERR_ARG;
    }
    gather_map m = {};
    for (int j = 0; j < n_map; ++j) {
        if (field_of[j] < 0 || field_of[j] >= VK_GRADIENT_MAX || row_of[j] < 0 || !gradient_spec_ok(specs[field_of[j]])) {
            vk::set_error("vk_static_gather: map entry %d: bad field, row or spec", j);
            return VK_ERR_ARG;
        }
        m.g[j] = specs[field_of[j]];
        m.row[j] = row_of[j];
    }
    if (n == 0 || n_map == 0) return VK_OK;
    hipLaunchKernelGGL(k_static_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, n_map,
                       loc, ld, n, conc, ld_conc);
    return vk::launch_check("k_static_gather");
}
