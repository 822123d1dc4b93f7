// Cell growth, derivers and division on MI355X (gfx950).
//
// Reference semantics (all per agent, per 1-s step):
//   GrowthProtein.next_update   vivarium/processes/growth_protein.py:88-107
//   Growth.next_update          vivarium/processes/growth.py:101-107
//   DivisionVolume.next_update  vivarium/processes/division_volume.py:39-45
//   TreeMass (calculate_mass)   vivarium/processes/tree_mass.py:10-18
//   DeriveGlobals.next_update   vivarium/processes/derive_globals.py:131-152 (+ :20-50)
//   MetaDivision / _divide      vivarium/processes/meta_division.py:15-88,
//                               vivarium/core/experiment.py:664-697
//   dividers                    vivarium/core/registry.py:197-280
// Compiled with -ffp-contract=off and written in the reference's operation
// order, so every float result is bit-identical to the reference's Python
// (the host evaluates exp(), pow() and the units' conversion factors with the
// same libraries the reference used and passes them in vk_cell_params).
//
// Division is a stable compaction: survivors keep their relative order and
// the two daughters of each mother are appended in mother order -- the agent
// order the reference's Store ends up with (daughters generated at the end of
// the agents dict, mother deleted).  The plan is one exclusive scan of the
// divide flags (block counts -> one-block scan -> per-block ranks); every SoA
// array is then gathered once into the new layout with its divider.
// vk_population_plan is the same plan with removal (the mother machine's outflow,
// multibody_physics.py:232-250 `_delete`; Colony.remove): a removed agent gets no slot.

#include <stdint.h>

#include "vk_internal.h"
#include "vk_philox.h"   // philox_uniform: counter = (step, root, path), key = (seed + depth)

// ---------------------------------------------------------------------------
// growth process + derivers
// ---------------------------------------------------------------------------

// The deriver tail of both cell kernels: the mass row, then globals_deriver on it
// (derive_globals.py:131-152): volume = mass / density (magnitude), then .to('fL');
// mmol_to_counts, length and surface area from the same magnitude.
__device__ __forceinline__ void cell_derive(const vk_cell_params &p, double m, int64_t a, int64_t ld,
                                            double *__restrict__ cell, double *__restrict__ m2c) {
    cell[(int64_t)VK_CELL_MASS * ld + a] = m;
    const double raw = m / p.density;
    cell[(int64_t)VK_CELL_VOLUME * ld + a] = raw * p.volume_to_fl;
    m2c[a] = p.avogadro * (raw * 1e-15) * 1e-3;
    const double len = (raw - p.cap_volume) / p.cap_area + p.two_r;
    cell[(int64_t)VK_CELL_LENGTH * ld + a] = len;
    cell[(int64_t)VK_CELL_SURFACE_AREA * ld + a] = p.sa_const + p.sa_lin * (len - p.width);
}

// GrowthProtein.next_update from the step-start protein (growth_protein.py:88-107): writes the
// new protein, returns it; div: the step-start protein reached divide_protein
__device__ __forceinline__ double cell_grow_protein(const vk_cell_params &p, int64_t a, double *__restrict__ protein,
                                                    const double *__restrict__ u, const int32_t *__restrict__ root,
                                                    const int32_t *__restrict__ depth,
                                                    const uint64_t *__restrict__ path, int32_t &div) {
    const double pr = *protein;
    const double total = pr * p.factor;
    double added = trunc(total - pr);            // int(total - protein)
    const double extra = total - trunc(total);   // total - int(total)
    const double draw = (p.rng == VK_RNG_PHILOX)
                            ? philox_uniform(p.seed, p.step, root[a], depth[a], path[a])
                            : u[a];
    if (draw < extra) added = added + 1.0;
    div = pr >= p.divide_protein;
    const double pn = pr + added;
    *protein = pn;
    return pn;
}

__global__ __launch_bounds__(256) void k_cell_step(vk_cell_params p, int64_t n, int64_t ld, double *__restrict__ cell,
                                                   double *__restrict__ m2c, const double *__restrict__ u,
                                                   const int32_t *__restrict__ root, const int32_t *__restrict__ depth,
                                                   const uint64_t *__restrict__ path, int32_t *__restrict__ divide) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const double *mass = cell + (int64_t)VK_CELL_MASS * ld + a;
    const double *volume = cell + (int64_t)VK_CELL_VOLUME * ld + a;
    int32_t div;
    double m;
    if (p.model == VK_GROWTH_PROTEIN) {
        const double pn = cell_grow_protein(p, a, cell + (int64_t)VK_CELL_PROTEIN * ld + a, u, root, depth, path, div);
        // mass_deriver: 0 fg + mw * (count / N_A), g -> fg
        m = 0.0 + (p.protein_mw * (pn / p.avogadro)) * p.fg_per_g;
    } else {
        div = *volume >= p.division_volume;          // DivisionVolume, step-start volume
        m = *mass * p.factor;                         // Growth
    }
    cell_derive(p, m, a, ld, cell, m2c);
    divide[a] = div;
}

extern "C" int vk_cell_step(const vk_cell_params *p, int64_t n, int64_t ld, double *cell, double *m2c,
                            const double *u, const int32_t *root, const int32_t *depth, const uint64_t *path,
                            int32_t *divide, vk_stream_t stream) {
    if (!p || n < 0 || ld < n || (n > 0 && (!cell || !m2c || !divide))) {
        vk::set_error("vk_cell_step: bad arguments");
        return VK_ERR_ARG;
    }
    if (p->model != VK_GROWTH_PROTEIN && p->model != VK_GROWTH_MASS) {
        vk::set_error("vk_cell_step: unknown growth model %d", p->model);
        return VK_ERR_ARG;
    }
    if (p->model == VK_GROWTH_PROTEIN && n > 0) {
        if (p->rng == VK_RNG_STREAM && !u) {
            vk::set_error("vk_cell_step: VK_RNG_STREAM needs u[]");
            return VK_ERR_ARG;
        }
        if (p->rng == VK_RNG_PHILOX && (!root || !depth || !path)) {
            vk::set_error("vk_cell_step: VK_RNG_PHILOX needs the lineage arrays");
            return VK_ERR_ARG;
        }
        if (p->rng != VK_RNG_STREAM && p->rng != VK_RNG_PHILOX) {
            vk::set_error("vk_cell_step: unknown rng %d", p->rng);
            return VK_ERR_ARG;
        }
    }
    if (n == 0) return VK_OK;
    hipLaunchKernelGGL(k_cell_step, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *p, n,
                       ld, cell, m2c, u, root, depth, path, divide);
    return vk::launch_check("k_cell_step");
}

// ---------------------------------------------------------------------------
// TreeMass over the colony's count table (tree_mass.py:10-18, 55-64)
// ---------------------------------------------------------------------------
//
// k_cell_step_tree is k_cell_step with the mass folded over weighted rows of the int32 count
// table: m = m + (mw * (count / N_A)) * fg_per_g per weighted row, rows ascending, after the
// aggregate protein (VK_GROWTH_PROTEIN) or from initial_mass[a] (VK_GROWTH_TREE).  The per-node
// expression is calculate_mass with pint's g -> fg factor; the ORDER of the fold is THE ENGINE'S
// OWN (the reference folds in its Store's depth-first dict order; include/vk_kinetics.h).
//
// Layout.  One agent per lane.  rows[] and weights[] are the same for every lane: wave-uniform
// addresses (ldc: the scalar cache).  A count is row * ld_counts + a: a wave's loads coalesce.
// The rows go in chunks of TREE_CHUNK whose loads are all issued before the chunk's arithmetic,
// so a lane has TREE_CHUNK loads in flight, not one dependent load after another.  The division
// by avogadro stays a division (a reciprocal multiply changes bits).  No LDS, no atomics.
// A row outside [0, n_rows) reads nothing and counts 0: the host side validates rows[]
// (lens_amd.cells.TreeWeights), the guard only keeps an unvalidated caller inside the table.

#define TREE_CHUNK 16

__global__ __launch_bounds__(256) void k_cell_step_tree(
    vk_cell_params p, int64_t n, int64_t ld, double *__restrict__ cell, double *__restrict__ m2c,
    const double *__restrict__ u, const int32_t *__restrict__ root, const int32_t *__restrict__ depth,
    const uint64_t *__restrict__ path, int32_t *__restrict__ divide, const int32_t *__restrict__ counts,
    int64_t ld_counts, int32_t n_rows, const int32_t *__restrict__ rows, const double *__restrict__ weights,
    int32_t n_weighted, const double *__restrict__ initial_mass) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    int32_t div;
    double m;
    if (p.model == VK_GROWTH_PROTEIN) {
        const double pn = cell_grow_protein(p, a, cell + (int64_t)VK_CELL_PROTEIN * ld + a, u, root, depth, path, div);
        m = 0.0 + (p.protein_mw * (pn / p.avogadro)) * p.fg_per_g;
    } else {
        div = cell[(int64_t)VK_CELL_VOLUME * ld + a] >= p.division_volume;   // DivisionVolume, step-start volume
        m = initial_mass[a];
    }
    for (int k0 = 0; k0 < n_weighted; k0 += TREE_CHUNK) {
        int32_t x[TREE_CHUNK];
#pragma unroll
        for (int i = 0; i < TREE_CHUNK; ++i) {
            x[i] = 0;
            if (k0 + i < n_weighted) {
                const int row = ldc(rows, k0 + i);
                if ((unsigned)row < (unsigned)n_rows) x[i] = counts[(int64_t)row * ld_counts + a];
            }
        }
#pragma unroll
        for (int i = 0; i < TREE_CHUNK; ++i)
            if (k0 + i < n_weighted) m = m + (ldc(weights, k0 + i) * ((double)x[i] / p.avogadro)) * p.fg_per_g;
    }
    cell_derive(p, m, a, ld, cell, m2c);
    divide[a] = div;
}

extern "C" int vk_cell_step_tree(const vk_cell_params *p, int64_t n, int64_t ld, double *cell, double *m2c,
                                 const double *u, const int32_t *root, const int32_t *depth, const uint64_t *path,
                                 int32_t *divide, const int32_t *counts, int64_t ld_counts, int32_t n_rows,
                                 const int32_t *rows, const double *weights, int32_t n_weighted,
                                 const double *initial_mass, vk_stream_t stream) {
    if (!p || n < 0 || ld < n || ld_counts < n || n_rows < 0 || n_weighted < 0 || n_weighted > VK_TREE_MAX_WEIGHTED ||
        n_weighted > n_rows || (n > 0 && (!cell || !m2c || !divide)) ||
        (n > 0 && n_weighted > 0 && (!counts || !rows || !weights))) {
        vk::set_error("vk_cell_step_tree: bad arguments (n <= ld, n <= ld_counts, 0 <= n_weighted <= %d and <= n_rows)",
                      VK_TREE_MAX_WEIGHTED);
        return VK_ERR_ARG;
    }
    if (p->model == VK_GROWTH_MASS) {
        vk::set_error("vk_cell_step_tree: VK_GROWTH_MASS writes the mass itself (vk_cell_step)");
        return VK_ERR_ARG;
    }
    if (p->model != VK_GROWTH_PROTEIN && p->model != VK_GROWTH_TREE) {
        vk::set_error("vk_cell_step_tree: unknown growth model %d", p->model);
        return VK_ERR_ARG;
    }
    if (p->model == VK_GROWTH_TREE && n > 0 && !initial_mass) {
        vk::set_error("vk_cell_step_tree: VK_GROWTH_TREE needs initial_mass[]");
        return VK_ERR_ARG;
    }
    if (p->model == VK_GROWTH_PROTEIN && n > 0) {
        if (p->rng == VK_RNG_STREAM && !u) {
            vk::set_error("vk_cell_step_tree: VK_RNG_STREAM needs u[]");
            return VK_ERR_ARG;
        }
        if (p->rng == VK_RNG_PHILOX && (!root || !depth || !path)) {
            vk::set_error("vk_cell_step_tree: VK_RNG_PHILOX needs the lineage arrays");
            return VK_ERR_ARG;
        }
        if (p->rng != VK_RNG_STREAM && p->rng != VK_RNG_PHILOX) {
            vk::set_error("vk_cell_step_tree: unknown rng %d", p->rng);
            return VK_ERR_ARG;
        }
    }
    if (n == 0) return VK_OK;
    hipLaunchKernelGGL(k_cell_step_tree, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *p, n,
                       ld, cell, m2c, u, root, depth, path, divide, counts, ld_counts, n_rows, rows, weights,
                       n_weighted, initial_mass);
    return vk::launch_check("k_cell_step_tree");
}

// ---------------------------------------------------------------------------
// division plan: exclusive scan of the divide flags
// ---------------------------------------------------------------------------

constexpr int DV_BLOCK = 1024;   // agents per scan block (256 threads x 4)

int64_t vk_divide_scratch_bytes_impl(int64_t n) {
    const int64_t nb = (n + DV_BLOCK - 1) / DV_BLOCK;
    return (nb + 2) * (int64_t)sizeof(int64_t);
}

extern "C" int64_t vk_divide_scratch_bytes(int64_t n) { return n < 0 ? 0 : vk_divide_scratch_bytes_impl(n); }

__global__ __launch_bounds__(256) void k_divide_count(const int32_t *__restrict__ divide, int64_t n,
                                                      int64_t *__restrict__ block_count) {
    const int64_t base = (int64_t)blockIdx.x * DV_BLOCK;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t a = base + k * 256 + threadIdx.x;
        if (a < n && divide[a]) ++c;
    }
    __shared__ int part[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// one block: exclusive scan of nb block counts in place; total -> *total, n + total -> *n_out
__global__ __launch_bounds__(256) void k_divide_scan_blocks(int64_t *__restrict__ block_count, int64_t nb,
                                                            int64_t n, int64_t *__restrict__ n_out) {
    __shared__ int64_t carry;
    __shared__ int64_t wsum[4];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nb; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        const int64_t v = b < nb ? block_count[b] : 0;
        // inclusive wave scan
        int64_t x = v;
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[threadIdx.x >> 6] = x;
        __syncthreads();
        int64_t wo = 0;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) wo += wsum[w];
        const int64_t excl = carry + wo + x - v;
        __syncthreads();
        if (b < nb) block_count[b] = excl;
        if (threadIdx.x == 255) carry = excl + v;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        block_count[nb] = carry;   // total number of mothers
        *n_out = n + carry;
    }
}

__global__ __launch_bounds__(256) void k_divide_place(const int32_t *__restrict__ divide, int64_t n,
                                                      const int64_t *__restrict__ block_off, int64_t nb,
                                                      int32_t *__restrict__ src_index, int32_t *__restrict__ kind) {
    const int64_t base = (int64_t)blockIdx.x * DV_BLOCK;
    const int64_t total = block_off[nb];
    const int64_t n_keep = n - total;
    __shared__ int wcount[16];
    // per-thread 4 consecutive agents -> thread-level counts -> block exclusive scan
    const int64_t a0 = base + (int64_t)threadIdx.x * 4;
    int f[4], c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[k] = (a0 + k < n) ? (divide[a0 + k] != 0) : 0;
        c += f[k];
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) wcount[w] = x;
    __syncthreads();
    int wo = 0;
    for (int k = 0; k < w; ++k) wo += wcount[k];
    int64_t m = block_off[blockIdx.x] + wo + x - c;   // mothers before a0
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t a = a0 + k;
        if (a >= n) break;
        if (f[k]) {
            const int64_t j = n_keep + 2 * m;
            src_index[j] = (int32_t)a;
            kind[j] = 0;
            src_index[j + 1] = (int32_t)a;
            kind[j + 1] = 1;
            ++m;
        } else {
            const int64_t j = a - m;
            src_index[j] = (int32_t)a;
            kind[j] = -1;
        }
    }
}

extern "C" int vk_divide_plan(const int32_t *divide, int64_t n, int32_t *src_index, int32_t *kind, int64_t *n_out,
                              void *scratch, vk_stream_t stream) {
    if (n < 0 || n > 0x3fffffff || !n_out || !scratch || (n > 0 && (!divide || !src_index || !kind))) {
        vk::set_error("vk_divide_plan: bad arguments");
        return VK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    int64_t *bc = (int64_t *)scratch;
    const int64_t nb = (n + DV_BLOCK - 1) / DV_BLOCK;
    if (nb > 0)
        hipLaunchKernelGGL(k_divide_count, dim3((unsigned)nb), dim3(256), 0, s, divide, n, bc);
    hipLaunchKernelGGL(k_divide_scan_blocks, dim3(1), dim3(256), 0, s, bc, nb, n, n_out);
    if (nb > 0)
        hipLaunchKernelGGL(k_divide_place, dim3((unsigned)nb), dim3(256), 0, s, divide, n, bc, nb, src_index, kind);
    return vk::launch_check("vk_divide_plan");
}

// ---------------------------------------------------------------------------
// population plan: division and removal in one stable compaction
// ---------------------------------------------------------------------------
//
// The same three launches as the division plan, carrying two counts per block: the agents
// removed and the mothers kept (divide && !remove).  An agent with R removed agents and M kept
// mothers before it goes to slot a - R - M when it stays as it is, to n_keep + 2 M (and the
// slot after) when it divides, nowhere when it is removed; n_keep = n - R_total - M_total.
// scratch: removed[nb + 1] | mothers[nb + 1], int64 (the totals in element nb).

extern "C" int64_t vk_population_scratch_bytes(int64_t n) {
    if (n < 0) return 0;
    const int64_t nb = (n + DV_BLOCK - 1) / DV_BLOCK;
    return 2 * (nb + 2) * (int64_t)sizeof(int64_t);
}

__global__ __launch_bounds__(256) void k_population_count(const int32_t *__restrict__ divide,
                                                          const int32_t *__restrict__ remove, int64_t n,
                                                          int64_t *__restrict__ removed,
                                                          int64_t *__restrict__ mothers) {
    const int64_t base = (int64_t)blockIdx.x * DV_BLOCK;
    int cr = 0, cm = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t a = base + k * 256 + threadIdx.x;
        if (a < n) {
            const int r = remove ? (remove[a] != 0) : 0;
            const int d = divide ? (divide[a] != 0) : 0;
            cr += r;
            cm += d & (r ^ 1);
        }
    }
    __shared__ int part_r[4], part_m[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cr += __shfl_xor(cr, o);
        cm += __shfl_xor(cm, o);
    }
    if ((threadIdx.x & 63) == 0) {
        part_r[threadIdx.x >> 6] = cr;
        part_m[threadIdx.x >> 6] = cm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        removed[blockIdx.x] = part_r[0] + part_r[1] + part_r[2] + part_r[3];
        mothers[blockIdx.x] = part_m[0] + part_m[1] + part_m[2] + part_m[3];
    }
}

// one block: exclusive scans of both arrays of nb block counts in place; the totals go to
// element nb of each, n - removed + mothers -> *n_out
__global__ __launch_bounds__(256) void k_population_scan_blocks(int64_t *__restrict__ removed,
                                                                int64_t *__restrict__ mothers, int64_t nb,
                                                                int64_t n, int64_t *__restrict__ n_out) {
    __shared__ int64_t carry[2];
    __shared__ int64_t wsum[2][4];
    if (threadIdx.x < 2) carry[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t b0 = 0; b0 < nb; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        const int64_t vr = b < nb ? removed[b] : 0, vm = b < nb ? mothers[b] : 0;
        int64_t xr = vr, xm = vm;     // inclusive wave scans
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t yr = __shfl_up(xr, o), ym = __shfl_up(xm, o);
            if (lane >= o) {
                xr += yr;
                xm += ym;
            }
        }
        if (lane == 63) {
            wsum[0][w] = xr;
            wsum[1][w] = xm;
        }
        __syncthreads();
        int64_t wr = 0, wm = 0;
        for (int k = 0; k < w; ++k) {
            wr += wsum[0][k];
            wm += wsum[1][k];
        }
        const int64_t er = carry[0] + wr + xr - vr, em = carry[1] + wm + xm - vm;
        __syncthreads();
        if (b < nb) {
            removed[b] = er;
            mothers[b] = em;
        }
        if (threadIdx.x == 255) {
            carry[0] = er + vr;
            carry[1] = em + vm;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        removed[nb] = carry[0];
        mothers[nb] = carry[1];
        *n_out = n - carry[0] + carry[1];
    }
}

__global__ __launch_bounds__(256) void k_population_place(const int32_t *__restrict__ divide,
                                                          const int32_t *__restrict__ remove, int64_t n,
                                                          const int64_t *__restrict__ removed_off,
                                                          const int64_t *__restrict__ mothers_off, int64_t nb,
                                                          int32_t *__restrict__ src_index,
                                                          int32_t *__restrict__ kind) {
    const int64_t base = (int64_t)blockIdx.x * DV_BLOCK;
    const int64_t n_keep = n - removed_off[nb] - mothers_off[nb];
    __shared__ int wcount[2][4];
    // per-thread 4 consecutive agents -> thread-level counts -> block exclusive scans
    const int64_t a0 = base + (int64_t)threadIdx.x * 4;
    int fr[4], fm[4], cr = 0, cm = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        fr[k] = (a0 + k < n && remove) ? (remove[a0 + k] != 0) : 0;
        fm[k] = (a0 + k < n && divide) ? ((divide[a0 + k] != 0) & (fr[k] ^ 1)) : 0;
        cr += fr[k];
        cm += fm[k];
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int xr = cr, xm = cm;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int yr = __shfl_up(xr, o), ym = __shfl_up(xm, o);
        if (lane >= o) {
            xr += yr;
            xm += ym;
        }
    }
    if (lane == 63) {
        wcount[0][w] = xr;
        wcount[1][w] = xm;
    }
    __syncthreads();
    int wr = 0, wm = 0;
    for (int k = 0; k < w; ++k) {
        wr += wcount[0][k];
        wm += wcount[1][k];
    }
    int64_t r = removed_off[blockIdx.x] + wr + xr - cr;   // removed before a0
    int64_t m = mothers_off[blockIdx.x] + wm + xm - cm;   // kept mothers before a0
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t a = a0 + k;
        if (a >= n) break;
        if (fr[k]) {
            ++r;
        } else if (fm[k]) {
            const int64_t j = n_keep + 2 * m;     // < n_out <= 2 n
            src_index[j] = (int32_t)a;
            kind[j] = 0;
            src_index[j + 1] = (int32_t)a;
            kind[j + 1] = 1;
            ++m;
        } else {
            const int64_t j = a - r - m;          // >= 0: r + m counts agents before a
            src_index[j] = (int32_t)a;
            kind[j] = -1;
        }
    }
}

extern "C" int vk_population_plan(const int32_t *divide, const int32_t *remove, int64_t n, int32_t *src_index,
                                  int32_t *kind, int64_t *n_out, void *scratch, vk_stream_t stream) {
    if (n < 0 || n > 0x3fffffff || !n_out || !scratch || (n > 0 && (!src_index || !kind))) {
        vk::set_error("vk_population_plan: bad arguments");
        return VK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (n + DV_BLOCK - 1) / DV_BLOCK;
    int64_t *removed = (int64_t *)scratch, *mothers = removed + nb + 2;
    if (nb > 0)
        hipLaunchKernelGGL(k_population_count, dim3((unsigned)nb), dim3(256), 0, s, divide, remove, n, removed,
                           mothers);
    hipLaunchKernelGGL(k_population_scan_blocks, dim3(1), dim3(256), 0, s, removed, mothers, nb, n, n_out);
    if (nb > 0)
        hipLaunchKernelGGL(k_population_place, dim3((unsigned)nb), dim3(256), 0, s, divide, remove, n, removed,
                           mothers, nb, src_index, kind);
    return vk::launch_check("vk_population_plan");
}

// ---------------------------------------------------------------------------
// gathers with dividers
// ---------------------------------------------------------------------------

template <typename T, int DIV>
__global__ __launch_bounds__(256) void k_divide_gather(int64_t n_out, const int32_t *__restrict__ src_index,
                                                       const int32_t *__restrict__ kind, const T *__restrict__ src,
                                                       int64_t ld_src, T *__restrict__ dst, int64_t ld_dst, int rows) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    const int64_t a = src_index[j];
    const bool daughter = kind[j] >= 0;
    for (int r = 0; r < rows; ++r) {
        T v = src[(int64_t)r * ld_src + a];
        if (daughter) {
            if constexpr (DIV == VK_DIVIDE_SPLIT) v = v / (T)2;
            if constexpr (DIV == VK_DIVIDE_ZERO) v = (T)0;
        }
        dst[(int64_t)r * ld_dst + j] = v;
    }
}

extern "C" int vk_divide_gather(int64_t n_out, const int32_t *src_index, const int32_t *kind, const void *src,
                                int64_t ld_src, void *dst, int64_t ld_dst, int32_t rows, int32_t elem_bytes,
                                int32_t divider, vk_stream_t stream) {
    if (n_out < 0 || ld_dst < n_out || rows < 0 || (n_out > 0 && rows > 0 && (!src || !dst || !src_index || !kind)) ||
        (elem_bytes != 4 && elem_bytes != 8) || divider < 0 || divider > 2 ||
        (divider == VK_DIVIDE_SPLIT && elem_bytes != 8)) {
        vk::set_error("vk_divide_gather: bad arguments");
        return VK_ERR_ARG;
    }
    if (n_out == 0 || rows == 0) return VK_OK;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g((unsigned)((n_out + 255) / 256)), b(256);
#define VK_G(T, D) hipLaunchKernelGGL((k_divide_gather<T, D>), g, b, 0, s, n_out, src_index, kind, (const T *)src, ld_src, (T *)dst, ld_dst, rows)
    if (elem_bytes == 8) {
        if (divider == VK_DIVIDE_SET) VK_G(double, VK_DIVIDE_SET);
        else if (divider == VK_DIVIDE_SPLIT) VK_G(double, VK_DIVIDE_SPLIT);
        else VK_G(double, VK_DIVIDE_ZERO);
    } else {
        if (divider == VK_DIVIDE_SET) VK_G(int32_t, VK_DIVIDE_SET);
        else VK_G(int32_t, VK_DIVIDE_ZERO);
    }
#undef VK_G
    return vk::launch_check("k_divide_gather");
}

__global__ __launch_bounds__(256) void k_divide_lineage(int64_t n_out, const int32_t *__restrict__ src_index,
                                                        const int32_t *__restrict__ kind,
                                                        const int32_t *__restrict__ root_src,
                                                        const int32_t *__restrict__ depth_src,
                                                        const uint64_t *__restrict__ path_src,
                                                        int32_t *__restrict__ root_dst, int32_t *__restrict__ depth_dst,
                                                        uint64_t *__restrict__ path_dst, int32_t *overflow) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    const int64_t a = src_index[j];
    const int k = kind[j];
    int32_t d = depth_src[a];
    uint64_t pth = path_src[a];
    if (k >= 0) {
        if (d >= 64 && overflow) *overflow = 1;
        pth = (pth << 1) | (uint64_t)k;
        d = d + 1;
    }
    root_dst[j] = root_src[a];
    depth_dst[j] = d;
    path_dst[j] = pth;
}

extern "C" int vk_divide_lineage(int64_t n_out, const int32_t *src_index, const int32_t *kind, const int32_t *root_src,
                                 const int32_t *depth_src, const uint64_t *path_src, int32_t *root_dst,
                                 int32_t *depth_dst, uint64_t *path_dst, int32_t *overflow, vk_stream_t stream) {
    if (n_out < 0 || (n_out > 0 && (!src_index || !kind || !root_src || !depth_src || !path_src || !root_dst ||
                                    !depth_dst || !path_dst))) {
        vk::set_error("vk_divide_lineage: bad arguments");
        return VK_ERR_ARG;
    }
    if (n_out == 0) return VK_OK;
    hipLaunchKernelGGL(k_divide_lineage, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       n_out, src_index, kind, root_src, depth_src, path_src, root_dst, depth_dst, path_dst, overflow);
    return vk::launch_check("k_divide_lineage");
}

__global__ __launch_bounds__(256) void k_divide_locations(int64_t n_out, const int32_t *__restrict__ src_index,
                                                          const int32_t *__restrict__ kind,
                                                          const double *__restrict__ loc_src, int64_t ld_src,
                                                          double *__restrict__ loc_dst, int64_t ld_dst,
                                                          const double *__restrict__ cell_dst) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    const int64_t a = src_index[j];
    const int k = kind[j];
    double x = loc_src[a], y = loc_src[ld_src + a];
    if (k >= 0) {
        // parent values: length was split into this slot (exact halving), angle copied
        const double parent_length = cell_dst[(int64_t)VK_CELL_LENGTH * ld_dst + j] * 2.0;
        const double angle = cell_dst[(int64_t)VK_CELL_ANGLE * ld_dst + j];
        const double ratio = k == 0 ? -0.25 : 0.25;
        const double dx = parent_length * ratio * cos(angle);
        const double dy = parent_length * ratio * sin(angle);
        x = x + dx;
        y = y + dy;
    }
    loc_dst[j] = x;
    loc_dst[ld_dst + j] = y;
}

extern "C" int vk_divide_locations(int64_t n_out, const int32_t *src_index, const int32_t *kind, const double *loc_src,
                                   int64_t ld_src, double *loc_dst, int64_t ld_dst, const double *cell_dst,
                                   vk_stream_t stream) {
    if (n_out < 0 || ld_dst < n_out || (n_out > 0 && (!src_index || !kind || !loc_src || !loc_dst || !cell_dst))) {
        vk::set_error("vk_divide_locations: bad arguments");
        return VK_ERR_ARG;
    }
    if (n_out == 0) return VK_OK;
    hipLaunchKernelGGL(k_divide_locations, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       n_out, src_index, kind, loc_src, ld_src, loc_dst, ld_dst, cell_dst);
    return vk::launch_check("k_divide_locations");
}
