// Antibiotic response, one agent per lane: membrane diffusion through porins,
// the death detector and the freeze, and the exchange of float counts.
//
// CellEnvironmentDiffusion.next_update (vivarium/processes/
// diffusion_cell_environment.py:92-138): rate = sum([porin * permeability ...])
// (Python's sum: from 0, in dict order), flux_mmol = (internal - external) *
// rate * timestep, the cell takes -(flux_mmol / volume).to(mmol/L) and the field
// takes (flux_mmol * N_A).to(count), a float.
// DeathFreezeState.next_update (vivarium/processes/death.py:105-118, 197-219):
// a detector fires when the step-start concentration is strictly above its
// threshold; the update of that step still applies, and the deleted processes
// are gone from the next step on.
//
// The kinetics, expression and growth launches stay as they are and run on every
// agent: `begin` saves the columns they overwrite for frozen agents, `end` puts
// them back.  Descriptor tables are small and the same for every agent, so their
// reads are wave-uniform (scalar-cache loads, ldc()).  -ffp-contract=off and the
// operation order below give the reference's rounding.

#include <stdint.h>

#include "vk_internal.h"

__global__ __launch_bounds__(256) void k_response_begin(
    vk_response_table t, int64_t n, int64_t ld, double dt, const double *__restrict__ conc,
    const double *__restrict__ volume, const int32_t *__restrict__ frozen, int32_t *__restrict__ dying,
    double *__restrict__ delta, double *__restrict__ fcounts, double *__restrict__ save_conc,
    const double *__restrict__ flux, double *__restrict__ save_flux, const int32_t *__restrict__ status,
    int32_t *__restrict__ save_status, const int32_t *__restrict__ nsteps, int32_t *__restrict__ save_nsteps) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const bool fr = frozen[a] != 0;
    // detectors (death.py:115-118): any key strictly above its threshold
    bool die = false;
    for (int d = 0; d < t.n_det; ++d) die = die || conc[(int64_t)ldc(t.det_row, d) * ld + a] > ldc(t.det_thr, d);
    dying[a] = (!fr && die) ? 1 : 0;
    // membrane (diffusion_cell_environment.py:93-137)
    if (t.n_mol > 0) {
        double rate = 0.0;
        for (int p = 0; p < t.n_porin; ++p)
            rate = rate + conc[(int64_t)ldc(t.porin_row, p) * ld + a] * ldc(t.porin_perm, p);
        const double vol = volume ? volume[a] : t.volume_fl;
        for (int m = 0; m < t.n_mol; ++m) {
            const double ci = conc[(int64_t)ldc(t.mol_int_row, m) * ld + a];
            const double ce = conc[(int64_t)ldc(t.mol_ext_row, m) * ld + a];
            const double flux_mmol = (ci - ce) * rate * dt;
            delta[(int64_t)m * ld + a] = -(flux_mmol / vol * 1e15);
            fcounts[(int64_t)m * ld + a] = flux_mmol * 1e-3 * t.avogadro;
        }
    }
    if (fr) {   // what the kinetics launch is about to overwrite
        for (int s = 0; s < t.n_save; ++s) save_conc[(int64_t)s * ld + a] = conc[(int64_t)ldc(t.save_row, s) * ld + a];
        for (int r = 0; r < t.n_flux; ++r) save_flux[(int64_t)r * ld + a] = flux[(int64_t)r * ld + a];
        if (status) save_status[a] = status[a];
        if (nsteps) save_nsteps[a] = nsteps[a];
    }
}

static bool table_ok(const vk_response_table *t) {
    return t && t->n_mol >= 0 && t->n_porin >= 0 && t->n_det >= 0 && t->n_save >= 0 && t->n_expr >= 0 &&
           t->n_flux >= 0 && t->n_ext >= 0 && (!t->n_mol || (t->mol_int_row && t->mol_ext_row)) &&
           (!t->n_porin || (t->porin_row && t->porin_perm)) && (!t->n_det || (t->det_row && t->det_thr)) &&
           (!t->n_save || t->save_row) && (!t->n_expr || t->expr_row);
}

extern "C" int vk_response_begin(const vk_response_table *t, int64_t n, int64_t ld, double dt, const double *conc,
                                 const double *volume, const int32_t *frozen, int32_t *dying, double *delta,
                                 double *fcounts, double *save_conc, const double *flux, double *save_flux,
                                 const int32_t *status, int32_t *save_status, const int32_t *nsteps,
                                 int32_t *save_nsteps, vk_stream_t stream) {
    if (!table_ok(t) || n < 0 || ld < n ||
        (n > 0 && (!conc || !frozen || !dying || (t->n_mol && (!delta || !fcounts)) || (t->n_save && !save_conc) ||
                   (t->n_flux && (!flux || !save_flux)) || (status && !save_status) || (nsteps && !save_nsteps)))) {
        vk::set_error("vk_response_begin: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0) return VK_OK;
    hipLaunchKernelGGL(k_response_begin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *t, n,
                       ld, dt, conc, volume, frozen, dying, delta, fcounts, save_conc, flux, save_flux, status,
                       save_status, nsteps, save_nsteps);
    return vk::launch_check("k_response_begin");
}

__global__ __launch_bounds__(256) void k_response_end(
    vk_response_table t, int64_t n, int64_t ld, double *__restrict__ conc, const double *__restrict__ delta,
    const double *__restrict__ expr_update, int32_t *__restrict__ frozen, const int32_t *__restrict__ dying,
    int32_t *__restrict__ dead, const double *__restrict__ save_conc, double *__restrict__ flux,
    const double *__restrict__ save_flux, int32_t *__restrict__ status, const int32_t *__restrict__ save_status,
    int32_t *__restrict__ nsteps, const int32_t *__restrict__ save_nsteps, int64_t *__restrict__ counts) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    if (frozen[a] != 0) {
        // the deleted processes' results are discarded; their exchange is nothing
        for (int s = 0; s < t.n_save; ++s) conc[(int64_t)ldc(t.save_row, s) * ld + a] = save_conc[(int64_t)s * ld + a];
        for (int r = 0; r < t.n_flux; ++r) flux[(int64_t)r * ld + a] = save_flux[(int64_t)r * ld + a];
        if (status) status[a] = save_status[a];
        if (nsteps) nsteps[a] = save_nsteps[a];
        for (int e = 0; e < t.n_ext; ++e) counts[(int64_t)e * ld + a] = 0;
    } else if (expr_update) {
        // ODE_expression's accumulate update, after the kinetics' (process order)
        for (int j = 0; j < t.n_expr; ++j) {
            const int64_t r = (int64_t)ldc(t.expr_row, j) * ld + a;
            conc[r] = conc[r] + expr_update[(int64_t)j * ld + a];
        }
    }
    // the membrane's update comes last: (conc + delta_kinetics) + delta_membrane
    for (int m = 0; m < t.n_mol; ++m) {
        const int64_t r = (int64_t)ldc(t.mol_int_row, m) * ld + a;
        conc[r] = conc[r] + delta[(int64_t)m * ld + a];
    }
    if (dying[a]) {   // death.py:207-217: dead := 1, the processes go
        dead[a] = 1;
        frozen[a] = 1;
    }
}

extern "C" int vk_response_end(const vk_response_table *t, int64_t n, int64_t ld, double *conc, const double *delta,
                               const double *expr_update, int32_t *frozen, const int32_t *dying, int32_t *dead,
                               const double *save_conc, double *flux, const double *save_flux, int32_t *status,
                               const int32_t *save_status, int32_t *nsteps, const int32_t *save_nsteps,
                               int64_t *counts, vk_stream_t stream) {
    if (!table_ok(t) || n < 0 || ld < n ||
        (n > 0 && (!conc || !frozen || !dying || !dead || (t->n_mol && !delta) || (t->n_save && !save_conc) ||
                   (t->n_flux && (!flux || !save_flux)) || (status && !save_status) || (nsteps && !save_nsteps) ||
                   (t->n_ext && !counts)))) {
        vk::set_error("vk_response_end: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0) return VK_OK;
    hipLaunchKernelGGL(k_response_end, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *t, n, ld,
                       conc, delta, expr_update, frozen, dying, dead, save_conc, flux, save_flux, status, save_status,
                       nsteps, save_nsteps, counts);
    return vk::launch_check("k_response_end");
}

// A frozen agent's growth is discarded the same way around vk_cell_step.  An agent
// detected in this step (dying) is frozen already but still grows and may divide: the
// step of detection applies every update.
__global__ __launch_bounds__(256) void k_response_cells(int restore, int64_t n, int64_t ld,
                                                        const int32_t *__restrict__ frozen,
                                                        const int32_t *__restrict__ dying, double *__restrict__ cell,
                                                        double *__restrict__ m2c, int32_t *__restrict__ divide,
                                                        double *__restrict__ save_cell, double *__restrict__ save_m2c,
                                                        int32_t *__restrict__ save_divide) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n || frozen[a] == 0 || dying[a] != 0) return;
    if (restore) {
        for (int r = 0; r < VK_CELL_ROWS; ++r) cell[(int64_t)r * ld + a] = save_cell[(int64_t)r * ld + a];
        m2c[a] = save_m2c[a];
        divide[a] = save_divide[a];
    } else {
        for (int r = 0; r < VK_CELL_ROWS; ++r) save_cell[(int64_t)r * ld + a] = cell[(int64_t)r * ld + a];
        save_m2c[a] = m2c[a];
        save_divide[a] = divide[a];
    }
}

extern "C" int vk_response_cells(int32_t restore, int64_t n, int64_t ld, const int32_t *frozen,
                                 const int32_t *dying, double *cell, double *m2c, int32_t *divide, double *save_cell, double *save_m2c,
                                 int32_t *save_divide, vk_stream_t stream) {
    if (n < 0 || ld < n || (n > 0 && (!frozen || !dying || !cell || !m2c || !divide || !save_cell || !save_m2c || !save_divide))) {
        vk::set_error("vk_response_cells: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0) return VK_OK;
    hipLaunchKernelGGL(k_response_cells, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (int)restore, n, ld, frozen, dying, cell, m2c, divide, save_cell, save_m2c, save_divide);
    return vk::launch_check("k_response_cells");
}

// count / (bin_volume * N_A) mol/L, to mmol/L (registry.py:179-182)
__device__ __forceinline__ double mM_i(int64_t count, double bva) { return ((double)count / bva) * 1000.0; }
__device__ __forceinline__ double mM_f(double count, double bva) { return (count / bva) * 1000.0; }

// k_exchange_ordered (vk_lattice.hip) with the float counts beside the int ones.  The
// head of a bin's segment walks it once per plane; a plane fed by both arrays takes
// each agent's int count and then its float count -- the order in which the
// reference applies one agent's updates after another's.
__global__ __launch_bounds__(256) void k_exchange_ordered_mixed(
    double *__restrict__ fields, int64_t field_stride, const int32_t *__restrict__ sorted_bin,
    const int32_t *__restrict__ order, int n, const int64_t *__restrict__ counts, int64_t ld,
    const int32_t *__restrict__ map_count, const int32_t *__restrict__ map_field, int n_map,
    const double *__restrict__ fcounts, int64_t ld_f, const int32_t *__restrict__ map_fcount,
    const int32_t *__restrict__ map_ffield, int n_fmap, double bva) {
    const int k0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (k0 >= n) return;
    const int32_t bin = sorted_bin[k0];
    if (k0 > 0 && sorted_bin[k0 - 1] == bin) return;
    int k1 = k0 + 1;
    while (k1 < n && sorted_bin[k1] == bin) ++k1;
    for (int i = 0; i < n_map; ++i) {
        const int f = ldc(map_field, i);
        const int64_t *cr = counts + (int64_t)ldc(map_count, i) * ld;
        const double *fr = nullptr;   // the float row going to the same plane, if any
        for (int j = 0; j < n_fmap; ++j)
            if (ldc(map_ffield, j) == f) {
                fr = fcounts + (int64_t)ldc(map_fcount, j) * ld_f;
                break;
            }
        double *p = fields + (int64_t)f * field_stride + bin;
        double v = *p;
        for (int k = k0; k < k1; ++k) {
            const int64_t a = order[k];
            v = v + mM_i(cr[a], bva);
            if (fr) v = v + mM_f(fr[a], bva);
        }
        *p = v;
    }
    for (int j = 0; j < n_fmap; ++j) {   // planes only the float counts feed
        const int f = ldc(map_ffield, j);
        bool mixed = false;
        for (int i = 0; i < n_map; ++i) mixed = mixed || ldc(map_field, i) == f;
        if (mixed) continue;
        const double *fr = fcounts + (int64_t)ldc(map_fcount, j) * ld_f;
        double *p = fields + (int64_t)f * field_stride + bin;
        double v = *p;
        for (int k = k0; k < k1; ++k) v = v + mM_f(fr[order[k]], bva);
        *p = v;
    }
}

extern "C" int vk_exchange_ordered_mixed(double *fields, int64_t field_stride, const int32_t *sorted_bin,
                                         const int32_t *order, int64_t n, const int64_t *counts, int64_t ld,
                                         const int32_t *map_count, const int32_t *map_field, int32_t n_map,
                                         const double *fcounts, int64_t ld_f, const int32_t *map_fcount,
                                         const int32_t *map_ffield, int32_t n_fmap, double binvol_avogadro,
                                         vk_stream_t stream) {
    if (!counts) n_map = n_map == 0 ? 0 : -1;
    if (!fcounts) n_fmap = n_fmap == 0 ? 0 : -1;
    if (n < 0 || n >= INT32_MAX || n_map < 0 || n_fmap < 0 || (n_map > 0 && ld < n) || (n_fmap > 0 && ld_f < n) ||
        (n > 0 && n_map + n_fmap > 0 && (!fields || !sorted_bin || !order)) ||
        (n > 0 && n_map > 0 && (!map_count || !map_field)) || (n > 0 && n_fmap > 0 && (!map_fcount || !map_ffield))) {
        vk::set_error("vk_exchange_ordered_mixed: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0 || n_map + n_fmap == 0) return VK_OK;
    hipLaunchKernelGGL(k_exchange_ordered_mixed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       fields, field_stride, sorted_bin, order, (int)n, counts, ld, map_count, map_field, n_map, fcounts,
                       ld_f, map_fcount, map_ffield, n_fmap, binvol_avogadro);
    return vk::launch_check("k_exchange_ordered_mixed");
}

__global__ __launch_bounds__(256) void k_exchange_atomic_f64(double *__restrict__ fields, int64_t field_stride,
                                                             const int32_t *__restrict__ bin_lin, int64_t n,
                                                             const double *__restrict__ fcounts, int64_t ld,
                                                             const int32_t *__restrict__ map_count,
                                                             const int32_t *__restrict__ map_field, int n_map,
                                                             double bva) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const int64_t b = bin_lin[a];
    for (int i = 0; i < n_map; ++i) {
        const double c = fcounts[(int64_t)ldc(map_count, i) * ld + a];
        unsafeAtomicAdd(fields + (int64_t)ldc(map_field, i) * field_stride + b, mM_f(c, bva));
    }
}

extern "C" int vk_exchange_atomic_f64(double *fields, int64_t field_stride, const int32_t *bin_lin, int64_t n,
                                      const double *fcounts, int64_t ld, const int32_t *map_count,
                                      const int32_t *map_field, int32_t n_map, double binvol_avogadro,
                                      vk_stream_t stream) {
    if (n < 0 || ld < n || n_map < 0 ||
        (n > 0 && n_map > 0 && (!fields || !bin_lin || !fcounts || !map_count || !map_field))) {
        vk::set_error("vk_exchange_atomic_f64: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0 || n_map == 0) return VK_OK;
    hipLaunchKernelGGL(k_exchange_atomic_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       fields, field_stride, bin_lin, n, fcounts, ld, map_count, map_field, n_map, binvol_avogadro);
    return vk::launch_check("k_exchange_atomic_f64");
}
