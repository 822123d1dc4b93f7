/*
 * vk_kinetics.h -- C ABI of the MI355X batched agent-kinetics engine.
 *
 * Drop-in boundary for the per-agent hot path of CovertLab/Lens ("vivarium").
 * The reference has no native FFI for this path: it is pure Python calling
 * numpy/scipy.  Each entry point below replaces one reference call site; the
 * Python host layer (lens_amd/native.py via ctypes) is the only caller.  See
 * INTEGRATION.md for the binding a vivarium maintainer would add.
 *
 *   vk_table_create / vk_table_destroy
 *       replaces KineticFluxModel.__init__ -> make_configuration /
 *       make_rate_laws (vivarium/library/kinetic_rate_laws.py:262-275,
 *       :43-98, :183-237).  The host compiler (lens_amd/rate_law_compiler.py)
 *       flattens the closures into the index arrays of vk_table_desc.
 *   vk_rate_fluxes
 *       replaces KineticFluxModel.get_fluxes (kinetic_rate_laws.py:277-297).
 *   vk_step_euler
 *       replaces ConvenienceKinetics.next_update
 *       (vivarium/processes/convenience_kinetics.py:303-352): one forward-Euler
 *       step, integer exchange counts truncated toward zero (:331).
 *   vk_step_dopri5
 *       replaces the reference's scipy.integrate.odeint step
 *       (vivarium/processes/Kremling2007_transport.py:384) for convenience
 *       networks: adaptive Dormand-Prince 5(4) over [0, dt] on the augmented
 *       system (internal species + per-reaction flux integrals).
 *   vk_field_uniform + vk_diffuse
 *       replace DiffusionField.diffuse / diffusion_delta
 *       (vivarium/processes/diffusion_field.py:385-407): fixed dt=0.01
 *       substeps of the reflect-boundary 5-point Laplacian, uniform-field skip.
 *   vk_gather
 *       replaces DiffusionField.get_local_environments (:362-379).
 *   vk_exchange_sorted / vk_exchange_atomic
 *       replace update_field_with_exchange (vivarium/core/registry.py:149-183)
 *       applied once per agent by Store.apply_update.
 *   vk_bin_sites
 *       replaces get_bin_site (vivarium/library/lattice_utils.py:18-40).
 *   vk_cell_step / vk_divide_*, vk_kremling_step, vk_expression_step,
 *   vk_motility_step, vk_flagella_step, vk_contact_step, vk_contact_step_channels, vk_population_plan,
 *   vk_flagella_counts, vk_divide_flagella, vk_ssa_step, vk_ssa_propensities, vk_divide_counts,
 *   vk_ssa_flagella_target, vk_colony_metrics, vk_translation_step, vk_divide_ribosomes,
 *   vk_transcription_step, vk_rna_degradation_step, vk_cell_step_tree
 *       are introduced by the comment blocks above their declarations.
 *
 * Conventions
 *   - All array arguments are DEVICE pointers except vk_table_desc's, which are
 *     host pointers copied at vk_table_create.  The library never frees caller
 *     memory; vk_table is the only object it owns.
 *   - Agent arrays are structure-of-arrays with row stride `ld` (>= n_agents):
 *     element (row, agent) lives at [row * ld + agent].
 *   - Every call is asynchronous on `stream` (a hipStream_t; NULL = legacy
 *     default stream) and returns a vk_status.  Per-agent problems are
 *     reported in the caller's int32 status[] array (vk_agent_status bits).
 *   - All arithmetic is FP64.
 */
#ifndef VK_KINETICS_H
#define VK_KINETICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VK_ABI_VERSION 1

typedef void *vk_stream_t;        /* hipStream_t */
typedef struct vk_table vk_table; /* opaque, device-resident reaction table */

enum vk_status {
    VK_OK = 0,
    VK_ERR_ARG = 1,   /* bad argument (null pointer, negative size, ...) */
    VK_ERR_HIP = 2,   /* a HIP runtime call failed; see vk_last_error() */
    VK_ERR_LIMIT = 3, /* network too large for the requested kernel variant */
    VK_ERR_NOMEM = 4
};

enum vk_agent_status {
    VK_AGENT_OK = 0,
    VK_AGENT_MAX_STEPS = 1,   /* integrator hit max_steps before t = dt */
    VK_AGENT_H_UNDERFLOW = 2, /* step size fell below 1e-14 * dt */
    VK_AGENT_NONFINITE = 4    /* NaN/Inf in the state or an exchange count */
};

/* Flattened rate-law table (lens_amd/rate_law_compiler.py:RateLawTable). */
typedef struct vk_table_desc {
    int32_t n_species;   /* rows of the agent concentration array            */
    int32_t n_dyn;       /* rows [0, n_dyn) receive deltas (non-external)    */
    int32_t n_reactions; /* flux rows                                        */
    int32_t n_rate_laws; /* (reaction, enzyme) closures, get_fluxes order    */
    int32_t n_params;    /* per-agent parameter rows (kcat, Km)              */
    int32_t n_ext;       /* exchange-count rows (external molecules)         */
    int32_t n_sets;      /* cofactor / partition sets                        */
    int32_t n_members;   /* (species, Km slot) members of all sets           */
    int32_t n_upd;       /* stoichiometry entries of dyn species             */
    int32_t n_exch;      /* stoichiometry entries of external molecules      */
    const int32_t *rl_reaction; /* [n_rate_laws] reaction row               */
    const int32_t *rl_enzyme;   /* [n_rate_laws] species row of the enzyme  */
    const int32_t *rl_kcat;     /* [n_rate_laws] parameter row of kcat_f    */
    const int32_t *rl_num_ptr;  /* [n_rate_laws+1] numerator sets           */
    const int32_t *rl_den_ptr;  /* [n_rate_laws+1] partition sets           */
    const int32_t *set_ptr;     /* [n_sets+1] members                       */
    const int32_t *mem_species; /* [n_members] species row                  */
    const int32_t *mem_param;   /* [n_members] parameter row of the Km      */
    const int32_t *upd_ptr;     /* [n_dyn+1]                                */
    const int32_t *upd_rxn;     /* [n_upd]                                  */
    const double *upd_coeff;    /* [n_upd]                                  */
    const int32_t *ex_ptr;      /* [n_ext+1]                                */
    const int32_t *ex_rxn;      /* [n_exch]                                 */
    const double *ex_coeff;     /* [n_exch]                                 */
} vk_table_desc;

typedef struct vk_ode_opts {
    double rtol;       /* relative tolerance (scipy RK45 semantics)          */
    double atol;       /* absolute tolerance                                 */
    int32_t max_steps; /* attempted steps per agent per call                 */
    int32_t variant;   /* 0 = agent-per-thread, table walked at run time
                              (n_dyn + n_reactions <= 32);
                          1 = agent-per-wavefront: one 64-lane wave per agent,
                              wave-reduced error norm, wave-uniform step
                              control (n_dyn + n_reactions <= 512);
                          2 = agent-per-thread, network-specialised
                              (vk_table_specialize);
                          3 = agent-per-wavefront, network-specialised:
                              rate laws padded to one shape per round of 64
                              lanes, per-lane operands in VGPRs
                              (vk_table_specialize with a wavefront source) */
} vk_ode_opts;

int vk_abi_version(void);
const char *vk_last_error(void);

int vk_table_create(const vk_table_desc *desc, vk_table **out);
int vk_table_destroy(vk_table *table);

/* Attach a network-specialised integrator to the table: `source` is the HIP
 * source lens_amd/codegen.py generates from the same table, compiled with
 * hiprtc for gfx950.  It defines `vk_dopri5_spec` (agent per lane: straight-
 * line rate laws, every species/parameter/stage value in VGPRs; used for
 * opts->variant == 2), `vk_dopri5_wspec` (agent per wavefront; variant 3),
 * or both. */
int vk_table_specialize(vk_table *table, const char *source);

/* flux[r*ld + a] = sum over the reaction's rate laws (exact reference order). */
int vk_rate_fluxes(const vk_table *t, int64_t n_agents, int64_t ld,
                   const double *params, const double *conc, double *flux,
                   vk_stream_t stream);

/* One reference Euler step.  If delta is NULL, conc rows [0, n_dyn) are
 * updated in place (conc += delta, the accumulate updater); otherwise conc is
 * left untouched and delta[s*ld+a] receives the reference's update value
 * (0 + sum_j (coeff_j*flux)*dt).  flux[r*ld+a] (set);
 * counts[e*ld+a] = sum_j trunc(((coeff_j*flux)*dt)*m2c[a]).               */
int vk_step_euler(const vk_table *t, int64_t n_agents, int64_t ld, double dt,
                  const double *params, double *conc, const double *mmol_to_counts,
                  double *delta, double *flux, int64_t *counts, int32_t *status,
                  vk_stream_t stream);

/* Adaptive Dormand-Prince 5(4) over [0, dt].  External/enzyme rows are held.
 * delta as for vk_step_euler (NULL: integrate conc in place; else
 * delta = y(dt) - y(0), conc untouched).  h_state[a]: step-size carry-over
 * (in/out; <= 0 selects the initial step).  flux = integral(flux)/dt;
 * counts from the integral; nsteps = attempted steps.                     */
int vk_step_dopri5(const vk_table *t, int64_t n_agents, int64_t ld, double dt,
                   const vk_ode_opts *opts, const double *params, double *conc,
                   const double *mmol_to_counts, double *delta, double *h_state,
                   double *flux, int64_t *counts, int32_t *status, int32_t *nsteps,
                   vk_stream_t stream);

/* vk_step_dopri5 (variant 2, after vk_table_specialize) fused with the
 * gather of the NEXT step's local environment: once agent a is integrated,
 * conc[map_row[i] * ld + a] = fields[map_field[i] * field_stride + bin_lin[a]]
 * for i < n_map (<= 8) -- the values vk_gather writes when it runs right after
 * the kinetics (DiffusionField.get_local_environments, diffusion_field.py:
 * 362-379, feeding ConvenienceKinetics.next_update, convenience_kinetics.py:
 * 303-352, one step later).  One launch and one sweep of the field lines
 * instead of two.                                                          */
int vk_step_dopri5_gather(const vk_table *t, int64_t n_agents, int64_t ld, double dt,
                          const vk_ode_opts *opts, const double *params, double *conc,
                          const double *mmol_to_counts, double *h_state, double *flux,
                          int64_t *counts, int32_t *status, int32_t *nsteps,
                          const double *fields, int64_t field_stride, const int32_t *bin_lin,
                          const int32_t *map_field, const int32_t *map_row, int32_t n_map,
                          vk_stream_t stream);

/* n_steps consecutive agent-steps of dt in one launch, for colonies whose
 * agents do not couple between steps (held externals; BASELINE config 2):
 * every step is vk_step_dopri5 variant 2's, bit for bit, with the state kept
 * in registers between steps.  Step s writes its mean fluxes at flux + s *
 * step_flux, its exchange counts at counts + s * step_counts and its attempts
 * at nsteps + s * step_nsteps (rows of ld, as vk_step_dopri5); conc and
 * h_state hold the end state, status ORs every step's bits.  Needs
 * vk_table_specialize with an agent-per-lane source.  Not a reference
 * interface: the reference steps agents one Delta t at a time
 * (Experiment.update, experiment.py:1351-1450).                            */
int vk_step_dopri5_multi(const vk_table *t, int64_t n_agents, int64_t ld, double dt, int32_t n_steps,
                         const vk_ode_opts *opts, const double *params, double *conc, const double *m2c,
                         double *h_state, double *flux, int64_t step_flux, int64_t *counts,
                         int64_t step_counts, int32_t *status, int32_t *nsteps, int64_t step_nsteps,
                         vk_stream_t stream);

/* Lattice fields: n_fields planes of rows x ny doubles, plane stride
 * field_stride.  Local rows may include halo rows of neighbouring ranks.   */

/* Uniform-plane test over rows [row_lo, row_hi) (diffusion_field.py:401-404).
 * summary[2f] == summary[2f+1] iff plane f holds a single value (both then
 * hold it); otherwise summary = (-inf, +inf) (a NaN plane is non-uniform).
 * Element-wise min of [2f] / max of [2f+1] over ranks gives the global test.
 * A non-uniform plane costs one 16-KiB chunk per probe block.              */
#define VK_UNIFORM_BLOCKS 512   /* scratch: n_fields * VK_UNIFORM_BLOCKS int32 */
int vk_field_uniform(const double *fields, int32_t n_fields, int64_t field_stride,
                     int32_t ny, int32_t row_lo, int32_t row_hi, double *summary,
                     int32_t *scratch, vk_stream_t stream);

/* Substeps [sub_begin, sub_begin+sub_count) of an n_sub-substep diffusion.
 * Substep j reads src(j) and writes dst(j):
 *   src(0) = field, src(j) = work[(j-1)&1]; dst(j) = work[j&1] except the
 *   last substep, which writes field = field + (new - field).
 * Owned rows are [row_lo, row_hi).  Within the call, substep j computes rows
 * [max(lo_min, row_lo-g), min(hi_max, row_hi+g)) with
 * g = sub_begin+sub_count-1-j (halo shrinking); rows lo_min and hi_max-1 are
 * reflected (Neumann) if they are global edges (edge_top/edge_bot != 0).
 * coeff_dt = (D/(dx*dy)) * 0.01.  uniform (nullable, a vk_field_uniform summary)
 * skips uniform planes.                                                      */
int vk_diffuse(double *field, double *work0, double *work1, int32_t n_fields,
               int64_t field_stride, int32_t ny, int32_t row_lo, int32_t row_hi,
               int32_t lo_min, int32_t hi_max, int32_t edge_top, int32_t edge_bot,
               int32_t sub_begin, int32_t sub_count, int32_t n_sub, double coeff_dt,
               const double *uniform, vk_stream_t stream);

/* vk_diffuse for one part of a row band's block (multi-GPU C4), so that the
 * halo exchange can run while the band computes what does not need it:
 *   VK_PART_INTERIOR  the first m = interior_passes passes of the block on the
 *                     rows whose inputs at the block's start are all owned
 *                     (10 (p+1) rows in from each side with halo rows, pass p);
 *   VK_PART_EDGES     the rest of those m passes (the rows next to the halo),
 *                     then the block's remaining passes whole;
 *   VK_PART_ALL       = vk_diffuse.
 * interior_passes <= 0 or > the block's passes means all of them.  INTERIOR
 * then EDGES (the halo in place before EDGES) equals vk_diffuse bit for bit.
 * Only the 10-deep plan (vk_set_stencil_depth(10), a block of 10 k substeps)
 * of a band of more than 2 * sub_count owned rows splits; otherwise
 * VK_ERR_LIMIT (nothing launched).  Replaces the same reference call as
 * vk_diffuse (diffusion_field.py:385-407).                                 */
enum { VK_PART_ALL = 0, VK_PART_INTERIOR = 1, VK_PART_EDGES = 2 };
int vk_diffuse_part(double *field, double *work0, double *work1, int32_t n_fields,
                    int64_t field_stride, int32_t ny, int32_t row_lo, int32_t row_hi,
                    int32_t lo_min, int32_t hi_max, int32_t edge_top, int32_t edge_bot,
                    int32_t sub_begin, int32_t sub_count, int32_t n_sub, double coeff_dt,
                    const double *uniform, int32_t part, int32_t interior_passes,
                    vk_stream_t stream);

/* As vk_diffuse for a call that ends at the last substep, except that the
 * last substep writes delta = new - field into `delta` (same layout; zero on
 * uniform planes) and leaves `field` as it was: DiffusionField.next_update's
 * delta (diffusion_field.py:385-394), for an accumulate updater that applies
 * it later (multi-rate schedules, lens_amd.process.BatchedDiffusionField).  */
int vk_diffuse_delta(double *field, double *work0, double *work1, double *delta, int32_t n_fields,
                     int64_t field_stride, int32_t ny, int32_t row_lo, int32_t row_hi, int32_t lo_min,
                     int32_t hi_max, int32_t edge_top, int32_t edge_bot, int32_t sub_begin,
                     int32_t sub_count, int32_t n_sub, double coeff_dt, const double *uniform,
                     vk_stream_t stream);

/* One whole-plane step of n_sub substeps (rows [0, rows), both edges
 * reflected) with the agent coupling carried by its passes -- one launch per
 * pass instead of vk_gather + the passes + vk_exchange_sorted, same results:
 *   - the first pass, before it changes anything, sets
 *       conc[gather_row[f]*conc_ld + a] = plane f at bin_lin[a]   (vk_gather)
 *   - the final pass, after writing plane f, adds
 *       counts[count_row[f]*counts_ld + a] / binvol_avogadro * 1000
 *     for the agents of each bin in agent order             (vk_exchange_sorted)
 * gather_row / count_row: host arrays of n_fields rows (-1 = none).  Agents
 * must be stored in bin order (bin_lin ascending, Colony.sort_by_bin), and
 * seg[r*nseg + s] (nseg = (ny+15)/16) = the first agent whose bin_lin >= r*ny + 16 s.
 * Uniform planes (the vk_field_uniform summary in `uniform`, nullable) keep
 * their values and still gather and exchange.  Returns VK_ERR_LIMIT and launches
 * nothing unless the step is planned as two or more pair-sum passes (the
 * tolerance mode, vk_set_stencil_mode(1), with kernel variants 20 / 70 and pass
 * depths 3..11; n_fields <= 8): the caller then runs the three steps itself.
 * Not a reference interface: DiffusionField.next_update (diffusion_field.py:
 * 362-407) and the agents' exchange updates (registry.py:149-183) fused.     */
int vk_diffuse_coupled(double *field, double *work0, double *work1, int32_t n_fields,
                       int64_t field_stride, int32_t ny, int32_t rows, int32_t n_sub, double coeff_dt,
                       const double *uniform, const int32_t *bin_lin, const int32_t *seg, int32_t nseg,
                       int64_t n_agents, const int32_t *gather_row, double *conc, int64_t conc_ld,
                       const int32_t *count_row, const int64_t *counts, int64_t counts_ld,
                       double binvol_avogadro, vk_stream_t stream);

/* The passes that vk_diffuse_part (part, interior_passes; VK_PART_ALL = vk_diffuse)
 * would launch for this geometry under the current vk_set_stencil_* settings, in
 * launch order; host only, launches nothing.  coupled != 0: vk_diffuse_coupled's
 * whole-plane step instead (row_lo = lo_min = sub_begin = 0, row_hi = hi_max = rows,
 * both edges, sub_count = n_sub, VK_PART_ALL), without or with agents.  Writes
 * min(*n_passes, capacity) passes to `out` (nullable when capacity = 0) and the
 * plan's length to *n_passes.  Returns VK_OK, VK_ERR_ARG for a geometry the call
 * would refuse, or VK_ERR_LIMIT (*n_passes = 0) where it has no plan: a part of
 * a block that does not split, a coupled step of fewer than two fused passes.
 * A pass of k substeps reads rows [in_lo, in_hi) of buffer src and writes rows
 * [lo, hi) of buffer dst, without [gap_lo, gap_hi) if gap_lo >= 0; f0: it is
 * handed the step-start field as base; couple: bit 0 = it gathers first, bit 1 =
 * it applies the exchange last; copy_back: the owned rows of work0 are copied to
 * the field after it.  Not a reference interface: the launch list of the same
 * reference call as vk_diffuse (diffusion_field.py:385-407).                 */
enum { VK_BUF_FIELD = 0, VK_BUF_WORK0 = 1, VK_BUF_WORK1 = 2 };
enum { VK_PASS_SINGLE = 0, VK_PASS_WL3, VK_PASS_WL6, VK_PASS_WL6NT, VK_PASS_PS, VK_PASS_PS10,
       VK_PASS_PS10_ALIGNED, VK_PASS_PS10_STRIPS, VK_PASS_SP };
enum { VK_PLAN_COUPLED = 1, VK_PLAN_COUPLED_AGENTS = 2 };
typedef struct vk_pass {
    int32_t k, src, dst, f0;
    int32_t lo, hi, in_lo, in_hi, gap_lo, gap_hi;
    int32_t kernel, couple, copy_back;
} vk_pass;
int vk_diffuse_plan(int32_t row_lo, int32_t row_hi, int32_t lo_min, int32_t hi_max, int32_t edge_top,
                    int32_t edge_bot, int32_t sub_begin, int32_t sub_count, int32_t n_sub, int32_t part,
                    int32_t interior_passes, int32_t coupled, vk_pass *out, int32_t capacity,
                    int32_t *n_passes);

/* vk_diffuse_plan with the lanes of a banded plan (vk_set_stencil_bands): beside
 * each pass, lane[i] = the stream it is launched on (0 = the caller's, 1 = the
 * library's second stream) and after[i] = the index of the pass on the other
 * lane that must have finished before it starts, or -1; passes of one lane run
 * in list order.  The caller's stream waits for lane 1 at the end of the call.
 * An unbanded plan is all lane 0, after -1.  lane / after: capacity entries
 * each, nullable.  Not a reference interface (as vk_diffuse_plan).          */
int vk_diffuse_plan_lanes(int32_t row_lo, int32_t row_hi, int32_t lo_min, int32_t hi_max, int32_t edge_top,
                          int32_t edge_bot, int32_t sub_begin, int32_t sub_count, int32_t n_sub,
                          int32_t part, int32_t interior_passes, int32_t coupled, vk_pass *out,
                          int32_t *lane, int32_t *after, int32_t capacity, int32_t *n_passes);

/* Row bands of a whole-plane step on two streams.  A tolerance-mode step of P
 * 10-deep pair-sum passes over the whole plane (vk_diffuse with rows [0, N),
 * both edges reflected, every substep; not vk_diffuse_coupled) can run each
 * pass as two launches: a top band, rows [0, m_p), on the caller's stream and
 * a bottom band, rows [m_p, N), on a stream the library owns, m_p = top_rows -
 * 10 p.  The top bands then never wait for the bottom bands, and the end of
 * one launch overlaps the start of the next; results are bit-identical.
 * bands: 1 = off, 2 = forced with m_0 = top_rows (a step whose last top band
 * would have fewer than 10 rows, or whose first bottom band none, runs
 * unbanded), 0 = the automatic rule (the default: bands only the shape measured
 * faster banded, DESIGN.md §10 -- a 4096-row plane stepping ten passes of variant
 * 70, with m_0 = 1638).  Returns the previous bands; other values only query
 * (top_rows has no query).  The second stream and its events are created by
 * the first banded call whose stream is not capturing; a captured call before
 * that runs unbanded.  Tuning only.                                         */
int vk_set_stencil_bands(int32_t bands, int32_t top_rows);

/* Maximum substeps fused per HBM pass by vk_diffuse (temporal blocking; odd,
 * 1..15; 1 = one launch per substep; or 10, the default: a block of a multiple
 * of 10 substeps as 10-deep passes -- in the tolerance mode over three buffers
 * when the block ends the step, in the exact mode with the final pass re-reading
 * the step-start field -- and every other call at depth 9).  Odd depths plan
 * each call as the fewest odd-depth passes <= k, as even as possible.  Returns
 * the previous value; other k only query.  Exact mode: bit-identical for every
 * depth.                                                                    */
int vk_set_stencil_depth(int32_t k);

/* Fused-pass kernel variant.  Exact mode: 2 / 3 = wave tile with DPP lane
 * shifts, stage q lagging q rows (two live rows per stage), 3 / 6 rows
 * prefetched; 6 = variant 3 with streaming (non-temporal) stores (the exact
 * mode's kernel for 6 and 20-22).  Tolerance mode: 20 = pair-sum passes,
 * (W+N)+(S+E) with each pair added once and used by two cells, 3 FP64 ops
 * per cell-substep (default); 21 / 22 = 20 with 2 / 6 rows prefetched; 6 =
 * the 4-op FMA form.  Other values are ignored (retired variants 0, 1, 4, 5,
 * 7-16).  rows = output rows per tile (8..4096; 0 = auto from
 * the band height; other values keep the current).  Returns the previous
 * variant.  Tuning only: exact-mode results are bit-identical for every
 * setting; tolerance-mode results stay within 1e-13 of them.               */
int vk_set_stencil_kernel(int32_t variant, int32_t rows);

/* Arithmetic mode of vk_diffuse's fused passes.  0 (default) = bit-identical
 * with the reference's f += coef * scipy.ndimage.convolve(f, LAP, 'reflect')
 * (diffusion_field.py:385-394: summation order N, W, -4C, E, S, two roundings
 * per update, delta-then-accumulate at the end of the step).  1 = tolerance
 * mode: fma(coef, (N+S)+(E+W), (1-4coef)*C) per cell-substep (5 FP64 ops
 * instead of 6) and a final pass that writes the new field without re-reading
 * the step-start field; within ~1e-14 relative of mode 0 over a 100-substep
 * step (tests/test_stencil_modes.py).  Single-substep passes and
 * vk_diffuse_delta stay exact.  Returns the previous mode; other values only
 * query.                                                                   */
int vk_set_stencil_mode(int32_t mode);

/* out[idx] = the device's constant-rate wall clock (s_memrealtime ticks, see
 * vk_wall_clock_khz), written by one lane of a one-wave launch on `stream`.
 * Not a reference interface: the bench stamps segment boundaries inside a
 * replayed HIP graph with it (torch refuses events in graphs on ROCm).     */
int vk_timestamp(uint64_t *out, int32_t idx, vk_stream_t stream);

/* dst[0:n) = src[0:n) as the box's fastest streaming copy (one 16-B element per
 * thread, non-temporal stores): the HBM floor any stencil pass over the same
 * planes has (bench.py copy_floor).  Not a reference interface.  n even, both
 * buffers 16-B aligned.                                                     */
int vk_copy_stream(const double *src, double *dst, int64_t n, vk_stream_t stream);

/* Tick rate of vk_timestamp's clock in kHz (hipDeviceAttributeWallClockRate
 * of the current device); 0 on error.                                       */
int64_t vk_wall_clock_khz(void);

/* dst[map_row[i]*ld + a] = fields[map_field[i]*field_stride + bin_lin[a]]. */
int vk_gather(const double *fields, int64_t field_stride, const int32_t *bin_lin,
              int64_t n_agents, const int32_t *map_field, const int32_t *map_row,
              int32_t n_map, double *dst, int64_t ld, vk_stream_t stream);

/* Deterministic exchange: for each occupied bin occ_bin[b] and each map entry
 * i, field += counts[map_count[i]*ld + a] / binvol_avogadro * 1000 for its
 * agents occ_agent[occ_ptr[b]..occ_ptr[b+1]) in that (agent) order --
 * bit-identical to applying update_field_with_exchange agent by agent.   */
int vk_exchange_sorted(double *fields, int64_t field_stride, const int32_t *occ_bin,
                       const int32_t *occ_ptr, const int32_t *occ_agent, int32_t n_occ,
                       const int64_t *counts, int64_t ld, const int32_t *map_count,
                       const int32_t *map_field, int32_t n_map, double binvol_avogadro,
                       vk_stream_t stream);

/* Order-free exchange with float64 atomics (same sum, any order). */
int vk_exchange_atomic(double *fields, int64_t field_stride, const int32_t *bin_lin,
                       int64_t n_agents, const int64_t *counts, int64_t ld,
                       const int32_t *map_count, const int32_t *map_field, int32_t n_map,
                       double binvol_avogadro, vk_stream_t stream);

/* bin = floor(loc*n/bound) mod n per axis; bin_lin = (ix - row_offset)*ny + iy.
 * loc is [2][ld] (x row then y row).  ix_out (nullable) receives ix.     */
int vk_bin_sites(const double *loc, int64_t n_agents, int64_t ld, int32_t nx, int32_t ny,
                 double bound_x, double bound_y, int32_t row_offset, int32_t *bin_lin,
                 int32_t *ix_out, vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Cell growth, derivers and division
 *
 *   vk_cell_step
 *       replaces, per agent and step, GrowthProtein.next_update
 *       (vivarium/processes/growth_protein.py:88-107) or Growth.next_update
 *       (growth.py:101-107) + DivisionVolume.next_update (division_volume.py:
 *       39-45) -- all from the step-start state -- followed by the derivers
 *       TreeMass (tree_mass.py:10-18) and DeriveGlobals.next_update
 *       (derive_globals.py:131-152) on the updated state.  Writes divide[a].
 *   vk_divide_plan + vk_divide_gather / vk_divide_lineage / vk_divide_locations
 *       replace MetaDivision.next_update (meta_division.py:60-88) and the
 *       `_divide` branch of Store.apply_update (core/experiment.py:664-697)
 *       with its dividers (core/registry.py:197-280): the new agent order is
 *       the survivors in order, then daughters id+'0', id+'1' of each mother
 *       in mother order; mothers are removed.
 *   vk_population_plan
 *       is vk_divide_plan with the `_delete` branch beside it (the mother
 *       machine's outflow, multibody_physics.py:232-250): a removed agent gets
 *       no slot, and a removed mother no daughters.
 * ------------------------------------------------------------------------- */

/* Rows of the per-agent cell array cell[VK_CELL_ROWS][ld] ("global" port). */
enum vk_cell_row {
    VK_CELL_MASS = 0,         /* fg                                  split */
    VK_CELL_VOLUME = 1,       /* fL                                  split */
    VK_CELL_LENGTH = 2,       /* um                                  split */
    VK_CELL_SURFACE_AREA = 3, /* um^2                                split */
    VK_CELL_PROTEIN = 4,      /* counts (float, as the reference)    split */
    VK_CELL_ANGLE = 5,        /* rad (orientation for daughter locations) set */
    VK_CELL_ROWS = 6
};

enum vk_growth_model {
    VK_GROWTH_PROTEIN = 0,  /* GrowthProtein + TreeMass; divide when protein >= divide_protein */
    VK_GROWTH_MASS = 1,     /* Growth (mass*factor); DivisionVolume: divide when volume >= division_volume */
    VK_GROWTH_TREE = 2      /* vk_cell_step_tree only: no growth process; mass = initial_mass + the weighted
                               rows of the count table; DivisionVolume                                  */
};

enum vk_rng {
    VK_RNG_STREAM = 0,      /* uniforms u[a] supplied by the caller in agent order (e.g. numpy's
                               MT19937 stream, which replays the reference exactly)            */
    VK_RNG_PHILOX = 1       /* Philox4x32-10 counter = (step, root, path lo, path hi),
                               key = (seed lo + depth, seed hi): order-independent               */
};

typedef struct vk_cell_params {
    int32_t model;            /* vk_growth_model                                     */
    int32_t rng;              /* vk_rng (VK_GROWTH_PROTEIN only)                     */
    double factor;            /* exp(growth_rate * dt), evaluated by the host        */
    double divide_protein;    /* GrowthProtein: 2 * initial protein                  */
    double division_volume;   /* DivisionVolume threshold (fL)                       */
    double protein_mw;        /* g/mol                                               */
    double avogadro;          /* 1/mol                                               */
    double fg_per_g;          /* g -> fg factor as the reference's units evaluate it */
    double density;           /* g/L                                                 */
    double volume_to_fl;      /* fg*L/g -> fL factor as the reference evaluates it   */
    /* capsule constants of the (colony-wide) width w, r = w/2, evaluated by the host
       exactly as derive_globals.py:20-50 writes them                                 */
    double cap_volume;        /* (4/3)*PI*r**3                                       */
    double cap_area;          /* PI*r**2                                             */
    double two_r;             /* 2*r                                                 */
    double width;             /* w                                                   */
    double sa_const;          /* 3*PI*r**2                                           */
    double sa_lin;            /* 2*PI*r                                              */
    uint64_t seed;            /* VK_RNG_PHILOX                                       */
    uint64_t step;            /* VK_RNG_PHILOX counter word                          */
} vk_cell_params;

/* Lineage (phylogeny id) of agent a: root[a] indexes the caller's root ids,
 * the id string is root id + the depth[a] low bits of path[a], MSB first.   */

/* Growth process + derivers for agents [0, n).  u: [ld] uniforms (VK_RNG_STREAM)
 * or NULL; root/depth/path: lineage (VK_RNG_PHILOX) or NULL.  cell rows and
 * mmol_to_counts are updated in place; divide[a] = 0/1.                     */
int vk_cell_step(const vk_cell_params *p, int64_t n_agents, int64_t ld, double *cell,
                 double *mmol_to_counts, const double *u, const int32_t *root,
                 const int32_t *depth, const uint64_t *path, int32_t *divide,
                 vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * vk_cell_step_tree: vk_cell_step with TreeMass over a count table
 *
 * Stands where the reference runs TreeMass (tree_mass.py:10-18, 55-64) over a compartment
 * whose Translation and Complexation ports hang an `mw` property on their proteins, complexes
 * and transcripts (translation.py:347-400, complexation.py:84-97): mass = initial_mass + the
 * sum over every node with `mw` of mw * (count / N_A), then DeriveGlobals on it.
 *
 * counts: the colony's int32 table [n_rows][ld_counts].  rows / weights: DEVICE arrays of
 * n_weighted entries (0 <= n_weighted <= VK_TREE_MAX_WEIGHTED), rows strictly ascending in
 * [0, n_rows), weights in g/mol.  initial_mass: [ld] fg, VK_GROWTH_TREE only.
 *
 * Per agent a, FP64 without contraction:
 *   VK_GROWTH_PROTEIN  growth, the draw, the divide flag and the new protein pn exactly as in
 *                      vk_cell_step; m = 0.0 + (protein_mw * (pn / avogadro)) * fg_per_g.
 *   VK_GROWTH_TREE     div = (step-start volume >= division_volume); m = initial_mass[a]; the
 *                      protein row is not touched.
 *   both               for k = 0 .. n_weighted - 1 in that order:
 *                        m = m + (weights[k] * ((double) counts[rows[k] * ld_counts + a] / avogadro)) * fg_per_g
 *                      then vk_cell_step's deriver tail on m (mass, volume, mmol_to_counts,
 *                      length, surface area) and divide[a] = div.
 *   VK_GROWTH_MASS     is refused (VK_ERR_ARG): Growth writes the mass itself.
 * With n_weighted == 0 and VK_GROWTH_PROTEIN the output is vk_cell_step's bit for bit.
 *
 * The per-node expression is calculate_mass with the g -> fg factor where pint applies it (the
 * protein node of vk_cell_step, pinned by the colony_metrics fixture).  THE ENGINE'S OWN: the
 * ORDER of the fold -- the aggregate protein first, then the table rows ascending.  The
 * reference folds in its Store's depth-first dict order, which is not reproduced (pint and the
 * reference's core do not import here); FP64 addition does not commute bit for bit, so the
 * last bits of a mass may differ from the reference's.  UNVERIFIED against the reference for
 * the same reason: pint's conversion bits for the table's nodes.
 *
 * Bad arguments return VK_ERR_ARG and launch nothing: a null pointer the model needs, n_weighted
 * outside 0..VK_TREE_MAX_WEIGHTED or above n_rows, ld < n, ld_counts < n, VK_GROWTH_MASS or an
 * unknown model or rng.  rows[] lives on the device and no call reads it back: the HOST SIDE
 * validates it once, when it uploads it (lens_amd.cells.TreeWeights refuses a row out of range
 * or not strictly ascending before anything is launched).  The C function trusts that; the
 * kernel still reads nothing outside the table (a row outside [0, n_rows) counts as 0).
 * One agent per lane, 256 lanes per workgroup; no LDS, no scratch, no atomics, no host read.
 * ------------------------------------------------------------------------- */
#define VK_TREE_MAX_WEIGHTED 256

int vk_cell_step_tree(const vk_cell_params *p, int64_t n_agents, int64_t ld, double *cell,
                      double *mmol_to_counts, const double *u, const int32_t *root,
                      const int32_t *depth, const uint64_t *path, int32_t *divide,
                      const int32_t *counts, int64_t ld_counts, int32_t n_rows,
                      const int32_t *rows, const double *weights, int32_t n_weighted,
                      const double *initial_mass, vk_stream_t stream);

/* Division plan: src_index[j] = source agent of new slot j, kind[j] = -1 for a
 * survivor, 0 / 1 for daughter 0 / 1 (j < n_agents + n_divide).  n_out: one
 * device int64 (new agent count).  scratch: >= vk_divide_scratch_bytes(n).
 * The new count must fit the destination capacity the caller then uses.    */
int64_t vk_divide_scratch_bytes(int64_t n_agents);
int vk_divide_plan(const int32_t *divide, int64_t n_agents, int32_t *src_index, int32_t *kind,
                   int64_t *n_out, void *scratch, vk_stream_t stream);

/* Population plan: division and removal in one stable compaction, in the shape
 * of vk_divide_plan's output (vk_divide_gather / _lineage / _locations take
 * it).  Slots [0, n_keep): every agent with !remove && !divide, in agent order,
 * kind -1; then two slots, kind 0 and 1, for every agent with divide &&
 * !remove, in agent order.  A removed agent appears nowhere, whether or not it
 * divides.  n_out = n - removed + kept mothers (may be < n, may be 0).  Either
 * flag array may be NULL (all zero); with remove NULL the result is
 * vk_divide_plan's bit for bit.  src_index and kind: n_out <= 2 n elements.
 * scratch: >= vk_population_scratch_bytes(n).  No atomics, no host read.     */
int64_t vk_population_scratch_bytes(int64_t n_agents);
int vk_population_plan(const int32_t *divide, const int32_t *remove, int64_t n_agents,
                       int32_t *src_index, int32_t *kind, int64_t *n_out, void *scratch,
                       vk_stream_t stream);

enum vk_divider {
    VK_DIVIDE_SET = 0,     /* both daughters copy the mother's value (no divider)  */
    VK_DIVIDE_SPLIT = 1,   /* float64 halves (registry.py divide_split, floats)     */
    VK_DIVIDE_ZERO = 2     /* daughters get 0 (divide flags: meta_division.py:21)   */
};

/* dst[r*ld_dst + j] = divider(src[r*ld_src + src_index[j]]) for rows [0, rows),
 * slots [0, n_out); elem_bytes 4 or 8 (SPLIT: 8 = float64 only).            */
int vk_divide_gather(int64_t n_out, const int32_t *src_index, const int32_t *kind,
                     const void *src, int64_t ld_src, void *dst, int64_t ld_dst, int32_t rows,
                     int32_t elem_bytes, int32_t divider, vk_stream_t stream);

/* Lineage divider (daughter_phylogeny_id, meta_division.py:15-18): daughter k
 * of (root, depth, path) is (root, depth+1, path*2+k).  Sets *overflow (device
 * int32, nullable) when a lineage would exceed 64 generations.              */
int vk_divide_lineage(int64_t n_out, const int32_t *src_index, const int32_t *kind,
                      const int32_t *root_src, const int32_t *depth_src, const uint64_t *path_src,
                      int32_t *root_dst, int32_t *depth_dst, uint64_t *path_dst,
                      int32_t *overflow, vk_stream_t stream);

/* daughter_locations (multibody_physics.py:77-87): daughter k of a mother at
 * (x, y) with length L and angle t sits at (x + L*q*cos t, y + L*q*sin t),
 * q = -0.25 / +0.25.  loc_* are [2][ld] (x row, y row); the mother's length
 * and angle are read from the gathered cell rows (length already split).    */
int vk_divide_locations(int64_t n_out, const int32_t *src_index, const int32_t *kind,
                        const double *loc_src, int64_t ld_src, double *loc_dst, int64_t ld_dst,
                        const double *cell_dst, vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Kremling 2007 sugar transport: the reference's only odeint
 * call, Transport.next_update (vivarium/processes/Kremling2007_transport.py:
 * 218-427).  DEFAULT_PARAMETERS (:19-70) in this field order; units as the
 * reference (time in hours).
 * ------------------------------------------------------------------------- */
typedef struct vk_kremling_params {
    double k1, k2, k3, K1, K2, K3, kd, m, n, x0, kg6p, Kg6p, kptsup, Kglc, Keiiap, klac, Km_lac,
        Kieiia, kgly, kpyk, kpdh, kpts, km_pts, mw1, mw2, mw3, Y1_sim, Y2_sim, Y3_sim, K, kb, ksyn,
        KI;
} vk_kremling_params;

/* state[15][ld]: mass, UHPT, LACZ, PTSG, G6P, PEP, PYR, XP, GLC[e], G6P[e],
 * LCTS[e], then 4 scratch rows (flux integrals GLCpts, PPS, PYK, glc__D_e).
 * Integrates over the reference's grid t_i = i*grid_h (hours), i <
 * n_grid (np.arange(0, dt/3600, 0.01/3600): 100 points, last at 0.99 s),
 * landing on every grid point.  Rows 0-7 := y(t_last); rows 8-10 (external)
 * are left as they were; flux[4][ld] := mean over the grid points of the
 * integrals; counts[3][ld] := int(N_A * V * ((c(t_last) - c(0)) * 1e-3)) for
 * GLC, G6P, LCTS (flux_conversion.millimolar_to_counts), V = volume_fl*1e-15.
 * h_state (nullable, in/out, hours): step-size carry-over.                  */
int vk_kremling_step(const vk_kremling_params *params, int64_t n_agents, int64_t ld,
                     double timestep_h, double grid_h, int32_t n_grid, double rtol, double atol,
                     int32_t max_steps, double *state, const double *volume_fl, double avogadro,
                     double *h_state, double *flux, int64_t *counts, int32_t *status,
                     int32_t *nsteps, vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * ODE gene expression with boolean regulation:
 * ODE_expression.next_update (vivarium/processes/ode_expression.py:265-303)
 * with regulation rules (vivarium/library/regulation_logic.py) compiled by
 * lens_amd/expression.py into postfix programs.
 * ------------------------------------------------------------------------- */
enum vk_expr_op {
    VK_EXPR_CMP_GT = 0,   /* push conc[a] > thr[b]                       */
    VK_EXPR_CMP_LT = 1,   /* push conc[a] < thr[b]                       */
    VK_EXPR_PRESENT = 2,  /* push conc[a] > 0  (a lone numeric operand)  */
    VK_EXPR_CONST = 3,    /* push a != 0                                 */
    VK_EXPR_NOT = 4,
    VK_EXPR_AND = 5,
    VK_EXPR_OR = 6
};

/* All pointers are DEVICE arrays owned by the caller.  Programs are
 * [op, a, b] int32 triples; transcript t's rule is code[prog_ptr[t] ..
 * prog_ptr[t+1]) (empty = unregulated).                                     */
typedef struct vk_expr_table {
    int32_t n_tx, n_tl;
    const int32_t *tx_row;        /* [n_tx] state row of each transcript      */
    const double *tx_rate;        /* [n_tx] transcription rate                */
    const double *tx_deg;         /* [n_tx] degradation rate (0 if absent)    */
    const int32_t *tx_prog_ptr;   /* [n_tx+1]                                 */
    const int32_t *code;          /* [3 * n_instr]                            */
    const double *thr;            /* thresholds                               */
    const int32_t *tl_row;        /* [n_tl] state row of each protein         */
    const int32_t *tl_mrna_row;   /* [n_tl] its transcript's row              */
    const double *tl_rate;        /* [n_tl] translation rate                  */
    const double *tl_deg;         /* [n_tl] degradation rate                  */
    double leak_p;                /* 1 - exp(-(-log(1 - rate)) * dt), host    */
    double leak_magnitude;
} vk_expr_table;

/* update[j][ld] := the reference's {'internal': {...}} values, transcripts
 * (j < n_tx) then proteins, all from the step-start conc; accumulate != 0
 * then adds them into conc (the accumulate updater).  u[n_tx][ld] (nullable):
 * uniforms for the leak draws of inhibited transcripts (NULL: no leak).      */
int vk_expression_step(const vk_expr_table *t, int64_t n_agents, int64_t ld, double dt, double *conc,
                       double *update, const double *u, int32_t accumulate, vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Motile agents: chemotaxis, and re-binning that stays on the device
 *
 *   vk_motility_step
 *       replaces, per agent and inner update, ReceptorCluster.next_update
 *       (vivarium/processes/chemoreceptor_cluster.py:166-209: methylation with
 *       its clamp quirk, piecewise-linear offset energy, MWC free energies,
 *       P_on) and MotorActivity.next_update (vivarium/processes/
 *       coarse_motor.py:134-164: CheY-P, motor bias, switching rates, the
 *       run/tumble switch; thrust and torque as run() / tumble() :177-190 emit
 *       them).  The reference then moves the cell with pymunk (multibody); the
 *       move here -- constant run speed, Gaussian heading jitter while
 *       tumbling, reflecting walls -- is THIS ENGINE'S STAND-IN, not reference
 *       parity.  The agent's new bin is computed with vk_bin_sites' arithmetic.
 *   vk_occupancy_sort + vk_exchange_ordered
 *       replace the host-side occupancy (two sorts, a unique, a host read of
 *       the occupied-bin count) + vk_exchange_sorted after agents move: the
 *       same per-bin sums in the same agent order, bit for bit, with no host
 *       read -- the whole step can be captured into a graph.
 * ------------------------------------------------------------------------- */

/* Rows of the per-agent motility array motil[VK_MOTIL_ROWS][ld]. */
enum vk_motil_row {
    VK_MOTIL_N_METHYL = 0,        /* methyl groups on the receptor cluster (0..8) */
    VK_MOTIL_ACTIVITY = 1,        /* chemoreceptor_activity, P_on                  */
    VK_MOTIL_CHEY_P = 2,          /* CheY_P                                        */
    VK_MOTIL_CCW_MOTOR_BIAS = 3,  /* ccw_motor_bias                                */
    VK_MOTIL_CCW_TO_CW = 4,       /* ccw_to_cw (1/s)                               */
    VK_MOTIL_MOTOR_STATE = 5,     /* motor_state: 0 run, 1 tumble                  */
    VK_MOTIL_ANGLE = 6,           /* heading (rad)                                 */
    VK_MOTIL_THRUST = 7,          /* pN: 250 running, 100 tumbling                 */
    VK_MOTIL_TORQUE = 8,          /* heading change / dt while tumbling, else 0    */
    VK_MOTIL_ROWS = 9
};

/* The reference defaults of both processes, plus this engine's two kinematic
 * constants.  CheR / CheB are in mM as the reference holds them; the kernel
 * uses them in uM as x * 1e3 (the reference converts through pint; that factor
 * is not pinned here).                                                       */
typedef struct vk_motility_params {
    double n_Tar, n_Tsr;                 /* receptors per cluster                     */
    double K_Tar_off, K_Tar_on;          /* mM                                        */
    double K_Tsr_off, K_Tsr_on;          /* mM                                        */
    double k_meth, k_demeth, adapt_rate;
    double CheR, CheB;                   /* mM                                        */
    double k_y, k_s, k_z, gamma_Y, adapt_precision;
    double mb_0, cw_to_ccw, cw_to_ccw_leak;
    double run_speed;                    /* um/s (engine kinematics)                  */
    double tumble_sigma;                 /* rad/s heading jitter (engine kinematics)  */
    uint64_t seed;                       /* Philox key                                */
} vk_motility_params;

/* `substeps` inner updates of dt / substeps for agents [0, n): sense the
 * ligand plane (ligand: [nx][ny], a whole unbanded plane, not written) at the
 * agent's bin, receptor, motor, move; motil / loc ([2][ld]) are updated in
 * place, bin_lin (and ix_out, nullable) receive the final bins.  Draw j of the
 * agent with key k (key[a], or a when key is NULL) at inner update s is
 * Philox(seed, counter (s, k, j, 0)); s = counter[0] + the inner index, and
 * the call then advances counter[0] by substeps (in stream order).          */
int vk_motility_step(const vk_motility_params *p, int64_t n_agents, int64_t ld, double dt,
                     int32_t substeps, double *motil, double *loc, const int64_t *key,
                     const double *ligand, int32_t nx, int32_t ny, double bound_x, double bound_y,
                     uint64_t *counter, int32_t *bin_lin, int32_t *ix_out, vk_stream_t stream);

/* The multi-flagellar motor: FlagellaActivity.next_update (vivarium/processes/
 * flagella_activity.py:135-261; Mears et al. 2014, Sneddon et al. 2012) in the
 * place of MotorActivity -- up to 32 flagella per agent that switch between CCW
 * and CW on their own, CheY-P as an Ornstein-Uhlenbeck process, a tumble when
 * any flagellum turns CW, thrust proportional to the flagella count and the
 * proton motive force.  Sense, receptor and move are vk_motility_step's, with
 * speed = run_speed * thrust / 250.                                          */

/* Rows of the per-agent FP64 flagella array flag[VK_FLAG_ROWS][ld]. */
enum vk_flag_row {
    VK_FLAG_CHEY = 0,             /* CheY (uM)                                     */
    VK_FLAG_CHEY_P = 1,           /* CheY_P (uM)                                   */
    VK_FLAG_CW_BIAS = 2,          /* cw_bias: emitted, read by nothing             */
    VK_FLAG_MOTILE_STATE = 3,     /* motile_state: -1 run, 0 none, 1 tumble        */
    VK_FLAG_PMF = 4,              /* proton motive force (mV): set by the user     */
    VK_FLAG_ROWS = 5
};

/* Rows of the per-agent int32 flagella array flag_int[VK_FLAGI_ROWS][ld]. */
enum vk_flagi_row {
    VK_FLAGI_TARGET = 0,          /* n_flagella wanted (used clamped into [0, 32]) */
    VK_FLAGI_HAVE = 1,            /* flagella the agent has                        */
    VK_FLAGI_MASK = 2,            /* bit i set: flagellum i turns CW; bits >= have are 0 */
    VK_FLAGI_ROWS = 3
};

/* FlagellaActivity.defaults, the parameters next_update reads. */
typedef struct vk_flagella_params {
    double YP_ss, sigma2_Y, tau;         /* CheY-P fluctuations: uM, uM^2, s          */
    double K_d, H;                       /* CW bias Hill curve                        */
    double omega, g_0, g_1, K_D;         /* a flagellum's switch                      */
    double flagellum_thrust;             /* pN per flagellum                          */
    double tumble_scaling, run_scaling;  /* 1 / mV                                    */
} vk_flagella_params;

/* As vk_motility_step (same counter, keys, bins; p supplies the receptor, the
 * kinematic constants and the seed), with the flagella motor: motil's n_methyl,
 * activity, motor_state (1 tumbling, else 0), angle, thrust and torque rows are
 * written, its coarse-motor rows (CheY_P, ccw_motor_bias, ccw_to_cw) are not
 * touched; flag and flag_int ([rows][ld]) are updated in place except PMF and
 * target, which are read.  The Philox paths are listed in vk_flagella.hip.   */
int vk_flagella_step(const vk_motility_params *p, const vk_flagella_params *f, int64_t n_agents,
                     int64_t ld, double dt, int32_t substeps, double *motil, double *flag,
                     int32_t *flag_int, double *loc, const int64_t *key, const double *ligand,
                     int32_t nx, int32_t ny, double bound_x, double bound_y, uint64_t *counter,
                     int32_t *bin_lin, int32_t *ix_out, vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Static fields: analytic gradients (the reference's chemotaxis experiment runs
 * on these, not on a diffusing lattice)
 *
 *   vk_gradient_fill
 *       replaces make_gradient (vivarium/processes/diffusion_field.py:42-206):
 *       the initial planes of a lattice, evaluated at the middle of every bin.
 *   vk_static_gather
 *       replaces StaticField.next_update / get_concentration (vivarium/
 *       processes/static_field.py:79-119): the field at every agent's own
 *       continuous location.
 *   vk_motility_step_static, vk_flagella_step_static
 *       the motile steps with that field sensed at the agent's position at every
 *       inner update instead of a lattice plane at its bin.
 * All four evaluate one device function in the reference's operation order:
 *   dx = x - cx; dy = y - cy; d = sqrt(dx*dx + dy*dy) / 1000.0   (um -> mm)
 *   uniform p0 | gaussian exp((-(d*d)) / (2.0 * (p0*p0))) | linear p0 + p1 * d |
 *   exponential p1 * pow(p0, d)
 * +, -, x, / and sqrt round as the reference's doubles do; exp and pow are the
 * device library's.  The gaussian has no base factor: its value lies in (0, 1].
 * ------------------------------------------------------------------------- */

enum { VK_GRADIENT_UNIFORM = 0, VK_GRADIENT_GAUSSIAN = 1, VK_GRADIENT_LINEAR = 2, VK_GRADIENT_EXPONENTIAL = 3 };
typedef struct { int32_t type; double cx, cy; double p0, p1; } vk_gradient_spec;
/* uniform: p0 = value.  gaussian: p0 = deviation.  linear: p0 = base, p1 = slope.
   exponential: p0 = base, p1 = scale.  cx, cy are in um: center[i] * bounds[i],
   multiplied on the host in Python doubles as the reference does. */
#define VK_GRADIENT_MAX 8      /* specs passed by value per launch */

/* Every entry point below refuses (VK_ERR_ARG) a spec it would evaluate whose type
 * is unknown, a gaussian with deviation 0 and an exponential with base <= 0.   */

/* planes[f*plane_stride + ix*row_stride + iy] = value of specs[f] at
 * (((ix + 0.5) * bound_x) / nx, ((iy + 0.5) * bound_y) / ny) for f < n_specs
 * (<= VK_GRADIENT_MAX), ix < nx (<= 65535), iy < ny (<= row_stride).  specs is a
 * host array, read during the call.  Nothing else of the planes is written.   */
int vk_gradient_fill(const vk_gradient_spec *specs, int32_t n_specs, double *planes,
                     int64_t plane_stride, int64_t row_stride, int32_t nx, int32_t ny,
                     double bound_x, double bound_y, vk_stream_t stream);

/* conc[row_of[j]*ld_conc + a] = value of specs[field_of[j]] at (loc[a], loc[ld + a])
 * for j < n_map (<= VK_GRADIENT_MAX) and a < n.  specs, field_of (each in [0,
 * VK_GRADIENT_MAX)) and row_of are host arrays, read during the call; loc ([2][ld])
 * and conc are device arrays.  Columns >= n and unmapped rows are not written. */
int vk_static_gather(const vk_gradient_spec *specs, const int32_t *field_of, const int32_t *row_of,
                     int32_t n_map, const double *loc, int64_t ld, int64_t n_agents, double *conc,
                     int64_t ld_conc, vk_stream_t stream);

/* vk_motility_step / vk_flagella_step with an analytic ligand: *ligand (a host
 * struct, read during the call) is evaluated at the agent's position at every
 * inner update -- at the position the previous inner update left, which is where
 * the reference's deriver order puts it.  Everything else (receptor, motor,
 * draws, move, bins, counter) is the same kernel body; nx, ny and the bounds
 * still give the bins that are emitted.                                       */
int vk_motility_step_static(const vk_motility_params *p, int64_t n_agents, int64_t ld, double dt,
                            int32_t substeps, double *motil, double *loc, const int64_t *key,
                            const vk_gradient_spec *ligand, int32_t nx, int32_t ny, double bound_x,
                            double bound_y, uint64_t *counter, int32_t *bin_lin, int32_t *ix_out,
                            vk_stream_t stream);
int vk_flagella_step_static(const vk_motility_params *p, const vk_flagella_params *f, int64_t n_agents,
                            int64_t ld, double dt, int32_t substeps, double *motil, double *flag,
                            int32_t *flag_int, double *loc, const int64_t *key,
                            const vk_gradient_spec *ligand, int32_t nx, int32_t ny, double bound_x,
                            double bound_y, uint64_t *counter, int32_t *bin_lin, int32_t *ix_out,
                            vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Motile agents that grow and divide (the reference's ChemotaxisODEExpressionFlagella,
 * vivarium/compartments/chemotaxis_flagella.py:94-173)
 *
 *   vk_flagella_counts
 *       replaces the counts deriver of ODE_expression for the flagella protein
 *       (vivarium/processes/derive_counts.py:42-51: counts = int(concentration *
 *       mmol_to_counts)), whose result FlagellaActivity reads as n_flagella
 *       (flagella_activity.py:138,155).  It runs after the expression update and
 *       before DeriveGlobals (Generator.generate, core/process.py:75-103,179-182:
 *       generated derivers first, in process order), so mmol_to_counts is the
 *       value the previous step's DeriveGlobals left.
 *   vk_divide_flagella
 *       replaces, for flag_int and the agents' motility keys, the `_divide` branch
 *       of Store.apply_update (core/experiment.py:664-697) with divide_split on the
 *       int count (core/registry.py:205-227) and the flagella's split_dict
 *       (flagella_activity.py:126-131, core/registry.py:246-262) -- either as
 *       declared, or as deep_merge (library/dict_utils.py:51-66) leaves it: the
 *       daughters start as deep copies of the mother and merging a divided dict into
 *       a copy only adds or overwrites keys, so both keep every flagellum.
 * ------------------------------------------------------------------------- */

/* target[a] = clamp(trunc(conc[a] * m2c[a]), 0, 32) for a < n: one FP64 multiply,
 * truncated toward zero like Python's int(); NaN and negative products give 0.
 * flags: one device int32, set to 1 (never cleared) when any product lay outside
 * [0, 33) -- the reference would fail there, or grow past the 32 flagella of the
 * mask.  No host synchronisation; the launch is the same inside a captured graph. */
int vk_flagella_counts(int64_t n_agents, const double *conc, const double *mmol_to_counts,
                       int32_t *target, int32_t *flags, vk_stream_t stream);

enum vk_flagella_divider {
    VK_FLAGELLA_MERGED = 0,      /* what the reference's Store does: both daughters keep every
                                    flagellum of the mother (have and mask copied); the split
                                    target makes each shed the surplus in her first update   */
    VK_FLAGELLA_SPLIT_DICT = 1   /* the declared divider: with h = have / 2, daughter 0 gets the
                                    flagella [h, have) (have - h, mask >> h), daughter 1 the
                                    flagella [0, h) (h, mask & ((1 << h) - 1))               */
};

/* Mixed into the seed of vk_divide_flagella's draw (seed ^ this). */
#define VK_DIVIDE_FLAGELLA_DOMAIN 0x666c6167656c6c61ULL

/* The motile state's dividers over a plan of vk_divide_plan (slots [0, n_keep) are the
 * survivors, the daughters follow; n_src agents in the source arrays).  flag_int_dst
 * [VK_FLAGI_ROWS][ld_dst] and key_dst [ld_dst] receive, per slot j with a = src_index[j]:
 *   survivor    the three rows and key_src[a], copied;
 *   daughter k  key_base + (j - n_keep), a key no agent has had (the caller advances
 *               key_base by n_out - n_keep; the last key must not pass 2^31 - 1, the motility
 *               kernels put it into a 32-bit counter word);
 *               target: half = t / 2, and the odd one (t - 2 half) to daughter 0 when u < 0.5,
 *               else to daughter 1; u is one draw per mother, the same for both daughters:
 *               Philox(key (seed ^ VK_DIVIDE_FLAGELLA_DOMAIN) lo + depth, hi; counter (step,
 *               root, path lo, path hi)) of the MOTHER's lineage root_src / depth_src /
 *               path_src -- vk_cell_step's layout under another key, so it coincides neither
 *               with the growth draw nor with a draw of the motility kernels (counter (s, k,
 *               j, 0), key seed);
 *               have, mask: by `mode` (vk_flagella_divider).
 * flag_int_src and flag_int_dst may both be NULL (the coarse motor has no flagella): keys
 * only.  No atomics, no host synchronisation.                                       */
int vk_divide_flagella(int64_t n_out, int64_t n_keep, int64_t n_src, const int32_t *src_index,
                       const int32_t *kind, const int32_t *flag_int_src, int64_t ld_src,
                       const int64_t *key_src, const int32_t *root_src, const int32_t *depth_src,
                       const uint64_t *path_src, int32_t *flag_int_dst, int64_t ld_dst,
                       int64_t *key_dst, int32_t mode, uint64_t seed, uint64_t step, int64_t key_base,
                       vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Stochastic mass-action kinetics: the Gillespie direct method per agent
 *
 *   vk_ssa_step
 *       stands where the reference calls arrow.StochasticSystem.evolve (Complexation,
 *       vivarium/processes/complexation.py:74,120; the flagella complexes of
 *       data/chromosomes/flagella_chromosome.py:371-453).  NOT bit-compatible with arrow:
 *       the algorithm is the direct method in this library's own arithmetic and its own
 *       Philox draws, stated below and restated in NumPy by tests/ssa_ref.py.
 *   vk_ssa_propensities
 *       the propensities alone, as vk_ssa_step evaluates them.
 *   vk_divide_counts
 *       the `_divide` branch of Store.apply_update for int counts with divide_split
 *       (core/registry.py:205-227), one coin per (mother, species).
 *   vk_ssa_flagella_target
 *       the twin of vk_flagella_counts for an int source: FlagellaActivity reads the
 *       'flagella' complex as internal_counts.flagella (chemotaxis_flagella.py:176-291).
 * ------------------------------------------------------------------------- */

#define VK_SSA_MAX_SPECIES 64
#define VK_SSA_MAX_REACTIONS 32
#define VK_SSA_MAX_ORDER 255

/* Mixed into the seed of vk_ssa_step's draws and of vk_divide_counts' coins (seed ^ this). */
#define VK_SSA_DOMAIN 0x7373615f73746570ULL
#define VK_SSA_DIVIDE_DOMAIN 0x7373615f64697669ULL
/* A count table may hold further rows below the network's n_species that no reaction names
 * (passive rows: vk_ssa_step and vk_ssa_propensities read and stage rows < n_species only).  The
 * host divides them in chunks of at most 64 rows by vk_divide_counts launches of their own, chunk
 * c under the seed (seed ^ VK_SSA_PASSIVE_DOMAIN) + c, with the same key_base: the daughters'
 * keys are written again with equal values. */
#define VK_SSA_PASSIVE_DOMAIN 0x7373615f70617373ULL

enum vk_ssa_status {            /* bits OR-ed into the caller's status[] by vk_ssa_step (never cleared) */
    VK_SSA_MAX_EVENTS = 1,      /* the agent fired max_events events and was stopped there         */
    VK_SSA_NONFINITE = 2,       /* the summed propensity was inf or NaN: stopped before the event  */
    VK_SSA_OVERFLOW = 4,        /* an event would take a count past INT32_MAX: not fired, stopped  */
    VK_SSA_BAD_KEY = 8          /* the agent's key lies outside [0, 2^31): not stepped             */
};

/* A network of n_species <= 64 species and n_reactions <= 32 reactions.  Every pointer is a
 * DEVICE array the caller owns (the struct itself is read on the host at the call):
 *   react_*   CSR of the reactants: reaction r consumes react_order[j] >= 1 (<= max_order)
 *             molecules of species react_species[j] for j in [react_ptr[r], react_ptr[r+1]),
 *             species ascending;
 *   stoich_*  CSR of the whole stoichiometry: an event of r adds stoich_delta[j] to species
 *             stoich_species[j];
 *   rates     [n_reactions]; inv [n_inv]: inv[i] = 1.0 / (i + 1) in FP64, n_inv >= max_order. */
typedef struct {
    int32_t n_species, n_reactions, max_order, n_inv;
    const int32_t *react_ptr, *react_species, *react_order;
    const int32_t *stoich_ptr, *stoich_species, *stoich_delta;
    const double *rates, *inv;
} vk_ssa_net;

/* One step of `duration` for agents [0, n) of counts [n_species][ld] (int32), one agent per
 * lane, each on her own clock t = 0:
 *   a_r    = rates[r] * prod C(x_s, k) over r's reactants in CSR order (no reactants: rates[r]);
 *            C(n, k) = 0 if n < k, else c = 1.0; for i < k: c = c * (double)(n - i); c = c * inv[i]
 *            (two FP64 multiplies per factor, no divide, no fused multiply-add);
 *   total  = a_0 + a_1 + ... in reaction order, cum_r the running sums;
 *   total == 0: the agent is done, no draw is consumed; total not finite: VK_SSA_NONFINITE, done;
 *   draw e = 0, 1, ... of the step: one Philox4x32-10 block, key (seed ^ VK_SSA_DOMAIN), counter
 *            (step, (int32) keys[a], e, 0); u1 from words 0 and 1, u2 from words 2 and 3 (the
 *            (w >> 5, w >> 6) construction of the other kernels);
 *   tau    = -log(1.0 - u1) / total; t + tau > duration: done, the event is discarded and
 *            nothing carries into the next step; else t = t + tau;
 *   fire   the first reaction q with cum_q > u2 * total (x += stoichiometry of q, one more
 *            event), unless a count would pass INT32_MAX: VK_SSA_OVERFLOW, not fired, done;
 *   the agent stops with VK_SSA_MAX_EVENTS once she has fired max_events (>= 1) events.
 * step_counter: one device int64, the `step` word of this launch; the launch sequence then
 * advances it by one (also for n = 0), so a captured graph replays successive steps.
 * events_out [ld]: the events each agent fired.  status [ld]: vk_ssa_status bits are OR-ed in.
 * An agent that fired nothing has no count written.  Draws depend on (seed, step, key, e)
 * alone.  No atomics, no host synchronisation, no wait between workgroups.  */
int vk_ssa_step(const vk_ssa_net *net, int64_t n_agents, int64_t ld, double duration, int32_t *counts,
                const int64_t *keys, uint64_t seed, int64_t *step_counter, int32_t max_events,
                int32_t *events_out, int32_t *status, vk_stream_t stream);

/* out[r * ld + a] = a_r of agent a < n exactly as vk_ssa_step evaluates it from counts
 * [n_species][ld] (the same device function).                                      */
int vk_ssa_propensities(const vk_ssa_net *net, int64_t n_agents, int64_t ld, const int32_t *counts,
                        double *out, vk_stream_t stream);

/* divide_split on n_species rows of int32 counts over a plan of vk_divide_plan or
 * vk_population_plan (slots [0, n_keep) are the survivors, the daughters follow; n_src agents
 * in the source arrays).  Per slot j with a = src_index[j]:
 *   survivor    her counts and key_src[a], copied;
 *   daughter k  key_base + (j - n_keep) (the caller advances key_base by n_out - n_keep; the
 *               last key must not pass 2^31 - 1); of each species s: half = x / 2 (toward zero),
 *               and the odd one (x - 2 half) to daughter 0 when u < 0.5, else to daughter 1, with
 *               u = Philox(key (seed ^ VK_SSA_DIVIDE_DOMAIN); counter (step, (int32) key_src[a],
 *               s, 0)): one coin per (mother, species), the same for both daughters.       */
int vk_divide_counts(int64_t n_out, int64_t n_keep, int64_t n_src, const int32_t *src_index,
                     const int32_t *kind, const int32_t *counts_src, int64_t ld_src,
                     const int64_t *key_src, int32_t *counts_dst, int64_t ld_dst, int64_t *key_dst,
                     int32_t n_species, uint64_t seed, uint64_t step, int64_t key_base,
                     vk_stream_t stream);

/* target[a] = clamp(counts_row[a], 0, 32) for a < n.  flags: one device int32, set to 1 (never
 * cleared) when a count was negative or above 32: the motor's mask holds 32 flagella.  */
int vk_ssa_flagella_target(int64_t n_agents, const int32_t *counts_row, int32_t *target,
                           int32_t *flags, vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Stochastic translation: ribosomes elongate on a bounded, ordered per-agent list
 *
 *   vk_translation_step
 *       stands where the reference runs Translation.next_update
 *       (vivarium/processes/translation.py:423-579) with polymerize_step
 *       (vivarium/library/polymerize.py:205-259).  Elongation is the reference's,
 *       operation for operation.  Initiation is the direct method in vk_ssa_step's
 *       arithmetic and Philox draws, NOT arrow's: trajectories agree with the reference
 *       in distribution only.  Restated as per-agent Python loops by
 *       tests/translation_ref.py.
 *   vk_divide_ribosomes
 *       THIS ENGINE'S OWN rule: the reference's `ribosomes` store declares no divider.
 * ------------------------------------------------------------------------- */

#define VK_TL_MAX_SLOTS 128       /* ribosomes per agent: 128 x 64 lanes x 4 B = 32 KiB of LDS   */
#define VK_TL_MAX_TEMPLATES 64    /* unbound[template][lane]: 16 KiB                             */
#define VK_TL_MAX_MONOMERS 24     /* limit[monomer][lane]: 6 KiB; 54 KiB and 260 B, under 64 KiB */
#define VK_TL_MAX_POSITION 0x00ffffff   /* a sequence holds at most 2^24 - 1 residues            */

/* Mixed into the seed of vk_translation_step's draws and of vk_divide_ribosomes' coins. */
#define VK_TL_DOMAIN 0x746c5f5f73746570ULL
#define VK_TL_DIVIDE_DOMAIN 0x746c5f5f64697669ULL

/* One ribosome: (position << 7) | (template << 1) | occluding. */
#define VK_TL_PACK(position, template_index, occluding) \
    ((int32_t)(((uint32_t)(position) << 7) | ((uint32_t)(template_index) << 1) | ((occluding) ? 1u : 0u)))

enum vk_tl_status {             /* bits OR-ed into the caller's status[] (never cleared)              */
    VK_TL_SLOTS_FULL = 1,       /* an initiation found the list at capacity: not fired, the agent
                                   initiates no more this step                                        */
    VK_TL_BAD_KEY = 2,          /* the agent's key lies outside [0, 2^31): not stepped                */
    VK_TL_NONFINITE = 4,        /* the summed propensity was inf or NaN: no more initiation this step */
    VK_TL_OVERFLOW = 8,         /* a count would pass INT32_MAX: see below                            */
    VK_TL_MAX_EVENTS = 16       /* the agent fired max_events initiations: no more this step          */
};

enum vk_tl_release { VK_TL_RELEASE_REFERENCE = 0, VK_TL_RELEASE_TEMPLATE = 1 };

/* The model, the same for every agent.  Every pointer is a DEVICE array the caller owns:
 *   operon_species [n_templates]   row of `counts` that holds the transcript count of template
 *                                  i's operon (templates are in transcript_order);
 *   seq_ptr [n_templates + 1], seq monomer index (< n_monomers) of every residue, the templates'
 *                                  sequences concatenated; the one terminator of template i
 *                                  stands at its length seq_ptr[i + 1] - seq_ptr[i] >= 1;
 *   prod_ptr [n_templates + 1], prod_species   rows of `counts` of the terminator's products;
 *   affinity [n_templates];
 *   interval [n_plan], elongate [n_plan]   the sub-interval plan of the step (below).          */
typedef struct {
    int32_t n_templates, n_monomers, n_species, max_slots;
    int32_t occlusion, release, ribosome_species, n_plan;
    const int32_t *operon_species, *seq_ptr, *prod_ptr, *prod_species, *elongate;
    const uint8_t *seq;
    const double *affinity, *interval;
} vk_tl_model;

/* One step for agents [0, n), one agent per lane.  Per agent: her ribosome list slots
 * [max_slots][ld] (VK_TL_PACK words, entries [0, length[a]) in insertion order), molecules
 * [n_monomers + 2][ld] (the monomers, then ATP, then ADP) and her column of counts
 * [n_species][ld], the table vk_ssa_step steps.
 *
 *   unbound[i] = counts[operon_species[i]] (the reference's gene - bound with bound = 0: no
 *                stored ribosome is 'bound', translation.py:444-450, 519-521);
 *   free = counts[ribosome_species]; limit[m] = molecules[m]; e = 0; events = 0.
 * The plan is the reference's float loop run once on the host (translation.py:478-499, 533):
 *   d = 1 / rate; while time < T: interval = min(d, T - time); elongate = (interval == d);
 *   time += interval.  A trailing partial sub-interval elongates nothing.
 * Per sub-interval k, in this order:
 *   1 substrate   ribosomes = free and unbound[] as they are now, before elongation (:480-483);
 *   2 elongation  if elongate[k], every ribosome in list order (polymerize.py:221-252): with
 *                 m = seq[seq_ptr[t] + p], if limit[m] > 0: limit[m] -= 1, p += 1, and at
 *                 p == length of t the ribosome completes: every product of the terminator gains
 *                 1, free += 1, she leaves the list and the order of the rest is kept.  A
 *                 ribosome whose monomer is exhausted stalls in place; the earlier in the list
 *                 takes the last monomer.  A completion that would take a product or free past
 *                 INT32_MAX is VK_TL_OVERFLOW: it is not made (no monomer taken) and the agent
 *                 does nothing more this step but the books below;
 *   3 initiation  the direct method on the substrate over interval[k], clock t = 0; while
 *                 ribosomes >= 1 (with none nothing binds and no draw is made):
 *                 a_i = (affinity[i] * (double) unbound[i]) * (double) ribosomes, 0 when either
 *                 count is < 1 (vk_ssa_step's a_r for first-order reactants);
 *                 total = a_0 + a_1 + ... in template order, cum_i the running sums;
 *                 total == 0 ends the sub-interval without a draw; total not finite:
 *                 VK_TL_NONFINITE; draw e: one Philox4x32-10 block, key (seed ^ VK_TL_DOMAIN),
 *                 counter (step, (int32) keys[a], e, 0), u1, u2 as vk_ssa_step; e += 1 for
 *                 every draw made, fired or not;
 *                 tau = -log(1.0 - u1) / total; t + tau > interval[k] ends the sub-interval, the
 *                 event is discarded; else t = t + tau and the first q with cum_q > u2 * total
 *                 fires: unbound[q] -= 1, ribosomes -= 1, free -= 1, VK_TL_PACK(0, q, 1) is
 *                 appended (it first elongates in sub-interval k + 1), events += 1; a full list:
 *                 VK_TL_SLOTS_FULL, not fired; events == max_events: VK_TL_MAX_EVENTS;
 *   4 release     every occluding ribosome with p >= occlusion becomes polymerizing and
 *                 unbound[r] += 1, r = 0 (VK_TL_RELEASE_REFERENCE: the reference decrements
 *                 bound[ribosome.template_index], which Translation never sets,
 *                 translation.py:528-531, polymerize.py:43) or r = t (VK_TL_RELEASE_TEMPLATE).
 * Then: counts[ribosome_species] = free; molecules[m] = limit[m]; with used = the sum of the
 * monomers taken, ATP -= 2 used, ADP += 2 used (:552-557; a result outside int32 is clamped with
 * VK_TL_OVERFLOW); the list and its length are stored.  Entries beyond the length keep stale
 * words.  Ribosomes found with t >= n_templates or p >= the template's length stall.
 * step_counter: one device int64, the `step` word; advance != 0 adds one after the launch (also
 * for n = 0), advance == 0 leaves it to the vk_ssa_step that follows on the same counter.
 * events_out [ld]: initiations per agent.  Draws depend on (seed, step, key, e) alone.  No
 * atomics, no host synchronisation, no wait between workgroups.  Bad n, ld, capacity, table
 * sizes or null pointers return VK_ERR_ARG and launch nothing.                          */
int vk_translation_step(const vk_tl_model *model, int64_t n_agents, int64_t ld, int32_t *slots,
                        int32_t *length, int32_t *molecules, int32_t *counts, const int64_t *keys,
                        uint64_t seed, int64_t *step_counter, int32_t advance, int32_t max_events,
                        int32_t *events_out, int32_t *status, vk_stream_t stream);

/* The ribosome lists over a plan of vk_divide_plan or vk_population_plan.  Per slot j with
 * a = src_index[j]: a survivor's list is copied; daughter k takes, in order, every ribosome
 * i < length_src[a] of the mother with (u < 0.5 ? 0 : 1) == k,
 * u = Philox(key (seed ^ VK_TL_DIVIDE_DOMAIN); counter (step, (int32) key_src[a], 0, i)): one
 * coin per (mother, list entry), the same for both daughters.  Entries of the destination
 * beyond the new length are zeroed.  key_src: the mothers' keys BEFORE vk_divide_counts
 * renews them.                                                                         */
int vk_divide_ribosomes(int64_t n_out, int64_t n_src, const int32_t *src_index, const int32_t *kind,
                        const int32_t *slots_src, const int32_t *length_src, int64_t ld_src,
                        const int64_t *key_src, int32_t *slots_dst, int32_t *length_dst,
                        int64_t ld_dst, int32_t max_slots, uint64_t seed, uint64_t step,
                        vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Stochastic transcription: RNA polymerases elongate on the chromosome's promoters
 *
 *   vk_transcription_step
 *       stands where the reference runs Transcription.next_update
 *       (vivarium/processes/transcription.py:370-553) with polymerize_step
 *       (vivarium/library/polymerize.py:205-259), Template.binding_state / terminates_at
 *       (polymerize.py:87-160) and Chromosome.sequences (vivarium/states/chromosome.py:248-254).
 *       The affinity vector, elongation, the read-through rule, unocclusion and the books
 *       (with the reference's ATP quirk) are the reference's, operation for operation.
 *       THE ENGINE'S OWN: initiation is the direct method in vk_ssa_step's arithmetic and
 *       Philox draws, NOT arrow's; the read-through uniform is Philox, not Python's
 *       random.random(); the factor levels are counts / mmol_to_counts taken at the start of
 *       the launch; the process edits the int table in place, in front of translation and the
 *       network.  Trajectories agree with the reference in distribution only.  Restated as
 *       per-agent Python loops by tests/transcription_ref.py.
 *   The RNAP list is divided by vk_divide_ribosomes as it is (it copies packed words and never
 *   looks inside them), under a seed the host mixes with VK_TX_DIVIDE_DOMAIN: THE ENGINE'S OWN
 *   rule, the reference's `rnaps` store declares no divider.
 * ------------------------------------------------------------------------- */

#define VK_TX_MAX_SLOTS 128       /* RNAPs per agent: 128 x 64 lanes x 4 B = 32 KiB of LDS        */
#define VK_TX_MAX_TEMPLATES 64    /* one word per (promoter, lane): 16 KiB                        */
#define VK_TX_MAX_TERMINATORS 4
#define VK_TX_MAX_MONOMERS 4      /* the sequence is held at 2 bits per base                      */
#define VK_TX_MAX_SITES 4         /* binding sites per promoter                                   */
#define VK_TX_MAX_FACTORS 4       /* thresholds per site                                          */
#define VK_TX_MAX_AFFINITIES 1024 /* entries of the dense affinity table, all promoters: 8 KiB    */
#define VK_TX_MAX_POSITION 0x003fffff   /* a template holds at most 2^22 - 1 bases                */

/* Mixed into the seed of vk_transcription_step's draws; the host mixes VK_TX_DIVIDE_DOMAIN into
 * the seed it hands vk_divide_ribosomes for the RNAP lists. */
#define VK_TX_DOMAIN 0x74785f5f73746570ULL
#define VK_TX_DIVIDE_DOMAIN 0x74785f5f64697669ULL

/* One RNAP: (position << 9) | (terminator << 7) | (template << 1) | occluding. */
#define VK_TX_PACK(position, terminator, template_index, occluding)                                    \
    ((int32_t)(((uint32_t)(position) << 9) | ((uint32_t)(terminator) << 7) | ((uint32_t)(template_index) << 1) | \
               ((occluding) ? 1u : 0u)))

enum vk_tx_status {             /* bits OR-ed into the caller's status[] (never cleared)              */
    VK_TX_SLOTS_FULL = 1,       /* an initiation found the list at capacity: not fired, the agent
                                   initiates no more this step                                        */
    VK_TX_BAD_KEY = 2,          /* the agent's key lies outside [0, 2^31): not stepped                */
    VK_TX_NONFINITE = 4,        /* the summed propensity was inf or NaN: no more initiation this step */
    VK_TX_OVERFLOW = 8,         /* a count would pass INT32_MAX: see below                            */
    VK_TX_MAX_EVENTS = 16       /* the agent fired max_events initiations: no more this step          */
};

enum vk_tx_sequence { VK_TX_SEQUENCE_AUTO = 0, VK_TX_SEQUENCE_GLOBAL = 1, VK_TX_SEQUENCE_LDS = 2 };

/* The model, the same for every agent.  Every pointer is a DEVICE array the caller owns; P =
 * n_templates, promoters in promoter order.  Per-terminator arrays have VK_TX_MAX_TERMINATORS
 * entries per promoter (entry 4 p + i is terminator i of promoter p; unused entries are 0):
 *   copy [P]                 the promoter's copy number;
 *   n_term [P]               1..4 terminators;
 *   term_pos [4 P]           the terminator's position RELATIVE to the promoter,
 *                            (terminator.position - promoter.position) * direction: strictly
 *                            increasing, >= 1, the last one the template's length;
 *   term_strength, term_from [4 P]   strength[i] and the reference's strength_from(i), summed on
 *                            the host in the reference's order (polymerize.py:140-144);
 *   prod_ptr [4 P + 1], prod_species   rows of `counts` of each terminator's products;
 *   seq_ptr [P + 1], seq     monomer index (< n_monomers) of every base of the templates'
 *                            RNA sequences, concatenated; seq2 the same at 2 bits per base, 16 to
 *                            a word, base b in bits [2 (b & 15), 2 (b & 15) + 2) of word b >> 4;
 *   site_ptr [P + 1]         the promoter's sites; thr_ptr [sites + 1] each site's thresholds in
 *                            the reference's dict order; thr_species (row of `counts`), thr_value;
 *   aff_ptr [P + 1], affinity [n_affinities]   one dense table per promoter, indexed in mixed
 *                            radix by the site states: index = (..(s_0 r_1 + s_1) r_2 + ..) with
 *                            r_j = 1 + thresholds of site j, state 0 = None, state 1 + i =
 *                            threshold i of the site; keys the reference's dict lacks hold 0.0;
 *   interval [n_plan], elongate [n_plan]   the sub-interval plan of the step (as translation's).
 * sequence: VK_TX_SEQUENCE_LDS stages seq2 in LDS whenever the workgroup's 64 KiB hold it;
 * VK_TX_SEQUENCE_GLOBAL always reads seq from global memory; VK_TX_SEQUENCE_AUTO stages only where
 * that costs no wave of occupancy (the same number of workgroups fits a CU's 160 KiB with and
 * without the staged words): the kernel waits on latency at few waves per CU, and a wave more
 * hides more of it than the LDS read saves.  Same results on every path.                    */
typedef struct {
    int32_t n_templates, n_monomers, n_species, max_slots;
    int32_t occlusion, rnap_species, n_plan, n_affinities;
    int32_t atp_row, adp_row, sequence, n_bases;   /* n_bases = seq_ptr[P] */
    const int32_t *copy, *n_term, *term_pos, *prod_ptr, *prod_species, *seq_ptr, *site_ptr, *thr_ptr,
        *thr_species, *aff_ptr, *elongate;
    const uint8_t *seq;
    const uint32_t *seq2;
    const double *term_strength, *term_from, *thr_value, *affinity, *interval;
} vk_tx_model;

/* One step for agents [0, n), one agent per lane.  Per agent: her RNAP list slots
 * [max_slots][ld] (VK_TX_PACK words, entries [0, length[a]) in insertion order), molecules
 * [adp_row + 1][ld] (the monomers, then ATP where it is no monomer, then ADP), her column of
 * counts [n_species][ld] (the table vk_ssa_step steps) and mmol_to_counts[a].
 *
 * Once, at the start (transcription.py:385-425, polymerize.py:87-138):
 *   level(s) = (double) counts[s] / mmol_to_counts[a] (ENGINE'S OWN: the reference reads
 *              concentrations a deriver left);
 *   state of a site = 1 + the first threshold i in its order with level(thr_species[i]) >=
 *              thr_value[i], else 0 (None); affinity[p] = the promoter's table entry at her
 *              sites' states.  Fixed over the step;
 *   blocked[p] = the stored RNAPs of promoter p that are occluding;
 *   free = counts[rnap_species]; limit[m] = molecules[m]; e = 0; events = 0.
 * Per sub-interval k of the plan, in this order:
 *   1 substrate   rnaps = free and open[p] = copy[p] - blocked[p] as they are now, before
 *                 elongation (:429-432);
 *   2 elongation  if elongate[k], every RNAP in list order, occluding or not (polymerize.py:
 *                 221-252): with m = seq[seq_ptr[t] + position], if limit[m] > 0: limit[m] -= 1,
 *                 position += 1; if the new position is term_pos of her terminator index i: at the
 *                 last terminator she terminates; else one draw e (u1 of its block, e += 1),
 *                 choice = u1 * term_from[i], she terminates iff choice <= term_strength[i], else
 *                 her terminator index becomes i + 1.  A termination adds 1 to every product of
 *                 that terminator and to free, she leaves the list and the order of the rest is
 *                 kept.  An RNAP whose monomer is exhausted stalls in place; the earlier in the
 *                 list takes the last monomer.  A step onto a terminator whose products or free
 *                 stand at INT32_MAX is VK_TX_OVERFLOW: it is not made (no monomer taken, no
 *                 draw) and the agent does nothing more this step but the books below;
 *   3 initiation  the direct method over interval[k], as vk_translation_step's with
 *                 a_p = (affinity[p] * (double) open[p]) * (double) rnaps, 0 when either count
 *                 is < 1; key (seed ^ VK_TX_DOMAIN), counter (step, (int32) keys[a], e, 0); e
 *                 counts EVERY draw of the agent's step, read-through draws included, in the order
 *                 they are made.  A fired p: blocked[p] += 1, rnaps -= 1, free -= 1,
 *                 VK_TX_PACK(0, 0, p, 1) is appended (it first elongates in sub-interval k + 1),
 *                 events += 1; VK_TX_SLOTS_FULL, VK_TX_NONFINITE and VK_TX_MAX_EVENTS as
 *                 translation's bits;
 *   4 unocclusion every occluding RNAP with position >= occlusion becomes polymerizing and
 *                 blocked[her own template] -= 1 (:487-494).
 * Then (the reference's books, :504-516): counts[rnap_species] = free; with used[m] the monomers
 * taken, molecules[m] -= used[m] for every monomer BUT ATP, molecules[atp_row] -= sum of used
 * (the reference overwrites ATP's own entry: not used[ATP] + sum), molecules[adp_row] += sum.
 * Within the step limit[ATP] falls by used[ATP] only, so the stored ATP may go below zero; it is
 * kept so (a result outside int32 is clamped with VK_TX_OVERFLOW).  The list and its length are
 * stored.  RNAPs found with t >= n_templates or position >= the template's length stall.
 * step_counter, advance, events_out (initiations per agent), the draws' dependence on (seed,
 * step, key, e) alone and the argument checks are vk_translation_step's.  No atomics, no host
 * synchronisation, no wait between workgroups.                                            */
int vk_transcription_step(const vk_tx_model *model, int64_t n_agents, int64_t ld, int32_t *slots,
                          int32_t *length, int32_t *molecules, int32_t *counts,
                          const double *mmol_to_counts, const int64_t *keys, uint64_t seed,
                          int64_t *step_counter, int32_t advance, int32_t max_events,
                          int32_t *events_out, int32_t *status, vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * RNA degradation: Michaelis-Menten in the endoRNAse and the transcript, with a carry
 *
 *   vk_rna_degradation_step
 *       stands where the reference runs RnaDegradation.next_update
 *       (vivarium/processes/degradation.py:136-182).  The rate law, its order of evaluation, the
 *       fractional carry from step to step and the books with their signs (ATP RISES by a base
 *       per nucleotide degraded and ADP FALLS, :172-178: the reference subtracts a negative
 *       count) are the reference's.  THE ENGINE'S OWN: the clamp d <= counts[t] (the reference
 *       would let a transcript go negative); the process edits the int table in place after
 *       translation and in front of the network; km in mM is the reference's km * mole / fL by
 *       this host's own factor, not by pint's conversion (not verified: lens_amd/degradation.py).
 *       Restated as per-agent Python loops by tests/degradation_ref.py.
 * ------------------------------------------------------------------------- */

#define VK_DEG_MAX_TRANSCRIPTS 64
#define VK_DEG_MAX_ENZYMES 8      /* their levels are held in registers                           */
#define VK_DEG_MAX_PAIRS 256      /* (enzyme, transcript) pairs with a km                         */
#define VK_DEG_MAX_MONOMERS 4
#define VK_DEG_MAX_LENGTH 0x003fffff   /* bases of a transcript, as VK_TX_MAX_POSITION            */

enum vk_deg_status {            /* bits OR-ed into the caller's status[] (never cleared)              */
    VK_DEG_NONFINITE = 1,       /* mmol_to_counts is not finite or not > 0, or a total was inf or NaN */
    VK_DEG_OVERFLOW = 2         /* a pool would leave [INT32_MIN, INT32_MAX]                          */
};                              /* in either case NOTHING of the agent is written                     */

/* The model, the same for every agent.  Every pointer is a DEVICE array the caller owns:
 *   transcript_row [n_transcripts]   the transcript's row of `counts`, transcripts in model order;
 *   enzyme_row [n_enzymes]           the enzyme's row of `counts`;
 *   pair_ptr [n_transcripts + 1], pair_enzyme [n_pairs], kcat [n_pairs], km [n_pairs]
 *                                    the pairs that name transcript t, in the reference's order of
 *                                    catalytic_rates: the enzyme (index into enzyme_row), her kcat
 *                                    and the pair's km in mM;
 *   composition [4 n_transcripts]    entry 4 t + i: the bases of transcript t that are monomer i
 *                                    (entries i >= n_monomers are 0); length [n_transcripts] their sum,
 *                                    at most VK_DEG_MAX_LENGTH.
 * n_rows: the rows of `counts` (a row outside [0, n_rows) reads 0 and is never written).  The
 * molecule rows are vk_tx_model's: the monomers, then ATP where it is no monomer, then ADP. */
typedef struct {
    int32_t n_transcripts, n_enzymes, n_pairs, n_monomers;
    int32_t n_rows, atp_row, adp_row, reserved;
    const int32_t *transcript_row, *enzyme_row, *pair_ptr, *pair_enzyme, *composition, *length;
    const double *kcat, *km;
} vk_deg_model;

/* One step of `timestep` (T) for agents [0, n), one agent per lane, on counts [n_rows][ld] (the
 * table vk_ssa_step steps), partial [n_transcripts][ld] (the carry), molecules [adp_row + 1][ld]
 * (transcription's pools) and m = mmol_to_counts[a].  FP64, no contraction, in exactly this order:
 *   for every transcript t in model order: level = 0.0;
 *     for every pair j of t in order, with e = her enzyme:
 *       E = (double) counts[e] / m,  S = (double) counts[t] / m,
 *       level = level + ((kcat[j] * E) * S) / (S + km[j]);
 *     total = (level * m) * T + partial[t][a];
 *     d = (int) trunc(total) (saturated where trunc(total) leaves int32),
 *     partial[t][a] = total - trunc(total);
 *     d = min(d, counts[t])                  THE ENGINE'S OWN clamp: the carry keeps only the
 *                                            fraction, the excess that could not be degraded is dropped;
 *   every E and S is evaluated from the counts as the launch found them.  Then the books:
 *     counts[t] -= d;  molecules[i] += d * composition[t][i] for every monomer i;
 *     molecules[atp_row] += d * length[t];  molecules[adp_row] -= d * length[t]
 *   (where ATP is a monomer its row takes both; ADP may go below zero).
 * VK_DEG_NONFINITE: m is not finite, m is not > 0, or a total is not finite.  VK_DEG_OVERFLOW
 * (only where not NONFINITE): a pool's new value, summed in int64, leaves int32.  In either case
 * nothing of that agent is written but her status bits and degraded_out[a] = 0.
 * degraded_out [ld]: the sum of d over the transcripts (saturated to int32).  Columns n..ld-1 of
 * every array are not touched.  A partial is always stored; a count or a pool only where it
 * changed.  No LDS, no atomics, no host synchronisation.
 * VK_ERR_ARG without a launch: a model over the VK_DEG_MAX_* limits or with a null array, n < 0,
 * ld < n, a timestep that is negative or not finite, a null array with n > 0.           */
int vk_rna_degradation_step(const vk_deg_model *model, int64_t n_agents, int64_t ld, double timestep,
                            int32_t *counts, double *partial, int32_t *molecules,
                            const double *mmol_to_counts, int32_t *degraded_out, int32_t *status,
                            vk_stream_t stream);

/* Occupancy on the device: order[k] = the agent column with the k-th smallest
 * (bin_lin[a], key[a]) (key NULL: the column index; keys distinct, < 2^32),
 * sorted_bin[k] = its bin.  n_bins bounds bin_lin (it limits the sorted bits).
 * scratch: 256-B aligned, scratch_bytes >= vk_occupancy_scratch_bytes(n).
 * No host synchronisation.                                                   */
int64_t vk_occupancy_scratch_bytes(int64_t n_agents);
int vk_occupancy_sort(const int32_t *bin_lin, const int64_t *key, int64_t n_agents, int64_t n_bins,
                      int32_t *order, int32_t *sorted_bin, void *scratch, int64_t scratch_bytes,
                      vk_stream_t stream);

/* vk_exchange_sorted from vk_occupancy_sort's output: one thread per sorted
 * slot, the head of each bin's segment adds its agents' counts in segment
 * (agent) order.  Bit-identical to vk_exchange_sorted on the host occupancy. */
int vk_exchange_ordered(double *fields, int64_t field_stride, const int32_t *sorted_bin,
                        const int32_t *order, int64_t n_agents, const int64_t *counts, int64_t ld,
                        const int32_t *map_count, const int32_t *map_field, int32_t n_map,
                        double binvol_avogadro, vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Colony mechanics: capsule contacts on a neighbour grid
 *
 *   vk_contact_step
 *       stands where the reference runs its `multibody` process
 *       (vivarium/processes/multibody_physics.py, a pymunk rigid-body
 *       simulation).  The contact model is THIS ENGINE'S OWN -- a Jacobi
 *       relaxation of capsule overlaps -- and no parity with pymunk's
 *       trajectories is claimed.  The capsules are the reference's: length
 *       and width as DeriveGlobals gives them, centre and angle as division
 *       places the daughters.
 *
 * Agent i is a capsule of centre (x, y), axis angle theta, total length L and
 * width w: radius r = w / 2, spine half-length h = max(L - w, 0) / 2.  One
 * iteration moves every agent from one snapshot of all agents: for each
 * neighbour j (ascending (grid cell, key) order) whose spine comes closer than
 * 2 r, overlap delta, it adds 0.5 * stiffness * delta along the contact normal
 * and the turn of that push about its centre times 12 / L^2; the summed push is
 * capped at max_push, the turn at +-max_turn; Gaussian jitter (jitter um on x
 * and y, jitter_angle rad) is added when either is non-zero; the centre is
 * clamped into [0, bound).  lens_amd/csrc/vk_contact.hip states every formula.
 * ------------------------------------------------------------------------- */

typedef struct vk_contact_params {
    int32_t iterations;                  /* relaxation iterations per call, >= 1       */
    int32_t gx, gy;                      /* neighbour grid: max(1, floor(bound / max_length)) per axis */
    int32_t reserved;
    double stiffness;                    /* (0, 1]: the share of an overlap removed per iteration */
    double max_length;                   /* um: no agent is longer (bit 0 of flags otherwise) */
    double width;                        /* um, every agent's                          */
    double length;                       /* um, every agent's when length is NULL      */
    double max_push;                     /* um per iteration                           */
    double max_turn;                     /* rad per iteration                          */
    double jitter, jitter_angle;         /* um, rad: standard deviations per iteration */
    uint64_t seed;                       /* Philox key                                 */
} vk_contact_params;

/* Scratch of vk_contact_step for n agents on a grid of n_grid_cells = gx * gy. */
int64_t vk_contact_scratch_bytes(int64_t n_agents, int64_t n_grid_cells);

/* p->iterations relaxation iterations for agents [0, n): location ([2][ld])
 * and angle ([ld]) are updated in place; length ([ld], NULL: p->length) is
 * read.  key (NULL: the column index; distinct, < 2^32) fixes the neighbour
 * order and the jitter draws, so results do not depend on the storage order.
 * Jitter draw j of key k at iteration s is Philox(seed + depth word 1, counter
 * (s, k, j, 0)); s = counter[0] + the iteration index, and the call then
 * advances counter[0] by p->iterations (in stream order).  flags: one int32;
 * bit 0 is ORed in when an agent is longer than a grid cell's edge (the 3 x 3
 * search may then miss contacts; the call still runs).  bin_lin (and bin_ix,
 * nullable) receive vk_bin_sites' bins of the final locations on the nx x ny
 * lattice of bound_x x bound_y (a whole, unbanded plane).  scratch: 256-B
 * aligned, >= vk_contact_scratch_bytes(n, gx * gy).  Argument errors return
 * VK_ERR_ARG and launch nothing; n == 0 returns VK_OK.  No host
 * synchronisation: the call can be captured into a graph.                   */
int vk_contact_step(const vk_contact_params *p, int64_t n_agents, int64_t ld, double *location,
                    double *angle, const double *length, const int64_t *key, uint64_t *counter,
                    int32_t *flags, int32_t nx, int32_t ny, double bound_x, double bound_y,
                    int32_t *bin_lin, int32_t *bin_ix, void *scratch, int64_t scratch_bytes,
                    vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Mother machine: channel walls and outflow in the contact launch
 *
 *   vk_contact_step_channels
 *       stands where the reference's multibody builds its mother machine
 *       (vivarium/library/pymunk_multibody.py:218-230: vertical wall segments
 *       at x = channel_space * line, 0 <= y <= channel_height, of thickness
 *       spacer_thickness) and marks the cells pushed out of the top
 *       (vivarium/processes/multibody_physics.py:232-250: y > channel_height
 *       goes into `_delete`).  The wall law is THIS ENGINE'S OWN -- a
 *       projection, not pymunk's segments -- and there is no flow.
 *
 * Lines stand at x = space * l, l = 0 .. n_lines - 1, n_lines = floor(bound_x /
 * space); channel c lies between lines c and c + 1, the last one between line
 * n_lines - 1 and the plane's edge.  After an agent's capped push and jitter,
 * and before the plane's clamp:
 *   y > height: the agent is left alone and outflow[a] is set (iteration 0
 *     writes the flag, later iterations OR into it: an agent above the channels
 *     after any iteration of the call stays flagged);
 *   otherwise c = clamp(floor(x_snapshot / space), 0, n_lines - 1), the channel
 *     the agent was in before the move, lo = c space + (r + spacer), hi =
 *     (c + 1) space - (r + spacer) (the last channel: nextafter(bound_x, 0));
 *     with h > 0 and |cos theta| > cmax = min((hi - lo) / (2 h), 1), theta :=
 *     atan2(copysign(sqrt(1 - cmax^2), sin theta), copysign(cmax, cos theta));
 *     then, e = h |cos theta|, x is clamped into [lo + e, max(hi - e, lo + e)].
 * ------------------------------------------------------------------------- */

typedef struct vk_contact_channels {
    double height;                       /* um: 0 < height <= bound_y                  */
    double space;                        /* um between lines, >= width + 2 spacer      */
    double spacer;                       /* um: a line's thickness, >= 0               */
    int32_t n_lines;                     /* floor(bound_x / space), >= 1               */
    int32_t reserved;
} vk_contact_channels;

/* vk_contact_step with channels: the same arguments, then ch and outflow ([ld]
 * int32, nullable: 1 for every agent of [0, n) above the channels after an
 * iteration of this call, 0 for the others).  ch == NULL runs vk_contact_step
 * itself (outflow is then not written).  Argument errors return VK_ERR_ARG and
 * launch nothing.  No host synchronisation.                                  */
int vk_contact_step_channels(const vk_contact_params *p, int64_t n_agents, int64_t ld,
                             double *location, double *angle, const double *length,
                             const int64_t *key, uint64_t *counter, int32_t *flags, int32_t nx,
                             int32_t ny, double bound_x, double bound_y, int32_t *bin_lin,
                             int32_t *bin_ix, void *scratch, int64_t scratch_bytes,
                             const vk_contact_channels *ch, int32_t *outflow, vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Colony metrics: connected colonies, mass, area, axes
 *
 *   vk_colony_metrics
 *       stands where the reference wires its ColonyShapeDeriver into the
 *       lattice (vivarium/compartments/lattice.py:61-64,
 *       vivarium/processes/derive_colony_shape.py:97-217) and emits
 *       colony_global.  The definition is THIS ENGINE'S OWN, not alphashape's:
 *       no polygon is built, there is no circumference, and the area is the
 *       sum of the capsules' own areas.  The colony count and the colony
 *       masses agree with the reference on its own seven test scenarios
 *       (cells as unit circles, link_gap 0.25).
 *
 * Agents are vk_contact_step's capsules (r = w / 2, h = max(L - w, 0) / 2).
 * Link: agents i != j are linked when (2 r + link_gap) - d_ij >= 0, d_ij the
 * distance of the closest points of the two spines by the contact kernel's own
 * arithmetic (its closest-point solve and clamps, the den > 1e-12 parallel
 * branch, d = 0 for coincident spines).  An agent whose x or y is not finite
 * links to nobody and gets colony = -1 whatever min_cells is.
 * Colony: a connected component of the link graph with >= min_cells members;
 * agents of smaller components get colony = -1.  Colonies are numbered
 * 0 .. C - 1 in the order of their first member in ascending (grid cell, key)
 * order; colony_key[c] is the smallest key among the members.  Nothing depends
 * on the storage order or the launch geometry.
 * Per colony c, over its members in ascending (grid cell, key) order:
 *   cells[c]                 the member count
 *   VK_COLONY_MASS           sum of mass (p->mass each when mass is NULL)
 *   VK_COLONY_CELL_AREA      sum of w max(L - w, 0) + pi w^2 / 4 (overlaps of
 *                            two capsules are counted twice)
 *   VK_COLONY_CX, _CY        the mean of the centres
 *   VK_COLONY_SXX, _SYY, _SXY   the second moments of the centres about it
 *   VK_COLONY_ANGLE          phi = 0.5 atan2(2 sxy, sxx - syy); isotropic: 0
 *   VK_COLONY_MAJOR, _MINOR  the larger and the smaller of the extents along
 *                            e1 = (cos phi, sin phi) and across it; along e:
 *                            max(p.e + h |u.e| + r) - min(p.e - h |u.e| - r)
 *                            over the members, p taken about the centroid
 * Sum order (also of min and max).  A run of members is combined by one
 * workgroup of 256 threads: thread t combines members t, t + 256, t + 512, ...
 * of the run in that order starting from the identity; each wave of 64
 * combines its lanes by the butterfly p = p op shfl_xor(p, o), o = 32, 16, 8,
 * 4, 2, 1; the four waves are combined as ((w0 op w1) op w2) op w3.  A colony
 * of at most 512 members is one run; a larger one is 64 runs of
 * S = 256 ceil(size / 16384) consecutive members each (the last may be short
 * or empty: the identity), combined in order as ((P0 op P1) op P2) ... op P63.
 * A function of the member sequence alone.  No floating-point atomics.
 * lens_amd/csrc/vk_colonies.hip states every formula.
 * ------------------------------------------------------------------------- */

enum vk_colony_row {
    VK_COLONY_MASS = 0,
    VK_COLONY_CELL_AREA = 1,
    VK_COLONY_CX = 2,
    VK_COLONY_CY = 3,
    VK_COLONY_SXX = 4,
    VK_COLONY_SYY = 5,
    VK_COLONY_SXY = 6,
    VK_COLONY_ANGLE = 7,
    VK_COLONY_MAJOR = 8,
    VK_COLONY_MINOR = 9,
    VK_COLONY_ROWS = 10
};

enum vk_colonies_flag {
    VK_COLONIES_TOO_LONG = 1,   /* an agent is longer than max_length (or than a grid cell's edge) */
    VK_COLONIES_GAVE_UP = 2     /* a union ran out of retries: the labels are not to be used      */
};

typedef struct vk_colonies_params {
    int32_t gx, gy;                      /* neighbour grid: max(1, floor(bound / (max_length + link_gap))) per axis */
    int32_t min_cells;                   /* >= 1: the members a component needs to be a colony */
    int32_t reserved;
    double max_length;                   /* um: no agent is longer (bit 0 of flags otherwise) */
    double width;                        /* um, every agent's                          */
    double length;                       /* um, every agent's when length is NULL      */
    double link_gap;                     /* um, >= 0: capsules closer than this are linked */
    double mass;                         /* every agent's mass when mass is NULL       */
} vk_colonies_params;

/* Scratch of vk_colony_metrics for n agents on a grid of n_grid_cells = gx * gy. */
int64_t vk_colonies_scratch_bytes(int64_t n_agents, int64_t n_grid_cells);

/* Colonies of agents [0, n): location ([2][ld]), angle ([ld]), length ([ld],
 * NULL: p->length), mass ([ld], NULL: p->mass) and key ([ld] int64, NULL: the
 * column index; distinct, < 2^32) are read.  Outputs: colony ([ld] int32: the
 * colony of each agent of [0, n), or -1), n_colonies (one device int32: C),
 * cells ([ld] int32), colony_key ([ld] int64) and metrics ([VK_COLONY_ROWS][ld]
 * doubles; NULL: labels, cells and keys only); entries at or beyond C are not
 * written.  flags: one int32 the caller zeroes; vk_colonies_flag bits are ORed
 * in (the call still runs).  scratch: 256-B aligned, >=
 * vk_colonies_scratch_bytes(n, gx * gy).  Argument errors return VK_ERR_ARG and
 * launch nothing; n == 0 returns VK_OK with *n_colonies = 0.  No host
 * synchronisation: the call can be captured into a graph.  No kernel waits on
 * another workgroup and nothing is polled.                                   */
int vk_colony_metrics(const vk_colonies_params *p, int64_t n_agents, int64_t ld, const double *location,
                      const double *angle, const double *length, const double *mass,
                      const int64_t *key, double bound_x, double bound_y, int32_t *colony,
                      int32_t *n_colonies, int32_t *cells, int64_t *colony_key, double *metrics,
                      int32_t *flags, void *scratch, int64_t scratch_bytes, vk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Antibiotic response: membrane diffusion, death, the float exchange
 *
 *   vk_response_begin / vk_response_end (+ vk_response_cells)
 *       stand, together with vk_expression_step, where the reference's
 *       Antibiotics compartment (vivarium/compartments/antibiotics.py:106-159)
 *       runs CellEnvironmentDiffusion.next_update (vivarium/processes/
 *       diffusion_cell_environment.py:92-138) and DeathFreezeState.next_update
 *       (vivarium/processes/death.py:105-118, 197-219) beside the kinetics.
 *   vk_exchange_ordered_mixed / vk_exchange_atomic_f64
 *       apply the membrane's float counts to the field with
 *       update_field_with_exchange's conversion (vivarium/core/registry.py:
 *       149-183), the first interleaved per agent with the kinetics' int64 counts.
 *
 * The existing launches (kinetics, expression, growth) run on every agent.  A
 * frozen (dead) agent's columns are saved by `begin` and put back by `end`, so
 * the launches' results for it are discarded and no launch changes.
 * ------------------------------------------------------------------------- */

/* All pointers are DEVICE arrays owned by the caller; rows index conc[][ld]. */
typedef struct vk_response_table {
    int32_t n_mol, n_porin, n_det, n_save, n_expr, n_flux, n_ext, reserved;
    const int32_t *mol_int_row;   /* [n_mol] the cell's row of each diffusing molecule   */
    const int32_t *mol_ext_row;   /* [n_mol] its ('external', m) row                      */
    const int32_t *porin_row;     /* [n_porin]                                            */
    const double *porin_perm;     /* [n_porin] permeability, summed in this order         */
    const int32_t *det_row;       /* [n_det] detector keys                                */
    const double *det_thr;        /* [n_det] dying when conc > thr (strict)               */
    const int32_t *save_row;      /* [n_save] conc rows the kinetics launch overwrites    */
    const int32_t *expr_row;      /* [n_expr] conc row of vk_expression_step's update row j */
    double avogadro;              /* counts = flux_mmol * 1e-3 * avogadro                 */
    double volume_fl;             /* every agent's volume (fL) when volume is NULL        */
} vk_response_table;

/* Before the kinetics launch, from the step-start state of agents [0, n):
 *   dying[a] = !frozen[a] && any_d(conc[det_row[d]] > det_thr[d]);
 *   rate = 0 + sum_p conc[porin_row[p]] * porin_perm[p] (in order);
 *   flux_mmol = (conc[int_m] - conc[ext_m]) * rate * dt;
 *   delta[m][a] = -(flux_mmol / volume * 1e15); fcounts[m][a] = flux_mmol * 1e-3 * avogadro;
 *   frozen agents: save_conc[s][a] = conc[save_row[s]][a], save_flux := flux,
 *   save_status := status, save_nsteps := nsteps.
 * volume ([ld], fL; NULL: t->volume_fl).  flux is [n_flux][ld]; status and
 * nsteps (and their save arrays) may be NULL.                                */
int vk_response_begin(const vk_response_table *t, int64_t n_agents, int64_t ld, double dt, const double *conc,
                      const double *volume, const int32_t *frozen, int32_t *dying, double *delta,
                      double *fcounts, double *save_conc, const double *flux, double *save_flux,
                      const int32_t *status, int32_t *save_status, const int32_t *nsteps,
                      int32_t *save_nsteps, vk_stream_t stream);

/* After the kinetics launch, before the exchange:
 *   frozen agents: the saved columns go back and counts[e][a] = 0 (e < n_ext);
 *   live agents: conc[expr_row[j]] += expr_update[j] (expr_update NULL: none);
 *   every agent: conc[int_m] = conc[int_m] + delta[m];
 *   dying agents: dead = frozen = 1.                                          */
int vk_response_end(const vk_response_table *t, int64_t n_agents, int64_t ld, double *conc, const double *delta,
                    const double *expr_update, int32_t *frozen, const int32_t *dying, int32_t *dead,
                    const double *save_conc, double *flux, const double *save_flux, int32_t *status,
                    const int32_t *save_status, int32_t *nsteps, const int32_t *save_nsteps,
                    int64_t *counts, vk_stream_t stream);

/* Around vk_cell_step: restore == 0 saves a frozen agent's cell rows
 * ([VK_CELL_ROWS][ld]), mmol_to_counts and divide flag, restore != 0 puts them back.
 * Agents with dying[a] != 0 (frozen by this step's vk_response_end) are left alone:
 * the step of detection still grows and may divide them.                      */
int vk_response_cells(int32_t restore, int64_t n_agents, int64_t ld, const int32_t *frozen,
                      const int32_t *dying, double *cell, double *m2c, int32_t *divide, double *save_cell, double *save_m2c,
                      int32_t *save_divide, vk_stream_t stream);

/* vk_exchange_ordered with a second, float64 counts array and its own map.  Per
 * bin, in segment (agent) order and per agent: v = v + mM(int count) then
 * v = v + mM(float count), mM(c) = c / binvol_avogadro * 1000 -- what applying
 * agent after agent gives.  Either array may be NULL (with its n_map 0).     */
int vk_exchange_ordered_mixed(double *fields, int64_t field_stride, const int32_t *sorted_bin,
                              const int32_t *order, int64_t n_agents, const int64_t *counts, int64_t ld,
                              const int32_t *map_count, const int32_t *map_field, int32_t n_map,
                              const double *fcounts, int64_t ld_f, const int32_t *map_fcount,
                              const int32_t *map_ffield, int32_t n_fmap, double binvol_avogadro,
                              vk_stream_t stream);

/* vk_exchange_atomic for float64 counts (launched after the int64 one). */
int vk_exchange_atomic_f64(double *fields, int64_t field_stride, const int32_t *bin_lin, int64_t n_agents,
                           const double *fcounts, int64_t ld, const int32_t *map_count,
                           const int32_t *map_field, int32_t n_map, double binvol_avogadro,
                           vk_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VK_KINETICS_H */
