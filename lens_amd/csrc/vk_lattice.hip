// diffusion_field lattice on MI355X (gfx950): 5-point reflect stencil,
// uniform-field detection, local-environment gather, agent exchange scatter.
//
// Reference semantics: vivarium/processes/diffusion_field.py:385-407
// (fixed 0.01 s substeps of f += (D/(dx*dy)*dt) * convolve(f, LAP,
// mode='reflect'), uniform skip, delta accumulated), :362-379 (local
// environments), vivarium/core/registry.py:149-183 (exchange updater),
// vivarium/library/lattice_utils.py:18-58 (bin sites / bin volume).
// Compiled with -ffp-contract=off: the Laplacian is summed up, left,
// -4*centre, right, down exactly as scipy.ndimage.convolve does, and the
// update is c + coef*lap with two roundings, so fields are bit-identical to
// the reference's.
//
// HBM layout: one plane per molecule, row-major [rows][ny] (axis 0 = x as in
// the reference's ndarray), planes field_stride apart.  A rank's plane holds
// its owned row band plus halo rows.

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>


#include "vk_bin.h"
#include "vk_internal.h"
#include "vk_pass_plan.h"
#include "vk_stencil_launch.h"

constexpr int ST_BX = 256;  // columns per block (4 waves, 2 KiB per row load)
constexpr int ST_RB = 16;   // rows walked per block

// One substep over rows [lo, hi) of every plane.  Each lane walks down a
// column keeping up/centre/down in registers: one new row load, two shifted
// loads (left/right: L1 hits on the lines the wave just fetched), one store.
__global__ __launch_bounds__(ST_BX) void k_diffuse_substep(const double *__restrict__ src,
                                                           double *dst,
                                                           const double *f0,
                                                           int64_t field_stride, int ny, int lo, int hi,
                                                           int top_reflect, int bot_reflect, double coef,
                                                           const double *__restrict__ uniform, int delta_mode) {
    const int f = blockIdx.z;
    const int j = blockIdx.x * ST_BX + threadIdx.x;
    const int r0 = lo + blockIdx.y * ST_RB;
    if (j >= ny || r0 >= hi) return;
    const int r1 = min(r0 + ST_RB, hi);
    const double *s = src + (int64_t)f * field_stride;
    double *d = dst + (int64_t)f * field_stride;
    const double *g = f0 ? f0 + (int64_t)f * field_stride : nullptr;
    if (uniform && uniform[2 * f] == uniform[2 * f + 1]) {   // uniform plane: the delta is zero
        if (delta_mode)
            for (int r = r0; r < r1; ++r) d[(int64_t)r * ny + j] = 0.0;
        return;
    }
    const int jl = j > 0 ? j - 1 : 0;
    const int jr = j < ny - 1 ? j + 1 : ny - 1;
    const int ru = (r0 == top_reflect) ? r0 : r0 - 1;
    double up = s[(int64_t)ru * ny + j];
    double c = s[(int64_t)r0 * ny + j];
    for (int r = r0; r < r1; ++r) {
        const int rd = (r == bot_reflect) ? r : r + 1;
        const double down = s[(int64_t)rd * ny + j];
        const double left = s[(int64_t)r * ny + jl];
        const double right = s[(int64_t)r * ny + jr];
        const double lap = (((up + left) + (-4.0 * c)) + right) + down;
        double v = c + coef * lap;
        if (g) {
            // delta_mode: the reference's delta = field_new - field, applied
            // later by the accumulate updater (diffusion_field.py:394)
            const double base = g[(int64_t)r * ny + j];
            v = delta_mode ? v - base : base + (v - base);
        }
        d[(int64_t)r * ny + j] = v;
        up = c;
        c = down;
    }
}

static int g_stencil_rows = 0;    // output rows per wave tile (vk_stencil_kernels.h chunk_rows); 0 = auto
// Exact mode: 2 / 3 = wave tile lag-1 prefetching 3 / 6 rows, 6 = variant 3 with
// streaming stores at depths 7 / 9 / 11 (the exact mode's kernel for every other
// setting).  Tolerance mode: 20 = pair-sum passes (vk_stencil_ps.h, the default; 2 /
// 3 / 6 select it too), 40 = the stage-split 10-deep pass (vk_stencil_sp.h; row
// bands), 70 = the 10-deep pair-sum pass with line-aligned tiles (96 written columns,
// vk_stencil_ps10.hip; the C4 default since round 6).  Tolerance-mode depths without a pair-sum pass (even depths below 10, 13,
// 15) run the exact wave tiles.
// Retired after A/B on the GPU: 0 (workgroup tile, LDS exchange),
// 1 (lag-2 wave tile), 4 (9 rows prefetched), 5 (4 waves/SIMD cap, spills),
// 7 (streaming loads), 8-11 (four columns per lane, compact boundary body, split
// stages, LDS-crossbar neighbours), 12-16 (prefetch ring, buffer stores, zigzag
// chunks, 6-row prefetch at depth 10), 21-32 (pair-sum prefetch depths, stagger,
// cache policies, one plane at a time, coupled-pass placements, the stage-0 ring as
// 16-B vectors: 30 tied variant 20 and was retired in round 5), the tolerance-mode
// FMA form of the wave tiles (4 FP64 ops per cell-substep; round 6) -- none faster.
static int g_stencil_kernel = 20;

extern "C" int vk_set_stencil_kernel(int32_t variant, int32_t rows) {
    const int prev = g_stencil_kernel;
    if (variant == 2 || variant == 3 || variant == 6 || variant == 20 || variant == 40 || variant == 70)
        g_stencil_kernel = variant;
    if (rows == 0 || (rows >= 8 && rows <= 4096)) g_stencil_rows = rows;
    return prev;
}

// 0 = bit-exact with scipy.ndimage.convolve (the default), 1 = tolerance mode: the
// pair-sum passes (3 FP64 ops per cell-substep instead of 6, vk_stencil_ps.h) and no
// base re-read in the final pass; fields agree with the exact mode to ~1e-14
// relative (tests/test_stencil_modes.py)
static int g_stencil_mode = 0;

extern "C" int vk_set_stencil_mode(int32_t mode) {
    const int prev = g_stencil_mode;
    if (mode == 0 || mode == 1) g_stencil_mode = mode;
    return prev;
}

// max substeps per HBM pass: odd, 1 = one launch per substep; or 10, which plans a
// tolerance-mode whole step of a multiple of 10 substeps as 10-deep passes (three
// buffers: the field itself is free once the first pass has read it), other calls
// as depth 9
static int g_stencil_depth = 10;   // 10-deep block plan (odd-depth plan at 9 for other counts)

extern "C" int vk_set_stencil_depth(int32_t k) {
    const int prev = g_stencil_depth;
    if (k == 10) g_stencil_depth = 10;
    else if (k >= 1 && k <= 15) g_stencil_depth = k | 1;
    return prev;
}

// ---------------------------------------------------------------------------
// Segment timestamps (bench instrumentation inside a replayed HIP graph)
// ---------------------------------------------------------------------------

__global__ void k_timestamp(uint64_t *out, int idx) {
    if (threadIdx.x == 0) out[idx] = wall_clock64();
}

extern "C" int vk_timestamp(uint64_t *out, int32_t idx, vk_stream_t stream) {
    if (!out || idx < 0) {
        vk::set_error("vk_timestamp: bad arguments");
        return VK_ERR_ARG;
    }
    hipLaunchKernelGGL(k_timestamp, dim3(1), dim3(64), 0, (hipStream_t)stream, out, idx);
    return vk::launch_check("k_timestamp");
}

// The box's streaming-copy floor for a pass's planes: one 16-B element per thread,
// non-temporal store, one wave of workgroups over the whole buffer.  Of the copy
// shapes measured (scripts/micro/copy_floor.hip, profiles/r03/copy_floor.log) this
// one is fastest: 84.4 us for a 4096^2 x 2 FP64 pair, 6.36 TB/s; grid-stride copies
// and torch's copy_ reach 5.5-6.1.
typedef double vk_d2v __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void k_copy_stream(const vk_d2v *__restrict__ s, vk_d2v *__restrict__ d, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) __builtin_nontemporal_store(s[i], d + i);
}

extern "C" int vk_copy_stream(const double *src, double *dst, int64_t n_doubles, vk_stream_t stream) {
    if (!src || !dst || n_doubles < 0 || (n_doubles & 1) || (((uintptr_t)src | (uintptr_t)dst) & 15)) {
        vk::set_error("vk_copy_stream: bad arguments (16-B aligned buffers of an even number of doubles)");
        return VK_ERR_ARG;
    }
    const int64_t n = n_doubles / 2;
    if (n == 0) return VK_OK;
    hipLaunchKernelGGL(k_copy_stream, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const vk_d2v *)src, (vk_d2v *)dst, n);
    return vk::launch_check("k_copy_stream");
}

extern "C" int64_t vk_wall_clock_khz(void) {
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return 0;
    return khz;
}

// rows [lo, hi) of every non-uniform plane: dst <- src
__global__ __launch_bounds__(256) void k_copy_rows(const double *__restrict__ src, double *dst,
                                                   int64_t field_stride, int64_t off, int64_t count,
                                                   const double *__restrict__ uniform) {
    const int f = blockIdx.y;
    if (uniform && uniform[2 * f] == uniform[2 * f + 1]) return;
    const int64_t base = (int64_t)f * field_stride + off;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x)
        dst[base + i] = src[base + i];
}

// ---------------------------------------------------------------------------
// vk_diffuse / vk_diffuse_part / vk_diffuse_coupled: validate, plan
// (vk_pass_plan.h), launch each pass of the plan
// ---------------------------------------------------------------------------

// Row bands of a whole-plane step on two streams (vk_plan::plan_lanes): 0 = the
// automatic rule, 1 = off, 2 = forced, the top band of the first pass top_rows rows
static int g_stencil_bands = 0;
static int g_stencil_top_rows = 0;

extern "C" int vk_set_stencil_bands(int32_t bands, int32_t top_rows) {
    const int prev = g_stencil_bands;
    if (bands == 0 || bands == 1 || (bands == 2 && top_rows > 0)) {
        g_stencil_bands = bands;
        g_stencil_top_rows = bands == 2 ? top_rows : 0;
    }
    return prev;
}

static vk_plan::Settings stencil_settings() {
    return {g_stencil_mode, g_stencil_depth, g_stencil_kernel, g_stencil_rows, g_stencil_bands, g_stencil_top_rows};
}

// Lane 1 of a banded plan: one non-blocking stream per device, owned by the library,
// and the events that order the two lanes (timing disabled; a pass's wait takes the
// event's state when it is enqueued, so the next call records the same events again).
// Made by the first banded call that finds the caller's stream not capturing: nothing
// is created under capture, where a call without them runs the unbanded plan.  A
// device's banded calls share them, so (like the settings) they are for one host
// thread at a time.
constexpr int BAND_EVENTS = 66;    // the fork, the join, and one per pass of the longest plan (64 passes)
struct BandLanes {
    hipStream_t stream = nullptr;
    hipEvent_t ev[BAND_EVENTS] = {};
};
static std::mutex g_band_mutex;
static std::vector<BandLanes *> g_band_lanes;   // by device

static BandLanes *band_lanes(hipStream_t caller) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return nullptr;
    std::lock_guard<std::mutex> lock(g_band_mutex);
    if ((size_t)dev >= g_band_lanes.size()) g_band_lanes.resize(dev + 1, nullptr);
    if (g_band_lanes[dev]) return g_band_lanes[dev];
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(caller, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return nullptr;
    BandLanes *l = new BandLanes;
    bool ok = hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < BAND_EVENTS; ++i) ok = hipEventCreateWithFlags(&l->ev[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        for (hipEvent_t e : l->ev)
            if (e) (void)hipEventDestroy(e);
        if (l->stream) (void)hipStreamDestroy(l->stream);
        delete l;
        (void)hipGetLastError();
        return nullptr;
    }
    g_band_lanes[dev] = l;
    return l;
}

// What a call's passes share: the three buffers (indexed by VK_BUF_*), the planes,
// the reflected rows, the coefficient; cp (nullable): the agent coupling of a
// coupled step, of which each pass carries its own bits.
struct PassArgs {
    double *buf[3];
    int nf;
    int64_t fs;
    int ny, top, bot, tile_rows;
    double coef;
    const double *uniform;
    const VkPsCouple *cp;
    hipStream_t stream;
};

static void launch_pass(const vk_pass &p, const PassArgs &a) {
    typedef void (*launcher)(VK_STENCIL_LAUNCH_ARGS);
    static const launcher launchers[] = {nullptr,        vk_launch_wl3,  vk_launch_wl6,          vk_launch_wl6nt,
                                         vk_launch_ps,   vk_launch_ps10, vk_launch_ps10_aligned, nullptr,
                                         vk_launch_sp};
    const double *src = a.buf[p.src], *f0 = p.f0 ? a.buf[VK_BUF_FIELD] : nullptr;
    double *dst = a.buf[p.dst];
    VkPsCouple c = {};
    if (a.cp) c = *a.cp, c.mode = p.couple;
    const VkPsCouple *cp = a.cp ? &c : nullptr;
    if (p.kernel == VK_PASS_SINGLE) {
        dim3 grid((a.ny + ST_BX - 1) / ST_BX, (p.hi - p.lo + ST_RB - 1) / ST_RB, a.nf);
        hipLaunchKernelGGL(k_diffuse_substep, grid, dim3(ST_BX), 0, a.stream, src, dst, f0, a.fs, a.ny, p.lo, p.hi, a.top,
                           a.bot, a.coef, a.uniform, 0);
    } else if (p.kernel == VK_PASS_PS10_STRIPS) {
        vk_launch_ps10_strips(p.k, a.stream, src, dst, f0, a.nf, a.fs, a.ny, p.lo, p.hi, p.in_lo, p.in_hi, a.top, a.bot,
                              a.coef, a.uniform, cp, a.tile_rows, p.gap_lo, p.gap_hi);
    } else {
        launchers[p.kernel](p.k, a.stream, src, dst, f0, a.nf, a.fs, a.ny, p.lo, p.hi, p.in_lo, p.in_hi, a.top, a.bot,
                            a.coef, a.uniform, cp, a.tile_rows);
    }
}

// Plans the call and launches its passes.  Uniform planes skip every pass (nothing
// reads the buffers they leave unwritten) and keep their field.
static int run_plan(const char *what, const vk_plan::Call &c, double *field, double *work0, double *work1, int32_t n_fields,
                    int64_t field_stride, int32_t ny, double coeff_dt, const double *uniform, const VkPsCouple *cp,
                    vk_stream_t stream) {
    vk_plan::Settings st = stencil_settings();
    std::vector<vk_pass> passes;
    std::vector<int32_t> lane, after;
    const char *why = "";
    int rc = vk_plan::plan_lanes(st, c, passes, lane, after, &why);
    if (rc) {
        vk::set_error("%s: %s", what, why);
        return rc;
    }
    if (n_fields == 0) return VK_OK;
    // A banded plan: lane 0 is the caller's stream, lane 1 the library's.  Lane 1 starts
    // after what the caller's stream holds (the fork); a pass with an `after` waits for
    // the event recorded behind that pass; the caller's stream ends waiting for lane 1's
    // last pass (the join), so whatever follows the call sees the whole step.
    const bool banded = std::find(lane.begin(), lane.end(), 1) != lane.end();
    BandLanes *bl = banded ? band_lanes((hipStream_t)stream) : nullptr;
    // the event of each pass that another waits for
    std::vector<int> slot(passes.size(), -1);
    int slots = 0;
    for (int32_t i : after)
        if (i >= 0 && slot[i] < 0) slot[i] = slots++;
    if (banded && (!bl || slots + 2 > BAND_EVENTS)) {   // (no lanes yet, under capture)
        st.bands = 1;
        bl = nullptr;
        if ((rc = vk_plan::plan_lanes(st, c, passes, lane, after, &why))) return rc;
    }
    PassArgs a = {{field, work0, work1}, n_fields, field_stride, ny, c.edge_top ? c.lo_min : -1,
                  c.edge_bot ? c.hi_max - 1 : 0x7fffffff, st.rows, coeff_dt, uniform, cp, (hipStream_t)stream};
    if (bl) {
        hipStream_t lanes[2] = {(hipStream_t)stream, bl->stream};
        hipEvent_t fork = bl->ev[BAND_EVENTS - 2], join = bl->ev[BAND_EVENTS - 1];
        if ((rc = vk::hip_check(hipEventRecord(fork, lanes[0]), what))) return rc;
        if ((rc = vk::hip_check(hipStreamWaitEvent(lanes[1], fork, 0), what))) return rc;
        // Once lane 1 has joined the caller's work (and, under capture, its capture) the
        // join below must be reached: a failed launch is reported after it.
        int failed = VK_OK;
        for (size_t i = 0; i < passes.size() && !failed; ++i) {
            a.stream = lanes[lane[i]];
            if (after[i] >= 0) failed = vk::hip_check(hipStreamWaitEvent(a.stream, bl->ev[slot[after[i]]], 0), what);
            if (failed) break;
            launch_pass(passes[i], a);
            failed = vk::launch_check(what);
            if (!failed && slot[i] >= 0) failed = vk::hip_check(hipEventRecord(bl->ev[slot[i]], a.stream), what);
        }
        rc = vk::hip_check(hipEventRecord(join, lanes[1]), what);
        if (!rc) rc = vk::hip_check(hipStreamWaitEvent(lanes[0], join, 0), what);
        return failed ? failed : rc;
    }
    for (const vk_pass &p : passes) {
        launch_pass(p, a);
        if ((rc = vk::launch_check(what))) return rc;
        if (p.copy_back) {
            const int64_t count = (int64_t)(c.row_hi - c.row_lo) * ny;
            const unsigned blocks = (unsigned)std::min<int64_t>(2048, (count + 255) / 256);
            hipLaunchKernelGGL(k_copy_rows, dim3(blocks, n_fields), dim3(256), 0, a.stream, work0, field, field_stride,
                               (int64_t)c.row_lo * ny, count, uniform);
            if ((rc = vk::launch_check("k_copy_rows"))) return rc;
        }
    }
    return VK_OK;
}

extern "C" int vk_diffuse_part(double *field, double *work0, double *work1, int32_t n_fields, int64_t field_stride,
                               int32_t ny, int32_t row_lo, int32_t row_hi, int32_t lo_min, int32_t hi_max,
                               int32_t edge_top, int32_t edge_bot, int32_t sub_begin, int32_t sub_count,
                               int32_t n_sub, double coeff_dt, const double *uniform, int32_t part,
                               int32_t interior_passes, vk_stream_t stream) {
    const vk_plan::Call c = {row_lo,    row_hi,    lo_min, hi_max, edge_top,        edge_bot,
                             sub_begin, sub_count, n_sub,  part,   interior_passes, 0};
    if (part != VK_PART_ALL && part != VK_PART_INTERIOR && part != VK_PART_EDGES) {
        vk::set_error("vk_diffuse_part: part must be VK_PART_ALL / _INTERIOR / _EDGES");
        return VK_ERR_ARG;
    }
    if (!field || n_fields < 0 || ny <= 0 || !vk_plan::geometry_ok(c) || (int64_t)hi_max * ny > field_stride) {
        vk::set_error("vk_diffuse: bad geometry");
        return VK_ERR_ARG;
    }
    if (!work0 || (n_sub > 2 && !work1)) {
        vk::set_error("vk_diffuse: work buffers required");
        return VK_ERR_ARG;
    }
    return run_plan("vk_diffuse", c, field, work0, work1, n_fields, field_stride, ny, coeff_dt, uniform, nullptr, stream);
}

extern "C" int vk_diffuse(double *field, double *work0, double *work1, int32_t n_fields,
                          int64_t field_stride, int32_t ny, int32_t row_lo, int32_t row_hi, int32_t lo_min,
                          int32_t hi_max, int32_t edge_top, int32_t edge_bot, int32_t sub_begin,
                          int32_t sub_count, int32_t n_sub, double coeff_dt, const double *uniform,
                          vk_stream_t stream) {
    return vk_diffuse_part(field, work0, work1, n_fields, field_stride, ny, row_lo, row_hi, lo_min, hi_max, edge_top,
                           edge_bot, sub_begin, sub_count, n_sub, coeff_dt, uniform, VK_PART_ALL, 0, stream);
}

extern "C" int vk_diffuse_plan_lanes(int32_t row_lo, int32_t row_hi, int32_t lo_min, int32_t hi_max, int32_t edge_top,
                                     int32_t edge_bot, int32_t sub_begin, int32_t sub_count, int32_t n_sub,
                                     int32_t part, int32_t interior_passes, int32_t coupled, vk_pass *out,
                                     int32_t *lane, int32_t *after, int32_t capacity, int32_t *n_passes) {
    const vk_plan::Call c = {row_lo,    row_hi,    lo_min, hi_max, edge_top,        edge_bot,
                             sub_begin, sub_count, n_sub,  part,   interior_passes, coupled};
    const bool whole_step = row_lo == 0 && lo_min == 0 && row_hi == hi_max && sub_begin == 0 && sub_count == n_sub &&
                            part == VK_PART_ALL;
    if (!n_passes || capacity < 0 || (capacity > 0 && !out) || part < VK_PART_ALL || part > VK_PART_EDGES ||
        coupled < 0 || coupled > VK_PLAN_COUPLED_AGENTS || (coupled && !whole_step) || !vk_plan::geometry_ok(c)) {
        vk::set_error("vk_diffuse_plan: bad arguments");
        return VK_ERR_ARG;
    }
    std::vector<vk_pass> passes;
    std::vector<int32_t> lanes, afters;
    const char *why = "";
    const int rc = vk_plan::plan_lanes(stencil_settings(), c, passes, lanes, afters, &why);
    if (rc) vk::set_error("vk_diffuse_plan: %s", why);
    *n_passes = (int32_t)passes.size();
    const size_t n = std::min<size_t>(passes.size(), (size_t)capacity);
    std::copy_n(passes.begin(), n, out);
    if (lane) std::copy_n(lanes.begin(), n, lane);
    if (after) std::copy_n(afters.begin(), n, after);
    return rc;
}

extern "C" int vk_diffuse_plan(int32_t row_lo, int32_t row_hi, int32_t lo_min, int32_t hi_max, int32_t edge_top,
                               int32_t edge_bot, int32_t sub_begin, int32_t sub_count, int32_t n_sub, int32_t part,
                               int32_t interior_passes, int32_t coupled, vk_pass *out, int32_t capacity,
                               int32_t *n_passes) {
    return vk_diffuse_plan_lanes(row_lo, row_hi, lo_min, hi_max, edge_top, edge_bot, sub_begin, sub_count, n_sub, part,
                                 interior_passes, coupled, out, nullptr, nullptr, capacity, n_passes);
}

// A whole-plane step's passes with the agent coupling inside them: the first
// pass also gathers each agent's external concentrations from the pre-step
// planes, the final pass also scatters the exchange into the new planes (one
// launch each less, and the exchange's read-modify-write of the planes happens
// while the final pass holds them).  Either arithmetic mode.  Returns
// VK_ERR_LIMIT, launching nothing, when the step is not planned as two or more
// fused passes.
extern "C" int vk_diffuse_coupled(double *field, double *work0, double *work1, int32_t n_fields,
                                  int64_t field_stride, int32_t ny, int32_t rows, int32_t n_sub, double coeff_dt,
                                  const double *uniform, const int32_t *bin_lin, const int32_t *seg, int32_t nseg,
                                  int64_t n_agents, const int32_t *gather_row, double *conc, int64_t conc_ld,
                                  const int32_t *count_row, const int64_t *counts, int64_t counts_ld,
                                  double binvol_avogadro, vk_stream_t stream) {
    if (!field || !work0 || !work1 || n_fields < 1 || ny <= 0 || rows <= 0 || n_sub < 0 ||
        (int64_t)rows * ny > field_stride || (int64_t)rows * ny >= INT32_MAX || n_agents < 0 ||
        n_agents >= INT32_MAX || nseg != (ny + 15) / 16 || (n_agents > 0 && (!bin_lin || !seg)) || !gather_row ||
        !count_row) {
        vk::set_error("vk_diffuse_coupled: bad arguments");
        return VK_ERR_ARG;
    }
    VkPsCouple cp = {};
    cp.bins = bin_lin;
    cp.seg = seg;
    cp.nseg = nseg;
    cp.n = (int32_t)n_agents;
    cp.gdst = conc;
    cp.gld = conc_ld;
    cp.counts = counts;
    cp.cld = counts_ld;
    cp.bva = binvol_avogadro;
    if (n_fields > VK_COUPLE_MAX_FIELDS) {
        vk::set_error("vk_diffuse_coupled: at most 8 planes");
        return VK_ERR_LIMIT;
    }
    for (int f = 0; f < n_fields; ++f) {
        if (gather_row[f] >= 127 || count_row[f] >= 127 || (gather_row[f] >= 0 && (!conc || conc_ld < n_agents)) ||
            (count_row[f] >= 0 && (!counts || counts_ld < n_agents))) {
            vk::set_error("vk_diffuse_coupled: bad gather / count rows");
            return VK_ERR_ARG;
        }
        cp.grow[f] = (int8_t)(gather_row[f] < 0 ? -1 : gather_row[f]);
        cp.crow[f] = (int8_t)(count_row[f] < 0 ? -1 : count_row[f]);
    }
    const vk_plan::Call c = {0, rows, 0, rows, 1, 1, 0, n_sub, n_sub, VK_PART_ALL, 0,
                             n_agents > 0 ? VK_PLAN_COUPLED_AGENTS : VK_PLAN_COUPLED};
    return run_plan("vk_diffuse_coupled", c, field, work0, work1, n_fields, field_stride, ny, coeff_dt, uniform, &cp, stream);
}

extern "C" int vk_diffuse_delta(double *field, double *work0, double *work1, double *delta, int32_t n_fields,
                                int64_t field_stride, int32_t ny, int32_t row_lo, int32_t row_hi, int32_t lo_min,
                                int32_t hi_max, int32_t edge_top, int32_t edge_bot, int32_t sub_begin,
                                int32_t sub_count, int32_t n_sub, double coeff_dt, const double *uniform,
                                vk_stream_t stream) {
    if (!delta || sub_count < 1 || sub_begin + sub_count != n_sub) {
        vk::set_error("vk_diffuse_delta: needs a delta buffer and the call must end at the last substep");
        return VK_ERR_ARG;
    }
    // substeps before the last: the ordinary passes, none of them final (n_sub + 1),
    // over one more row on each side (the last substep's neighbours) where there is one
    if (sub_count > 1) {
        const int rc = vk_diffuse(field, work0, work1, n_fields, field_stride, ny, std::max(lo_min, row_lo - 1),
                                  std::min(hi_max, row_hi + 1), lo_min, hi_max, edge_top, edge_bot, sub_begin,
                                  sub_count - 1, n_sub + 1, coeff_dt, uniform, stream);
        if (rc) return rc;
    }
    const int jl = n_sub - 1;
    double *work[2] = {work0, work1};
    const double *src = jl == 0 ? field : work[(jl - 1) & 1];
    const int top_reflect = edge_top ? lo_min : -1;
    const int bot_reflect = edge_bot ? hi_max - 1 : 0x7fffffff;
    dim3 grid((ny + ST_BX - 1) / ST_BX, (row_hi - row_lo + ST_RB - 1) / ST_RB, n_fields);
    hipLaunchKernelGGL(k_diffuse_substep, grid, dim3(ST_BX), 0, (hipStream_t)stream, src, delta, field, field_stride,
                       ny, row_lo, row_hi, top_reflect, bot_reflect, coeff_dt, uniform, 1);
    return vk::launch_check("vk_diffuse_delta");
}

// ---------------------------------------------------------------------------
// uniform-plane test (diffusion_field.py:401-404: a field whose values are all
// equal gets a zero delta).  Summary per plane: sum[2f] == sum[2f+1] iff the
// owned rows hold one value (both = that value); otherwise (-inf, +inf).  The
// summary min/max-reduces across ranks (distributed.make_uniform_allreduce).
// A fixed grid of VK_UNIFORM_BLOCKS blocks per plane strides over the plane
// in 16-KiB chunks and stops at its first chunk holding a second value, so a
// non-uniform plane costs one chunk per block (a few microseconds); every
// block writes its own flag (no shared address is polled or stored to), and
// a one-block pass folds the flags into the summary.
// ---------------------------------------------------------------------------

constexpr int UN_PER_THREAD = 8;
constexpr int UN_CHUNK = 256 * UN_PER_THREAD;

__global__ __launch_bounds__(256) void k_uniform_probe(const double *__restrict__ fields, int64_t field_stride,
                                                       int64_t off, int64_t count, int32_t *__restrict__ found) {
    const int f = blockIdx.y;
    const double *p = fields + (int64_t)f * field_stride + off;
    const double v0 = p[0];
    int hit = !(v0 == v0);                       // a NaN plane is non-uniform
    for (int64_t c = blockIdx.x; !hit && c * UN_CHUNK < count; c += gridDim.x) {
        const int64_t base = c * UN_CHUNK + threadIdx.x;
        bool diff = false;
#pragma unroll
        for (int k = 0; k < UN_PER_THREAD; ++k) {
            const int64_t i = base + (int64_t)k * 256;
            if (i < count) diff |= !(p[i] == v0);
        }
        hit = __syncthreads_or(diff);
    }
    if (threadIdx.x == 0) found[(int64_t)f * gridDim.x + blockIdx.x] = hit;
}

__global__ __launch_bounds__(256) void k_uniform_finish(const double *__restrict__ fields, int64_t field_stride,
                                                        int64_t off, const int32_t *__restrict__ found,
                                                        int n_blocks, double *__restrict__ sum) {
    const int f = blockIdx.x;
    int hit = 0;
    for (int b = threadIdx.x; b < n_blocks; b += 256) hit |= found[(int64_t)f * n_blocks + b];
    hit = __syncthreads_or(hit);
    if (threadIdx.x == 0) {
        const double v0 = fields[(int64_t)f * field_stride + off];
        sum[2 * f] = hit ? -INFINITY : v0;
        sum[2 * f + 1] = hit ? INFINITY : v0;
    }
}

extern "C" int vk_field_uniform(const double *fields, int32_t n_fields, int64_t field_stride, int32_t ny,
                                int32_t row_lo, int32_t row_hi, double *summary, int32_t *scratch,
                                vk_stream_t stream) {
    if (!fields || !summary || !scratch || n_fields < 0 || n_fields > 65535 || ny <= 0 || row_lo < 0 ||
        row_hi <= row_lo || (int64_t)row_hi * ny > field_stride) {
        vk::set_error("vk_field_uniform: bad arguments");
        return VK_ERR_ARG;
    }
    if (n_fields == 0) return VK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t off = (int64_t)row_lo * ny;
    const int64_t count = (int64_t)(row_hi - row_lo) * ny;
    const int blocks = (int)std::min<int64_t>(VK_UNIFORM_BLOCKS, (count + UN_CHUNK - 1) / UN_CHUNK);
    hipLaunchKernelGGL(k_uniform_probe, dim3(blocks, n_fields), dim3(256), 0, s, fields, field_stride, off, count,
                       scratch);
    hipLaunchKernelGGL(k_uniform_finish, dim3(n_fields), dim3(256), 0, s, fields, field_stride, off, scratch, blocks,
                       summary);
    return vk::launch_check("k_uniform_probe");
}

// ---------------------------------------------------------------------------
// agent <-> field coupling
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_gather(const double *__restrict__ fields, int64_t field_stride,
                                                const int32_t *__restrict__ bin_lin, int64_t n,
                                                const int32_t *__restrict__ map_field,
                                                const int32_t *__restrict__ map_row, int n_map,
                                                double *dst, int64_t ld) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const int64_t b = bin_lin[a];
    for (int i = 0; i < n_map; ++i)
        dst[(int64_t)ldc(map_row, i) * ld + a] = fields[(int64_t)ldc(map_field, i) * field_stride + b];
}

extern "C" int vk_gather(const double *fields, int64_t field_stride, const int32_t *bin_lin, int64_t n,
                         const int32_t *map_field, const int32_t *map_row, int32_t n_map, double *dst,
                         int64_t ld, vk_stream_t stream) {
    if (n < 0 || ld < n || n_map < 0 || (n > 0 && n_map > 0 && (!fields || !bin_lin || !map_field || !map_row || !dst))) {
        vk::set_error("vk_gather: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0 || n_map == 0) return VK_OK;
    hipLaunchKernelGGL(k_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fields,
                       field_stride, bin_lin, n, map_field, map_row, n_map, dst, ld);
    return vk::launch_check("k_gather");
}

// count / (bin_volume * N_A) mol/L, to mmol/L (registry.py:179-182)
__device__ __forceinline__ double exchange_mM(int64_t count, double binvol_avogadro) {
    return ((double)count / binvol_avogadro) * 1000.0;
}

__global__ __launch_bounds__(256) void k_exchange_sorted(double *__restrict__ fields, int64_t field_stride,
                                                         const int32_t *__restrict__ occ_bin,
                                                         const int32_t *__restrict__ occ_ptr,
                                                         const int32_t *__restrict__ occ_agent, int n_occ,
                                                         const int64_t *__restrict__ counts, int64_t ld,
                                                         const int32_t *__restrict__ map_count,
                                                         const int32_t *__restrict__ map_field, int n_map,
                                                         double bva) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_occ) return;
    const int64_t bin = occ_bin[b];
    const int k0 = occ_ptr[b], k1 = occ_ptr[b + 1];
    for (int i = 0; i < n_map; ++i) {
        double *p = fields + (int64_t)ldc(map_field, i) * field_stride + bin;
        const int64_t *cr = counts + (int64_t)ldc(map_count, i) * ld;
        double v = *p;
        for (int k = k0; k < k1; ++k) v = v + exchange_mM(cr[occ_agent[k]], bva);
        *p = v;
    }
}

extern "C" int vk_exchange_sorted(double *fields, int64_t field_stride, const int32_t *occ_bin,
                                  const int32_t *occ_ptr, const int32_t *occ_agent, int32_t n_occ,
                                  const int64_t *counts, int64_t ld, const int32_t *map_count,
                                  const int32_t *map_field, int32_t n_map, double binvol_avogadro,
                                  vk_stream_t stream) {
    if (n_occ < 0 || n_map < 0 ||
        (n_occ > 0 && n_map > 0 && (!fields || !occ_bin || !occ_ptr || !occ_agent || !counts || !map_count || !map_field))) {
        vk::set_error("vk_exchange_sorted: bad arguments");
        return VK_ERR_ARG;
    }
    if (n_occ == 0 || n_map == 0) return VK_OK;
    hipLaunchKernelGGL(k_exchange_sorted, dim3((unsigned)((n_occ + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, fields, field_stride, occ_bin, occ_ptr, occ_agent, n_occ, counts,
                       ld, map_count, map_field, n_map, binvol_avogadro);
    return vk::launch_check("k_exchange_sorted");
}

// The same per-bin sums from a device-side occupancy (vk_occupancy_sort): thread k is
// the head of a bin's segment iff sorted_bin[k] differs from sorted_bin[k - 1]; a head
// walks its segment and does what k_exchange_sorted does for one bin.  No occupied-bin
// count is needed, so nothing is read back to the host.
__global__ __launch_bounds__(256) void k_exchange_ordered(double *__restrict__ fields, int64_t field_stride,
                                                          const int32_t *__restrict__ sorted_bin,
                                                          const int32_t *__restrict__ order, int n,
                                                          const int64_t *__restrict__ counts, int64_t ld,
                                                          const int32_t *__restrict__ map_count,
                                                          const int32_t *__restrict__ map_field, int n_map,
                                                          double bva) {
    const int k0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (k0 >= n) return;
    const int32_t bin = sorted_bin[k0];
    if (k0 > 0 && sorted_bin[k0 - 1] == bin) return;
    int k1 = k0 + 1;
    while (k1 < n && sorted_bin[k1] == bin) ++k1;
    for (int i = 0; i < n_map; ++i) {
        double *p = fields + (int64_t)ldc(map_field, i) * field_stride + bin;
        const int64_t *cr = counts + (int64_t)ldc(map_count, i) * ld;
        double v = *p;
        for (int k = k0; k < k1; ++k) v = v + exchange_mM(cr[order[k]], bva);
        *p = v;
    }
}

extern "C" int vk_exchange_ordered(double *fields, int64_t field_stride, const int32_t *sorted_bin,
                                   const int32_t *order, int64_t n, const int64_t *counts, int64_t ld,
                                   const int32_t *map_count, const int32_t *map_field, int32_t n_map,
                                   double binvol_avogadro, vk_stream_t stream) {
    if (n < 0 || n >= INT32_MAX || ld < n || n_map < 0 ||
        (n > 0 && n_map > 0 && (!fields || !sorted_bin || !order || !counts || !map_count || !map_field))) {
        vk::set_error("vk_exchange_ordered: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0 || n_map == 0) return VK_OK;
    hipLaunchKernelGGL(k_exchange_ordered, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       fields, field_stride, sorted_bin, order, (int)n, counts, ld, map_count, map_field, n_map,
                       binvol_avogadro);
    return vk::launch_check("k_exchange_ordered");
}

__global__ __launch_bounds__(256) void k_exchange_atomic(double *__restrict__ fields, int64_t field_stride,
                                                         const int32_t *__restrict__ bin_lin, int64_t n,
                                                         const int64_t *__restrict__ counts, int64_t ld,
                                                         const int32_t *__restrict__ map_count,
                                                         const int32_t *__restrict__ map_field, int n_map,
                                                         double bva) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const int64_t b = bin_lin[a];
    for (int i = 0; i < n_map; ++i) {
        const int64_t c = counts[(int64_t)ldc(map_count, i) * ld + a];
        if (c != 0)
            unsafeAtomicAdd(fields + (int64_t)ldc(map_field, i) * field_stride + b, exchange_mM(c, bva));
    }
}

extern "C" int vk_exchange_atomic(double *fields, int64_t field_stride, const int32_t *bin_lin, int64_t n,
                                  const int64_t *counts, int64_t ld, const int32_t *map_count,
                                  const int32_t *map_field, int32_t n_map, double binvol_avogadro,
                                  vk_stream_t stream) {
    if (n < 0 || ld < n || n_map < 0 ||
        (n > 0 && n_map > 0 && (!fields || !bin_lin || !counts || !map_count || !map_field))) {
        vk::set_error("vk_exchange_atomic: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0 || n_map == 0) return VK_OK;
    hipLaunchKernelGGL(k_exchange_atomic, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       fields, field_stride, bin_lin, n, counts, ld, map_count, map_field, n_map,
                       binvol_avogadro);
    return vk::launch_check("k_exchange_atomic");
}

__global__ __launch_bounds__(256) void k_bin_sites(const double *__restrict__ loc, int64_t n, int64_t ld, int nx,
                                                   int ny, double bx, double by, int row_offset,
                                                   int32_t *__restrict__ bin_lin, int32_t *__restrict__ ix_out) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    int ix;
    bin_lin[a] = bin_site_lin(loc[a], loc[ld + a], nx, ny, bx, by, row_offset, &ix);
    if (ix_out) ix_out[a] = ix;
}

extern "C" int vk_bin_sites(const double *loc, int64_t n, int64_t ld, int32_t nx, int32_t ny, double bound_x,
                            double bound_y, int32_t row_offset, int32_t *bin_lin, int32_t *ix_out,
                            vk_stream_t stream) {
    if (n < 0 || ld < n || nx <= 0 || ny <= 0 || (n > 0 && (!loc || !bin_lin))) {
        vk::set_error("vk_bin_sites: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0) return VK_OK;
    hipLaunchKernelGGL(k_bin_sites, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, loc, n,
                       ld, nx, ny, bound_x, bound_y, row_offset, bin_lin, ix_out);
    return vk::launch_check("k_bin_sites");
}
