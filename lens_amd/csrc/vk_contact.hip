// Colony mechanics on MI355X (gfx950): growing capsules push each other apart.
//
// THIS ENGINE'S OWN contact model, not the reference's.  The reference resolves overlaps
// with its `multibody` process (vivarium/processes/multibody_physics.py), a pymunk
// rigid-body simulation with an impulse solver; no parity with its trajectories is claimed.
// What is kept from the reference is what feeds this: the capsule geometry of DeriveGlobals
// (length, width) and the daughter placement of division.
//
// Every agent is a 2-D capsule: centre c, axis angle theta, total length L, width w; radius
// r = w / 2, spine half-length h = max(L - w, 0) / 2, spine direction u = (cos, sin) theta.
// One call runs `iterations` Jacobi relaxation iterations.  In an iteration every agent reads
// the same snapshot of all agents; agent i visits every j != i of the 3 x 3 grid cells around
// its own in ascending (cell, key) order, finds the closest points of the two spines, and for
// an overlap delta = 2 r - d > 0 accumulates a push of 0.5 * stiffness * delta along the
// normal and the turn that push makes about its centre (12 / L^2: the rotational-to-
// translational mobility ratio of a uniformly dragged rod).  The summed push is capped at
// max_push, the turn at +-max_turn, optional Gaussian jitter is added, and the centre is
// clamped into [0, bound) -- the clamp the motility walls end with.
//
// The neighbour order is part of the result (floating-point sums), which is why it is fixed
// by (cell, key) and not by storage order or launch geometry, and why the unit keeps
// -ffp-contract=off like the rest of the library.
//
// Neighbour search: a uniform grid of gx x gy cells with edge bound / g >= max_length.  Two
// capsules can touch only when their centres are closer than (L_i + L_j) / 2 <= max_length,
// so 3 x 3 cells suffice.  An agent longer than a cell edge breaks that; the kernel ORs bit 0
// into the caller's flag word and still runs.  Per iteration, all on the caller's stream:
//   k_contact_cells   linear cell cx * gy + cy per agent (+ the too-long flag)
//   vk_occupancy_sort the library's (bin, key) radix sort, with cell as the bin
//   k_contact_pack    sorted slot k := {x, y, theta, L} and {cos, sin} of agent order[k],
//                     its key, and the cell_start / cell_end tables where sorted_cell changes
//   k_contact_relax   one thread per sorted slot; cells (cx', cy-1 .. cy+1) are adjacent in
//                     the sorted array, so an agent reads three contiguous runs.  Writes the
//                     agent's own column; `packed` is the snapshot, so the write is in place.
// The last iteration also writes bin_lin / bin_ix with vk_bin_sites' arithmetic.  The cells and
// pack kernels and the closest-point routine live in vk_capsule_grid.h, which the colony
// metrics (vk_colonies.hip) include too.
//
// Channels (vk_contact_step_channels, the reference's mother machine: pymunk_multibody.py:
// 218-230, multibody_physics.py:232-250): vertical lines at x = space * l, l < n_lines, from the
// floor to `height`.  k_contact_relax<true> projects each agent after its push and jitter and
// before the plane's clamp -- an agent above `height` is left alone and flagged in outflow[],
// any other is turned until its spine fits its channel and its centre is clamped between the
// lines -- a closed form per agent: no loop over lines, no LDS, nothing shared.  This too is
// the engine's own law, not pymunk's segments.  k_contact_relax<false> is the kernel without.
//
// Hazards: no kernel waits on another workgroup, nothing is polled, every loop is bounded by
// cell_end - cell_start, and the only atomic is the atomicOr on the flag word.
//
// Jitter draws: philox_uniform(seed, s, key, 1, j), j = 0..3 (depth word 1: motility uses 0),
// Box-Muller in pairs.  s = counter[0] + the iteration index; the call then advances
// counter[0] by `iterations` in stream order, so a captured graph replays successive steps.

#include <math.h>
#include <stdint.h>

#include "vk_bin.h"
#include "vk_capsule_grid.h"
#include "vk_internal.h"
#include "vk_philox.h"

// scratch layout: cell[n] i32 | order[n] i32 | sorted_cell[n] i32 | skey[n] u32 |
// packed[n] 32 B | dir[n] 16 B | cell_start[g] i32 | cell_end[g] i32 | the sort's scratch
static inline int64_t contact_fixed_bytes(int64_t n, int64_t g) {
    return 4 * align256(n * 4) + align256(n * 32) + align256(n * 16) + 2 * align256(g * 4);
}

extern "C" int64_t vk_contact_scratch_bytes(int64_t n, int64_t n_grid_cells) {
    if (n <= 0 || n_grid_cells <= 0) return 0;
    return contact_fixed_bytes(n, n_grid_cells) + vk_occupancy_scratch_bytes(n) + 256;
}

#define CONTACT_CAND 16   // candidates a lane collects before it solves them

// CH: the mother machine's channel walls and outflow flag (vk_contact_step_channels); the
// instantiation without them is the kernel as it was.
template <bool CH>
__global__ __launch_bounds__(256) void k_contact_relax(
    vk_contact_params p, int n, int64_t ld, const contact_slot *__restrict__ packed, const double2 *__restrict__ dir,
    const uint32_t *__restrict__ skey, const int32_t *__restrict__ order, const int32_t *__restrict__ sorted_cell,
    const int32_t *__restrict__ cell_start, const int32_t *__restrict__ cell_end, const uint64_t *__restrict__ counter,
    int iteration, double bx_below, double by_below, double *__restrict__ loc, double *__restrict__ angle, int nx,
    int ny, double bx, double by, int32_t *__restrict__ bin_lin, int32_t *__restrict__ bin_ix,
    vk_contact_channels ch, int32_t *__restrict__ outflow) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const contact_slot me = packed[k];
    const double2 ui = dir[k];
    const uint32_t key_i = skey[k];
    const double r = p.width / 2.0;
    const double hi = fmax(me.L - p.width, 0.0) / 2.0;
    const int c = sorted_cell[k];
    const int cx = c / p.gy, cy = c - cx * p.gy;
    const int y0 = cy > 0 ? cy - 1 : 0, y1 = cy < p.gy - 1 ? cy + 1 : p.gy - 1;
    double dcx = 0.0, dcy = 0.0, dth = 0.0;
    // one neighbour's contribution, in the order the neighbours are visited
    auto contact = [&](int j) {
        const contact_slot o = packed[j];
        const double2 uj = dir[j];
        const double hj = fmax(o.L - p.width, 0.0) / 2.0;
        // closest points of the two spines (vk_capsule_grid.h)
        double rx, ry, s, vx, vy;
        const double d = contact_closest(me, ui, hi, o, uj, hj, rx, ry, s, vx, vy);
        const double delta = (r + r) - d;
        if (!(delta > 0.0)) return;
        double nxn, nyn;
        if (d > 1e-9) {
            nxn = vx / d;
            nyn = vy / d;
        } else {
            const double rho = sqrt(rx * rx + ry * ry);
            if (rho > 1e-9) {          // crossing spines: along the centre line
                nxn = rx / rho;
                nyn = ry / rho;
            } else {                   // coincident centres: the key order decides
                nxn = key_i < skey[j] ? 1.0 : -1.0;
                nyn = 0.0;
            }
        }
        const double mag = 0.5 * p.stiffness * delta;
        const double px = mag * nxn, py = mag * nyn;
        dcx += px;
        dcy += py;
        dth += ((s * ui.x) * py - (s * ui.y) * px) * 12.0 / (me.L * me.L);
    };
    // Two phases, because the kernel is bound by VALU issue and only one
    // visited pair in ten is within reach: a lane first collects the neighbours that can touch
    // it (a cheap test on the centre distance) in its own column of an LDS list, then solves
    // them, so that the lanes of a wave run the closest-point solve together instead of each
    // waiting through the other lanes' hits.  The list keeps the visiting order and is solved
    // whenever it is full, so the sums are those of the single loop, bit for bit.  No barrier:
    // a lane reads only what it wrote.
    __shared__ int32_t cand[CONTACT_CAND][256];
    const int lane = threadIdx.x;
    int nc = 0;
    for (int xx = (cx > 0 ? cx - 1 : 0); xx <= (cx < p.gx - 1 ? cx + 1 : p.gx - 1); ++xx) {
        // cells (xx, y0 .. y1) are adjacent in the sorted array: one run, in ascending
        // (cell, key) order (an empty cell has start == end == 0 and contributes nothing)
        for (int cc = xx * p.gy + y0; cc <= xx * p.gy + y1; ++cc) {
            const int j1 = cell_end[cc];
            for (int j = cell_start[cc]; j < j1; ++j) {
                if (j == k) continue;
                const contact_slot o = packed[j];
                const double hj = fmax(o.L - p.width, 0.0) / 2.0;
                const double rx = me.x - o.x, ry = me.y - o.y;
                // exact: a spine point is within h of its centre, so d >= |rho| - hi - hj;
                // with |rho| more than 5e-7 of the reach beyond hi + hj + 2 r the overlap is
                // negative by far more than rounding, and the pair adds nothing
                const double reach = hi + hj + (r + r);
                if (rx * rx + ry * ry > reach * reach * 1.000001) continue;
                cand[nc][lane] = j;
                if (++nc == CONTACT_CAND) {
                    for (int i = 0; i < CONTACT_CAND; ++i) contact(cand[i][lane]);
                    nc = 0;
                }
            }
        }
    }
    for (int i = 0; i < nc; ++i) contact(cand[i][lane]);
    const double m = sqrt(dcx * dcx + dcy * dcy);
    if (m > p.max_push) {
        const double scale = p.max_push / m;
        dcx *= scale;
        dcy *= scale;
    }
    dth = clampd(dth, -p.max_turn, p.max_turn);
    double x = me.x + dcx, y = me.y + dcy, th = me.theta + dth;
    if (p.jitter != 0.0 || p.jitter_angle != 0.0) {
        const uint64_t step = counter[0] + (uint64_t)iteration;
        const double u0 = philox_uniform(p.seed, step, (int32_t)key_i, 1, 0);
        const double u1 = philox_uniform(p.seed, step, (int32_t)key_i, 1, 1);
        const double u2 = philox_uniform(p.seed, step, (int32_t)key_i, 1, 2);
        const double u3 = philox_uniform(p.seed, step, (int32_t)key_i, 1, 3);
        const double r0 = sqrt(-2.0 * log(1.0 - u0)), r1 = sqrt(-2.0 * log(1.0 - u2));   // Box-Muller
        x += p.jitter * (r0 * cos(6.283185307179586 * u1));
        y += p.jitter * (r0 * sin(6.283185307179586 * u1));
        th += p.jitter_angle * (r1 * cos(6.283185307179586 * u3));
    }
    const int a = order[k];
    if constexpr (CH) {
        // The channel walls: a projection, after the push and the jitter.  An agent above the
        // channels is left alone and flagged (iteration 0 writes the flag, later ones OR into
        // it).  Any other stays in the channel its snapshot centre was in: its axis is turned
        // until the spine fits between the two lines, then the centre is clamped so that both
        // spine ends keep r + spacer from them.  Right of the last line the plane's edge stands in.
        const bool out = y > ch.height;
        if (outflow) {
            if (iteration == 0) outflow[a] = out ? 1 : 0;
            else if (out) outflow[a] = 1;
        }
        if (!out) {
            const double cf = floor(me.x / ch.space);
            const int c = !(cf >= 0.0) ? 0 : (cf < (double)ch.n_lines ? (int)cf : ch.n_lines - 1);
            const double wl = (double)c * ch.space + (r + ch.spacer);
            const double wh = c + 1 < ch.n_lines ? (double)(c + 1) * ch.space - (r + ch.spacer) : bx_below;
            double ac = 0.0;      // |cos theta| of the angle the agent ends with
            if (hi > 0.0) {
                const double cs = cos(th), sn = sin(th);
                const double cmax = fmin((wh - wl) / (2.0 * hi), 1.0);
                ac = fabs(cs);
                if (ac > cmax) {
                    th = atan2(copysign(sqrt(1.0 - cmax * cmax), sn), copysign(cmax, cs));
                    ac = cmax;
                }
            }
            const double e = hi * ac;
            x = fmin(fmax(x, wl + e), fmax(wh - e, wl + e));
        }
    }
    x = fmin(fmax(x, 0.0), bx_below);
    y = fmin(fmax(y, 0.0), by_below);
    loc[a] = x;
    loc[ld + a] = y;
    angle[a] = th;
    if (bin_lin) {       // the last iteration: the bins vk_bin_sites would give the new location
        int ix;
        bin_lin[a] = bin_site_lin(x, y, nx, ny, bx, by, 0, &ix);
        if (bin_ix) bin_ix[a] = ix;
    }
}

// after the agents' kernels, in stream order: the next call's first iteration
__global__ void k_contact_advance(uint64_t *counter, uint64_t by) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counter[0] += by;
}

static int contact_step(const vk_contact_params *p, int64_t n, int64_t ld, double *location, double *angle,
                        const double *length, const int64_t *key, uint64_t *counter, int32_t *flags, int32_t nx,
                        int32_t ny, double bound_x, double bound_y, int32_t *bin_lin, int32_t *bin_ix, void *scratch,
                        int64_t scratch_bytes, vk_stream_t stream, const vk_contact_channels *ch, int32_t *outflow) {
    if (!p || n < 0 || n >= INT32_MAX || ld < n || !counter || !flags || nx <= 0 || ny <= 0 || !(bound_x > 0.0) ||
        !(bound_y > 0.0) || (int64_t)nx * ny >= INT32_MAX) {
        vk::set_error("vk_contact_step: bad arguments");
        return VK_ERR_ARG;
    }
    if (p->iterations < 1 || !(p->stiffness > 0.0) || !(p->stiffness <= 1.0) || !(p->width > 0.0) ||
        !(p->max_length >= p->width) || !(p->max_push >= 0.0) || !(p->max_turn >= 0.0) ||
        (!length && !(p->length > 0.0))) {
        vk::set_error("vk_contact_step: iterations >= 1, 0 < stiffness <= 1, 0 < width <= max_length, "
                      "max_push, max_turn >= 0, length > 0");
        return VK_ERR_ARG;
    }
    // the grid: a cell edge of at least max_length on an axis with more than one cell
    if (p->gx < 1 || p->gy < 1 || (int64_t)p->gx * p->gy >= INT32_MAX ||
        (p->gx > 1 && bound_x / p->gx < p->max_length) || (p->gy > 1 && bound_y / p->gy < p->max_length)) {
        vk::set_error("vk_contact_step: the grid must be gx = max(1, floor(bound_x / max_length)) by gy likewise "
                      "(cell edges >= max_length)");
        return VK_ERR_ARG;
    }
    if (ch && (!(ch->height > 0.0) || !(ch->height <= bound_y) || !(ch->spacer >= 0.0) ||
               !(ch->space >= p->width + 2.0 * ch->spacer) || ch->n_lines < 1 ||
               (double)ch->n_lines != floor(bound_x / ch->space))) {
        vk::set_error("vk_contact_step_channels: 0 < height <= bound_y, spacer >= 0, space >= width + 2 spacer, "
                      "n_lines = floor(bound_x / space) >= 1");
        return VK_ERR_ARG;
    }
    if (n == 0) return VK_OK;
    const int64_t g = (int64_t)p->gx * p->gy;
    if (!location || !angle || !bin_lin || !scratch || ((uintptr_t)scratch & 255) ||
        scratch_bytes < vk_contact_scratch_bytes(n, g)) {
        vk::set_error("vk_contact_step: null array, or scratch not 256-B aligned / smaller than "
                      "vk_contact_scratch_bytes(n, gx * gy)");
        return VK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    char *base = (char *)scratch;
    int32_t *cell = (int32_t *)base;
    int32_t *order = (int32_t *)(base + align256(n * 4));
    int32_t *sorted_cell = (int32_t *)(base + 2 * align256(n * 4));
    uint32_t *skey = (uint32_t *)(base + 3 * align256(n * 4));
    base += 4 * align256(n * 4);
    contact_slot *packed = (contact_slot *)base;
    base += align256(n * 32);
    double2 *dir = (double2 *)base;
    base += align256(n * 16);
    int32_t *cell_start = (int32_t *)base;     // cell_end follows: one memset clears both
    int32_t *cell_end = (int32_t *)(base + align256(g * 4));
    base += 2 * align256(g * 4);
    const int64_t sort_bytes = scratch_bytes - contact_fixed_bytes(n, g);
    const double edge_x = bound_x / p->gx, edge_y = bound_y / p->gy;
    const double bx_below = nextafter(bound_x, 0.0), by_below = nextafter(bound_y, 0.0);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    for (int it = 0; it < p->iterations; ++it) {
        const bool last = it == p->iterations - 1;
        hipLaunchKernelGGL(k_contact_cells, grid, block, 0, s, (int)n, ld, location, length, p->length, edge_x,
                           edge_y, p->gx, p->gy, cell, flags);
        int rc = vk::launch_check("k_contact_cells");
        if (rc) return rc;
        rc = vk_occupancy_sort(cell, key, n, g, order, sorted_cell, base, sort_bytes, stream);
        if (rc) return rc;
        rc = vk::hip_check(hipMemsetAsync(cell_start, 0, (size_t)(2 * align256(g * 4)), s), "hipMemsetAsync(cells)");
        if (rc) return rc;
        hipLaunchKernelGGL(k_contact_pack, grid, block, 0, s, (int)n, ld, location, angle, length, p->length, key,
                           order, sorted_cell, packed, dir, skey, cell_start, cell_end);
        rc = vk::launch_check("k_contact_pack");
        if (rc) return rc;
        if (ch)
            hipLaunchKernelGGL(k_contact_relax<true>, grid, block, 0, s, *p, (int)n, ld, packed, dir, skey, order,
                               sorted_cell, cell_start, cell_end, counter, it, bx_below, by_below, location, angle, nx,
                               ny, bound_x, bound_y, last ? bin_lin : (int32_t *)nullptr,
                               last ? bin_ix : (int32_t *)nullptr, *ch, outflow);
        else
            hipLaunchKernelGGL(k_contact_relax<false>, grid, block, 0, s, *p, (int)n, ld, packed, dir, skey, order,
                               sorted_cell, cell_start, cell_end, counter, it, bx_below, by_below, location, angle, nx,
                               ny, bound_x, bound_y, last ? bin_lin : (int32_t *)nullptr,
                               last ? bin_ix : (int32_t *)nullptr, vk_contact_channels{}, (int32_t *)nullptr);
        rc = vk::launch_check("k_contact_relax");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_contact_advance, dim3(1), dim3(64), 0, s, counter, (uint64_t)p->iterations);
    return vk::launch_check("k_contact_advance");
}

extern "C" int vk_contact_step(const vk_contact_params *p, int64_t n, int64_t ld, double *location, double *angle,
                               const double *length, const int64_t *key, uint64_t *counter, int32_t *flags,
                               int32_t nx, int32_t ny, double bound_x, double bound_y, int32_t *bin_lin,
                               int32_t *bin_ix, void *scratch, int64_t scratch_bytes, vk_stream_t stream) {
    return contact_step(p, n, ld, location, angle, length, key, counter, flags, nx, ny, bound_x, bound_y, bin_lin,
                        bin_ix, scratch, scratch_bytes, stream, nullptr, nullptr);
}

// vk_contact_step with the mother machine's channels; ch == NULL runs vk_contact_step's own code
extern "C" int vk_contact_step_channels(const vk_contact_params *p, int64_t n, int64_t ld, double *location,
                                        double *angle, const double *length, const int64_t *key, uint64_t *counter,
                                        int32_t *flags, int32_t nx, int32_t ny, double bound_x, double bound_y,
                                        int32_t *bin_lin, int32_t *bin_ix, void *scratch, int64_t scratch_bytes,
                                        const vk_contact_channels *ch, int32_t *outflow, vk_stream_t stream) {
    return contact_step(p, n, ld, location, angle, length, key, counter, flags, nx, ny, bound_x, bound_y, bin_lin,
                        bin_ix, scratch, scratch_bytes, stream, ch, ch ? outflow : nullptr);
}
