// The pass plan of a diffusion call (vk_diffuse, vk_diffuse_part, vk_diffuse_coupled):
// which fused passes run, in order, each with its depth, the buffer it reads and
// the one it writes, its rows and its kernel family.  Pure host code -- no HIP header,
// no global: vk_lattice.hip fills the settings from vk_set_stencil_*, plans, and turns
// each pass into its launch; vk_diffuse_plan hands the same list to callers and to the
// CPU tests (tests/test_pass_plan_host.py, tests/test_band_plan_host.py).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "vk_kinetics.h"

namespace vk_plan {

struct Settings {
    int mode;     // vk_set_stencil_mode: 0 = exact, 1 = tolerance
    int depth;    // vk_set_stencil_depth: odd 1..15, or 10
    int kernel;   // vk_set_stencil_kernel's variant
    int rows;     // ... and its rows per wave tile (0 = auto); the launchers' tile_rows, no part of the plan
    int bands;    // vk_set_stencil_bands: 0 = automatic rule, 1 = off, 2 = forced (plan_lanes only)
    int top_rows; // ... and the forced top band's rows in the first pass, m_0
};

// A call's geometry as vk_diffuse_part takes it; coupled: VK_PLAN_* (vk_diffuse_coupled's
// whole-plane step: rows [0, row_hi), both edges reflected, every substep).
struct Call {
    int row_lo, row_hi, lo_min, hi_max, edge_top, edge_bot, sub_begin, sub_count, n_sub, part, interior_passes, coupled;
};

inline bool geometry_ok(const Call &c) {
    return c.row_lo >= c.lo_min && c.row_hi <= c.hi_max && c.row_lo < c.row_hi && c.sub_begin >= 0 && c.sub_count >= 0 &&
           c.sub_begin + c.sub_count <= c.n_sub;
}

// The odd pass depths of sub_count substeps: the fewest odd depths <= the set depth
// that sum to the count (a sum of P odd numbers has the parity of P), as even as
// possible -- e.g. 100 = 8x9 + 4x7 rather than 11x9 + a lone single-substep pass.
inline std::vector<int> odd_depths(int set_depth, int sub_count) {
    const int depth = set_depth == 10 ? 9 : std::min(set_depth | 1, 15);
    int passes = (sub_count + depth - 1) / depth;
    if ((passes & 1) != (sub_count & 1)) ++passes;
    std::vector<int> ks;
    for (int j = 0, left = passes; j < sub_count; --left) {
        const int rem = sub_count - j;   // rem has the parity of `left`
        int k = (rem + left - 1) / left;
        if ((k & 1) == 0) ++k;
        if (k > depth) k = depth;
        while (k > 1 && rem - k < left - 1) k -= 2;
        ks.push_back(k);
        j += k;
    }
    return ks;
}

// The kernel family of a pass of k substeps.  `base`: the pass is handed the step-start
// field; `strip`: a short edge strip of vk_diffuse_part, latency-bound, which runs
// faster as single-wave tiles of a few rows than as the stage-split or aligned pass.
inline int kernel_of(const Settings &s, int k, bool base, int couple, bool strip) {
    if (k == 1) return VK_PASS_SINGLE;
    if (s.mode == 1 && k <= 11 && ((k & 1) || k == 10)) {
        // tolerance mode, pair-sum passes: instantiated for k = 3, 5, 7, 9, 10, 11.  The
        // stage-split pass (variant 40) carries no agent coupling.
        if (k != 10) return VK_PASS_PS;
        if (s.kernel == 40 && !strip && !couple) return VK_PASS_SP;
        return s.kernel == 70 && !strip ? VK_PASS_PS10_ALIGNED : VK_PASS_PS10;
    }
    // the exact mode's 10-deep pass, and its variant 6 (streaming stores)
    if (k == 10 || ((s.kernel == 6 || s.kernel >= 20) && (k == 7 || k == 9 || k == 11))) return VK_PASS_WL6NT;
    // other depths (and variants 2 / 3): the plain-store wave tiles; a pass that also
    // streams the base plane keeps the shallow row prefetch (3 waves per SIMD)
    return (s.kernel == 2 || base) ? VK_PASS_WL3 : VK_PASS_WL6;
}

// The state before substep j lives in work[(j-1) & 1] (the field for j == 0, and
// after the last substep): the rotation halo exchanges between blocks rely on
// (Lattice.state_buffer).
inline int state_buffer(int j) { return j == 0 ? VK_BUF_FIELD : VK_BUF_WORK0 + ((j - 1) & 1); }

// Destination buffers of a block of P 10-deep passes, or empty.  In the tolerance mode
// the final pass writes the field without reading it back, so when the block ends the
// step the field is a third buffer (its step-start values are not needed once the first
// pass has read them); the exact mode's final pass re-reads the step-start field, so
// there the field is never scratch.  The block starts in state_buffer(sub_begin) and
// ends in the buffer the rotation expects after it.  Buffers are assigned backwards
// from that target: each pass writes one its source is not (a block inside the step
// starts and ends in the same work buffer, so it needs an even number of passes).
inline std::vector<int> ten_deep_buffers(const Settings &s, const Call &c, int P) {
    const bool ends_step = c.sub_begin + c.sub_count == c.n_sub;
    const int S = state_buffer(c.sub_begin);
    const int T = ends_step ? VK_BUF_FIELD : state_buffer(c.sub_begin + c.sub_count);
    const int cand[3] = {VK_BUF_WORK0, VK_BUF_WORK1, VK_BUF_FIELD};
    const int nc = (ends_step && s.mode == 1) ? 3 : 2;
    std::vector<int> dsts(P, -1);
    dsts[P - 1] = T;
    for (int p = P - 2; p >= 0; --p) {
        for (int i = 0; i < nc && dsts[p] < 0; ++i)
            if (cand[i] != dsts[p + 1] && (p > 0 || cand[i] != S)) dsts[p] = cand[i];
        if (dsts[p] < 0) return {};
    }
    if (dsts[0] == S) return {};
    return dsts;
}

// The passes of a call, in launch order.  Returns VK_OK, or VK_ERR_LIMIT (and *why)
// where the call has no plan: a part of a block that does not split, a coupled step
// that is not two or more fused passes.  The caller has checked geometry_ok.
inline int plan(const Settings &s, const Call &c, std::vector<vk_pass> &out, const char **why) {
    out.clear();
    const bool halo_top = !c.edge_top && c.row_lo > c.lo_min, halo_bot = !c.edge_bot && c.row_hi < c.hi_max;
    const bool ten_block = s.depth == 10 && c.sub_count % 10 == 0 && c.sub_count > 0;
    if (c.part != VK_PART_ALL && !(ten_block && (halo_top || halo_bot) && c.row_hi - c.row_lo > 2 * c.sub_count)) {
        *why = "the block is not a 10-deep-plan band block with an interior";
        return VK_ERR_LIMIT;
    }
    if (c.sub_count == 0 && !c.coupled) return VK_OK;
    const int last = c.sub_begin + c.sub_count - 1;
    const bool ends_step = last == c.n_sub - 1;
    // rows of the pass ending at substep e (the halo shrinks over the call), its inputs k rows wider
    auto add = [&](int k, int e, int src, int dst, bool base, int lo, int hi, bool strip, int gap_lo, int gap_hi) {
        vk_pass p = {};
        p.k = k, p.src = src, p.dst = dst, p.f0 = base;
        p.lo = lo, p.hi = hi;
        p.in_lo = std::max(c.lo_min, lo - k), p.in_hi = std::min(c.hi_max, hi + k);
        p.gap_lo = gap_lo, p.gap_hi = gap_hi;
        if (c.coupled == VK_PLAN_COUPLED_AGENTS)   // the gather rides on the first pass, the exchange on the last
            p.couple = (e - k + 1 == 0 ? 1 : 0) | (e == c.n_sub - 1 ? 2 : 0);
        p.kernel = gap_lo >= 0 ? VK_PASS_PS10_STRIPS : kernel_of(s, k, base, p.couple, strip);
        out.push_back(p);
    };
    // A block of 10 P substeps as P passes of 10 (a coupled step: in the tolerance mode, two or more)
    const int P = c.sub_count / 10;
    std::vector<int> dsts;
    if (ten_block && P <= 64 && (!c.coupled || (s.mode == 1 && P >= 2))) dsts = ten_deep_buffers(s, c, P);
    if (!dsts.empty()) {
        // part (vk_diffuse_part): the interior of pass p is the rows whose inputs at the
        // block's start are all owned -- [row_lo + 10 (p+1), row_hi - 10 (p+1)) on a side
        // with halo rows -- and the edges are the rest of the pass's rows.  The interior
        // passes read and write only interior rows of each buffer, the edge passes read
        // at most 20 rows into the interior of the pass before, which no later interior
        // pass writes (it starts 10 rows deeper per pass), so the interior of the first m
        // passes can run before any edge pass (while the halo arrives).  Then (part EDGES)
        // the edges of those m passes, and the remaining passes whole.
        const int m = (c.interior_passes <= 0 || c.interior_passes > P) ? P : c.interior_passes;
        for (int p = 0; p < P; ++p) {
            if (c.part == VK_PART_INTERIOR && p >= m) break;
            const int e = c.sub_begin + 10 * p + 9, grow = last - e;
            const int lo = std::max(c.lo_min, c.row_lo - grow), hi = std::min(c.hi_max, c.row_hi + grow);
            const int src = p ? dsts[p - 1] : state_buffer(c.sub_begin);
            // (a coupled step names the base in either mode; the pair-sum passes do not read it)
            const bool base = (s.mode != 1 || c.coupled) && ends_step && p == P - 1;
            const int ilo = halo_top ? c.row_lo + 10 * (p + 1) : lo, ihi = halo_bot ? c.row_hi - 10 * (p + 1) : hi;
            if (c.part == VK_PART_ALL || (c.part == VK_PART_EDGES && p >= m)) {
                add(10, e, src, dsts[p], base, lo, hi, false, -1, -1);
            } else if (c.part == VK_PART_INTERIOR) {
                if (ilo < ihi) add(10, e, src, dsts[p], base, ilo, ihi, false, -1, -1);
            } else if (halo_top && halo_bot && ilo < ihi && s.mode == 1) {
                add(10, e, src, dsts[p], base, lo, hi, true, ilo, ihi);   // both strips as one launch
            } else {
                if (halo_top && lo < ilo) add(10, e, src, dsts[p], base, lo, ilo, true, -1, -1);
                if (halo_bot && ihi < hi) add(10, e, src, dsts[p], base, ihi, hi, true, -1, -1);
            }
        }
        return VK_OK;
    }
    if (c.part != VK_PART_ALL) {
        *why = "no 10-deep buffer plan for this block";
        return VK_ERR_LIMIT;
    }
    // Odd depths: the pass of substeps [j, j+k) reads state_buffer(j) and writes
    // state_buffer(j+k), which differ because k is odd; the pass that ends the step writes
    // the field and is handed it as base.  A pass that both starts from and ends in the
    // field cannot run in place (neighbours would read new values): it writes work0, and
    // its owned rows are copied back.
    const std::vector<int> ks = odd_depths(s.depth, c.sub_count);
    if (c.coupled && (ks.size() < 2 || *std::min_element(ks.begin(), ks.end()) < 2)) {
        *why = "the step is not planned as two or more fused passes";
        return VK_ERR_LIMIT;
    }
    int j = c.sub_begin;
    for (int k : ks) {
        const int e = j + k - 1, grow = last - e;
        const bool final_pass = e == c.n_sub - 1, in_place = final_pass && j == 0;
        const int dst = in_place ? VK_BUF_WORK0 : (final_pass ? VK_BUF_FIELD : state_buffer(e + 1));
        add(k, e, state_buffer(j), dst, final_pass, std::max(c.lo_min, c.row_lo - grow),
            std::min(c.hi_max, c.row_hi + grow), false, -1, -1);
        out.back().copy_back = in_place;
        j += k;
    }
    return VK_OK;
}

// The top band's rows in the first pass, m_0, with which the automatic rule
// (Settings::bands == 0) runs a plan banded, or 0.  Only the shape measured faster
// banded than whole: the 4096-row plane stepping ten aligned 10-deep passes (variant 70,
// the C4 step: 1.170-1.178 against 1.245-1.260 ms per step with the top two fifths,
// m_0 = 1638; 1600-1800 and 2418-2500 rows within 0.02 ms of that, halves in lockstep
// and a top band of 0.35 or less, whose launches fall under the cached-store size, no
// better than whole; DESIGN.md §10, profiles/bands/).
inline int auto_top_rows(const Call &c, const std::vector<vk_pass> &passes) {
    if (c.row_hi - c.row_lo != 4096 || passes.size() != 10) return 0;
    for (const vk_pass &p : passes)
        if (p.kernel != VK_PASS_PS10_ALIGNED) return 0;
    return 2 * 4096 / 5;
}

// The call's passes as plan() lists them, or, for a whole-plane step of P 10-deep
// pair-sum passes, each pass as two launches on two lanes (streams): a top band T_p =
// rows [0, m_p) on lane 0 and a bottom band B_p = [m_p, N) on lane 1, m_p = m_0 - 10 p.
// The boundary climbs by the pass depth, so T_p+1 reads only rows T_p wrote: lane 0 is
// a chain that never waits for lane 1, and B_p+1 (which reads from row m_p - 20) needs
// B_p, its lane's order, and T_p, its `after`.  A later T writes only rows above
// m_p - 10, which a lagging B_p neither reads nor writes, in any buffer.  The tails of
// one lane's launches then run beside the other lane's next launch.  lane[i] and
// after[i] (the index of the pass on the other lane that must have finished, or -1) run
// parallel to `out`; an unbanded plan is all lane 0, after -1.  Unbanded when the
// setting says so, for any other call (a part, a row band, a coupled step, other
// kernels), when T_P-1 would have fewer rows than one pass depth or B_0 none.
inline int plan_lanes(const Settings &s, const Call &c, std::vector<vk_pass> &out, std::vector<int32_t> &lane,
                      std::vector<int32_t> &after, const char **why) {
    const int rc = plan(s, c, out, why);
    lane.assign(out.size(), 0);
    after.assign(out.size(), -1);
    if (rc != VK_OK || s.bands == 1 || out.empty()) return rc;
    const bool whole_step = c.part == VK_PART_ALL && c.edge_top && c.edge_bot && c.row_lo == c.lo_min &&
                            c.row_hi == c.hi_max && c.sub_begin == 0 && c.sub_count == c.n_sub && !c.coupled;
    if (!whole_step) return rc;
    for (const vk_pass &p : out)
        if (p.k != 10 || (p.kernel != VK_PASS_PS10 && p.kernel != VK_PASS_PS10_ALIGNED) || p.copy_back) return rc;
    const int P = (int)out.size(), N = c.row_hi - c.row_lo;
    const int m0 = s.bands == 2 ? s.top_rows : auto_top_rows(c, out);
    if (m0 - 10 * (P - 1) < 10 || m0 >= N) return rc;
    std::vector<vk_pass> banded;
    lane.clear(), after.clear();
    for (int p = 0; p < P; ++p) {
        const int m = c.row_lo + m0 - 10 * p;
        vk_pass t = out[p], b = out[p];
        t.hi = m, t.in_hi = std::min(c.hi_max, m + 10);
        b.lo = m, b.in_lo = std::max(c.lo_min, m - 10);
        banded.push_back(t), lane.push_back(0), after.push_back(-1);
        banded.push_back(b), lane.push_back(1), after.push_back(p ? 2 * (p - 1) : -1);   // B_p after T_p-1
    }
    out.swap(banded);
    return rc;
}

}  // namespace vk_plan
