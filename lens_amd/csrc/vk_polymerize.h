// The polymerization core, as vk_translation_step uses it and vk_transcription_step restates it
// (gfx950): what the reference keeps in one place too (vivarium/library/polymerize.py, stepped by
// both Translation and Transcription).  One agent per lane, one wavefront per workgroup; the packed polymerases of
// a wave sit in LDS as slot[j * 64 + lane], a lane only ever touching her own column.
//
//   pz_stage_list     the key check and the list's way into LDS
//   pz_initiate       the direct-method initiation loop of one sub-interval
//   pz_unocclude      the sweep that reopens what a cleared polymerase occluded
//   pz_store_list     the list, its length and the free polymerases back to HBM
//   pz_advance        the step word's advance, vk_ssa_step's too
//
// A kernel hands in what differs as functors of its own (how a template's propensity is read,
// what a binding edits, what a reopening edits): they are inlined, nothing is switched at run
// time.  Elongation, the affinity vector, the books of the monomers and the LDS layout stay with
// each kernel.  vk_transcription.hip writes the same pieces out itself (its header says why) and
// takes only pz_advance.  The arithmetic, its order and the draw sequence are the ones include/vk_kinetics.h states above
// the two entry points; tests/translation_ref.py and tests/transcription_ref.py restate them
// independently.
//
// Register constraint: functors capture what they read by value, never the
// kernel's model argument by reference, and pz_initiate takes and returns its state by value.
#pragma once

#include <math.h>
#include <stdint.h>

#include "vk_internal.h"
#include "vk_philox.h"

#define PZ_LANES 64

// the status bits of a polymerase step: both public enums, bit for bit
enum { PZ_SLOTS_FULL = 1, PZ_BAD_KEY = 2, PZ_NONFINITE = 4, PZ_OVERFLOW = 8, PZ_MAX_EVENTS = 16 };
static_assert(PZ_SLOTS_FULL == VK_TL_SLOTS_FULL && PZ_SLOTS_FULL == VK_TX_SLOTS_FULL, "status bits");
static_assert(PZ_BAD_KEY == VK_TL_BAD_KEY && PZ_BAD_KEY == VK_TX_BAD_KEY, "status bits");
static_assert(PZ_NONFINITE == VK_TL_NONFINITE && PZ_NONFINITE == VK_TX_NONFINITE, "status bits");
static_assert(PZ_OVERFLOW == VK_TL_OVERFLOW && PZ_OVERFLOW == VK_TX_OVERFLOW, "status bits");
static_assert(PZ_MAX_EVENTS == VK_TL_MAX_EVENTS && PZ_MAX_EVENTS == VK_TX_MAX_EVENTS, "status bits");

// The two factors of a template's propensity besides the free polymerases: a_i = aff * max(x, 0)
struct pz_factors {
    double aff;
    int32_t x;
};

// Agent a's key and list.  key, bits (PZ_BAD_KEY or 0) and run (false: the agent does nothing
// more but the books) are set; the length is returned and entries [0, length) are staged.
__device__ __forceinline__ int pz_stage_list(int32_t *slot, int lane, int64_t a, bool live, int64_t ld, int cap,
                                             const int64_t *__restrict__ keys, const int32_t *__restrict__ slots,
                                             const int32_t *__restrict__ length, int64_t &key, int &bits, bool &run) {
    key = live ? keys[a] : 0;
    bits = 0;
    if (key < 0 || key > (int64_t)INT32_MAX) bits = PZ_BAD_KEY;
    run = live && bits == 0;
    const int n_r = run ? min(max(length[a], 0), cap) : 0;
    for (int j = 0; __any(j < n_r); ++j)
        if (j < n_r) slot[j * PZ_LANES + lane] = slots[(int64_t)j * ld + a];
    return n_r;
}

// The running sum of a_i over the templates, each a_i three FP64 operations in this order; with
// SEARCH also the first template whose running sum passes thr (q stays as it is if none does).
// The running sums are not kept: the search sums the same products again in the same order, which
// gives the same bits (-ffp-contract=off).
template <bool SEARCH, class Propensity>
__device__ __forceinline__ double pz_sum(int T, double pol, double thr, int &q, Propensity propensity) {
    double cum = 0.0;
    for (int i = 0; i < T; ++i) {
        const pz_factors f = propensity(i);
        double a_i = f.aff;
        a_i = a_i * (f.x < 1 ? 0.0 : (double)f.x);
        a_i = a_i * pol;
        cum = cum + a_i;
        if (SEARCH && q < 0 && cum > thr) q = i;
    }
    return cum;
}

// What initiation reads and edits of a lane's step: the free polymerases before elongation, the
// list's length, the initiations and draws so far, the status bits, and whether she still initiates
struct pz_state {
    int32_t pol;
    int n_r, events, bits;
    uint64_t e;
    bool initiates;
};

// Initiation over one sub-interval: the direct method, each lane on her own clock.  propensity(i)
// gives template i's factors; bind(q) edits what a binding to template q edits and returns the
// packed polymerase, which is appended.  Every lane draws every round, and e advances only for the
// active ones.
template <class Propensity, class Bind>
__device__ __forceinline__ pz_state pz_initiate(int32_t *slot, int lane, int T, int cap, double interval,
                                                uint64_t seed, uint64_t step, int64_t key, int max_events,
                                                const pz_state st, Propensity propensity, Bind bind) {
    int32_t pol = st.pol;
    int n_r = st.n_r, events = st.events, bits = st.bits;
    uint64_t e = st.e;
    bool initiates = st.initiates;
    double t_now = 0.0;
    bool active = initiates && pol >= 1;                 // no free polymerase: nothing binds, no draw
    while (__any(active)) {
        const double free_pol = pol < 1 ? 0.0 : (double)pol;
        int q = -1;
        const double total = pz_sum<false>(T, free_pol, 0.0, q, propensity);
        if (active) {
            if (total == 0.0) {
                active = false;                          // nothing can bind: no draw is consumed
            } else if (!isfinite(total)) {
                bits |= PZ_NONFINITE;
                active = initiates = false;
            }
        }
        double u1, u2;
        philox_uniform_pair(seed, step, (int32_t)key, 0, e, u1, u2);
        if (active) e += 1;
        const double tau = -log(1.0 - u1) / total;
        if (active && t_now + tau > interval) active = false;     // the overshooting event is discarded
        pz_sum<true>(T, free_pol, u2 * total, q, propensity);
        // u2 < 1 and cum_(T-1) == total > 0, so u2 * total rounds below total and a q is found
        if (q < 0) q = T - 1;
        if (active) {
            if (n_r >= cap) {
                bits |= PZ_SLOTS_FULL;
                active = initiates = false;
            } else {
                t_now = t_now + tau;
                pol -= 1;
                slot[n_r * PZ_LANES + lane] = bind(q);
                ++n_r;
                if (++events >= max_events) {
                    bits |= PZ_MAX_EVENTS;
                    active = initiates = false;
                }
                if (pol < 1) active = false;
            }
        }
    }
    return pz_state{pol, n_r, events, bits, e, initiates};
}

// Unocclusion: an occluding polymerase whose position (the word >> SHIFT) has reached the
// occlusion length stops occluding, and reopen(t) edits what her template t gets back.
template <int SHIFT, class Reopen>
__device__ __forceinline__ void pz_unocclude(int32_t *slot, int lane, bool run, int n_r, int occlusion,
                                             Reopen reopen) {
    for (int j = 0; __any(run && j < n_r); ++j) {
        if (!run || j >= n_r) continue;
        const uint32_t v = (uint32_t)slot[j * PZ_LANES + lane];
        if ((v & 1u) && (int)(v >> SHIFT) >= occlusion) {
            slot[j * PZ_LANES + lane] = (int32_t)(v & ~1u);
            reopen((int)((v >> 1) & 63u));
        }
    }
}

// The books of the list: its entries, its length and the free polymerases (free_row: her species'
// row of the counts).
__device__ __forceinline__ void pz_store_list(const int32_t *slot, int lane, int64_t a, int64_t ld, int n_r,
                                              int32_t free_pol, int32_t *__restrict__ slots,
                                              int32_t *__restrict__ length, int32_t *__restrict__ free_row) {
    for (int j = 0; j < n_r; ++j) slots[(int64_t)j * ld + a] = slot[j * PZ_LANES + lane];
    length[a] = n_r;
    free_row[a] = free_pol;
}

// After a step on the same stream: the next launch (the next replay of a graph) draws under the
// next step word.
static __global__ void k_step_word_advance(int64_t *step_counter) {
    if (blockIdx.x == 0 && threadIdx.x == 0) step_counter[0] += 1;
}

static inline int pz_advance(int64_t *step_counter, hipStream_t stream) {
    hipLaunchKernelGGL(k_step_word_advance, dim3(1), dim3(64), 0, stream, step_counter);
    return vk::launch_check("k_step_word_advance");
}
