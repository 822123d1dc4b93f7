// Stochastic transcription on MI355X (gfx950): a bounded, ordered RNAP list per agent, one agent
// per lane, one wavefront per workgroup.
//
//   k_transcription_step  stands where the reference runs Transcription.next_update
//                         (vivarium/processes/transcription.py:370-553) with polymerize_step
//                         (vivarium/library/polymerize.py:205-259).  The step is the one
//                         include/vk_kinetics.h states above vk_transcription_step, restated as
//                         Python loops by tests/transcription_ref.py.  The affinity vector,
//                         elongation, read-through, unocclusion and the books are the
//                         reference's; the initiation arithmetic, every Philox draw, the factor
//                         levels from counts / mmol_to_counts and the in-place process order are
//                         THE ENGINE'S OWN (see the header).
//
// The key check, the list's staging and write-back, the initiation loop and the unocclusion sweep are
// written out here, and are what csrc/vk_polymerize.h states once for translation: the same
// arithmetic, order and draws, pinned by tests/transcription_ref.py.  Taken from that header, each of
// them moved this kernel's idle step (empty lists, no free RNAP) above the parent's own timing
// spread, so only the step word's advance is shared.
//
// Layout: each wave stages slot[j][lane] (the packed RNAPs) and one word
// per (promoter, lane) in LDS, a lane only ever touching her own column, so every such access is
// conflict-free and one wave per workgroup needs no barrier but the one after staging.  The list
// crosses HBM once per launch ([slot][ld]: a wave's loads coalesce).
//
// What four monomers allow that translation's 24 do not:
//   - limit[m] lives in four VGPRs, picked by compares on the monomer index, not in LDS;
//   - the sequence can be staged in LDS at 2 bits per base (the flagella chromosome's 36 927 bases
//     are 9.2 KiB), so that the per-lane load at the head of every elongation's dependent chain is
//     an LDS read, not a divergent global byte load.  Measured, the staged words cost more than
//     they save wherever they take a wave of occupancy (flagella fixture, 128 slots: 3 waves per CU
//     instead of 4, 85 against 72 ms), so VK_TX_SEQUENCE_AUTO stages only where they take none;
//     else, and where 64 KiB do not hold them, the global byte table is read.
//
// The (promoter, lane) word is (blocked << 16) | entry: the number of occluding RNAPs and the index
// of the promoter's affinity in the dense table, which is staged in LDS once per wave (fp64 per
// (promoter, lane) would take 32 KiB at 64 promoters).  Thresholds, factor rows, copy numbers and
// the plan are read through wave-uniform addresses (ldc: the scalar cache); the terminators'
// positions and the templates' offsets sit in LDS; strengths and product rows are read per lane only
// at a terminator.

#include <math.h>
#include <stdint.h>

#include "vk_internal.h"
#include "vk_philox.h"
#include "vk_polymerize.h"     // the step word's advance

#define TX_LANES 64
#define TX_LDS_BYTES 65536
#define TX_CU_LDS_BYTES 163840
#define TX_NT VK_TX_MAX_TERMINATORS

__global__ __launch_bounds__(TX_LANES) void k_transcription_step(
    vk_tx_model mdl, int seq_words, int64_t n, int64_t ld, int32_t *__restrict__ slots, int32_t *__restrict__ length,
    int32_t *__restrict__ molecules, int32_t *__restrict__ counts, const double *__restrict__ m2c,
    const int64_t *__restrict__ keys, uint64_t seed, const int64_t *__restrict__ step_counter, int max_events,
    int32_t *__restrict__ events_out, int32_t *__restrict__ status) {
    extern __shared__ __align__(16) unsigned char tx_lds[];
    const int P = mdl.n_templates, M = mdl.n_monomers, cap = mdl.max_slots, NA = mdl.n_affinities;
    double *aff = (double *)tx_lds;                      // [NA]: the dense affinity table, the wave's
    int32_t *slot = (int32_t *)(aff + NA);               // [cap][64]
    int32_t *pw = slot + (size_t)cap * TX_LANES;         // [P][64]: (blocked << 16) | affinity entry
    int32_t *sp = pw + (size_t)P * TX_LANES;             // [P + 1]: the templates' offsets
    int32_t *tp = sp + P + 1;                            // [4 P]: the terminators' relative positions
    uint32_t *sq = (uint32_t *)(tp + TX_NT * P);         // [seq_words]: 2 bits per base, if staged
    const int lane = threadIdx.x;
    const int64_t a = (int64_t)blockIdx.x * TX_LANES + lane;
    const bool live = a < n;
    const int64_t key = live ? keys[a] : 0;
    int bits = 0;
    if (key < 0 || key > (int64_t)INT32_MAX) bits = VK_TX_BAD_KEY;
    bool run = live && bits == 0;            // false: the agent does nothing more but the books
    int n_r = run ? min(max(length[a], 0), cap) : 0;
    for (int j = 0; __any(j < n_r); ++j)
        if (j < n_r) slot[j * TX_LANES + lane] = slots[(int64_t)j * ld + a];
    for (int i = lane; i < NA; i += TX_LANES) aff[i] = mdl.affinity[i];
    for (int i = lane; i <= P; i += TX_LANES) sp[i] = mdl.seq_ptr[i];
    for (int i = lane; i < TX_NT * P; i += TX_LANES) tp[i] = mdl.term_pos[i];
    for (int i = lane; i < seq_words; i += TX_LANES) sq[i] = mdl.seq2[i];
    // the affinity vector, once: every site's state from the factor levels at the start of the launch
    const double per_mmol = run ? m2c[a] : 1.0;
    for (int p = 0; p < P; ++p) {
        int idx = 0;
        for (int s = ldc(mdl.site_ptr, p); s < ldc(mdl.site_ptr, p + 1); ++s) {
            const int j0 = ldc(mdl.thr_ptr, s), j1 = ldc(mdl.thr_ptr, s + 1);
            int state = 0;
            for (int j = j0; j < j1; ++j) {
                const int row = ldc(mdl.thr_species, j);
                const int32_t x = run && (unsigned)row < (unsigned)mdl.n_species ? counts[(int64_t)row * ld + a] : 0;
                const double level = (double)x / per_mmol;
                if (state == 0 && level >= ldc(mdl.thr_value, j)) state = j - j0 + 1;
            }
            idx = idx * (1 + j1 - j0) + state;
        }
        pw[p * TX_LANES + lane] = ldc(mdl.aff_ptr, p) + idx;
    }
    // blocked[p]: the stored RNAPs that are occluding
    for (int j = 0; __any(j < n_r); ++j) {
        if (j >= n_r) continue;
        const uint32_t v = (uint32_t)slot[j * TX_LANES + lane];
        const int t = (int)((v >> 1) & 63u);
        if ((v & 1u) && t < P) pw[t * TX_LANES + lane] += 1 << 16;
    }
    int32_t l0 = 0, l1 = 0, l2 = 0, l3 = 0;  // limit[m]
    if (run) {
        l0 = molecules[a];
        if (M > 1) l1 = molecules[ld + a];
        if (M > 2) l2 = molecules[2 * ld + a];
        if (M > 3) l3 = molecules[3 * ld + a];
    }
    int32_t free_r = run ? counts[(int64_t)mdl.rnap_species * ld + a] : 0;
    __syncthreads();                         // one wave: orders the staging before the lanes' reads
    const uint64_t step = (uint64_t)step_counter[0];
    const bool stepped = run;
    bool initiates = run;                    // false: no more initiation this step
    int events = 0;
    uint64_t e = 0;
    for (int k = 0; k < mdl.n_plan; ++k) {
        const double interval = ldc(mdl.interval, k);
        // 1 the substrate: the free RNAPs before elongation
        int32_t rnaps = free_r, terminated = 0;
        // 2 elongation, in list order, compacting behind the read
        if (ldc(mdl.elongate, k)) {
            int w = 0;
            for (int j = 0; __any(j < n_r); ++j) {
                if (j >= n_r) continue;
                const uint32_t v = (uint32_t)slot[j * TX_LANES + lane];
                const int t = (int)((v >> 1) & 63u);
                uint32_t ti = (v >> 7) & 3u, p = v >> 9;
                bool keep = true;
                if (run && t < P) {
                    const int o = sp[t], len = sp[t + 1] - o;
                    if ((int)p < len) {
                        const int b = o + (int)p;
                        const int m = seq_words ? (int)((sq[b >> 4] >> ((b & 15) * 2)) & 3u) : (int)mdl.seq[b];
                        const int32_t lim = m == 0 ? l0 : m == 1 ? l1 : m == 2 ? l2 : l3;
                        if (m < M && lim > 0) {
                            const int ix = TX_NT * t + (int)ti;
                            const bool at = (int)p + 1 == tp[ix];
                            bool last = false;
                            int i0 = 0, i1 = 0;
                            if (at) {
                                last = (int)ti + 1 >= mdl.n_term[t];
                                i0 = mdl.prod_ptr[ix];
                                i1 = mdl.prod_ptr[ix + 1];
                                bool over = free_r == INT32_MAX;
                                for (int i = i0; i < i1; ++i) {
                                    const int s = mdl.prod_species[i];
                                    if ((unsigned)s < (unsigned)mdl.n_species && counts[(int64_t)s * ld + a] == INT32_MAX)
                                        over = true;
                                }
                                if (over) {
                                    bits |= VK_TX_OVERFLOW;
                                    run = false;
                                    initiates = false;
                                }
                            }
                            if (run) {
                                l0 -= m == 0;
                                l1 -= m == 1;
                                l2 -= m == 2;
                                l3 -= m == 3;
                                p += 1;
                                if (at) {
                                    bool ends = last;
                                    if (!last) {
                                        double u1, u2;
                                        philox_uniform_pair(seed, step, (int32_t)key, 0, e, u1, u2);
                                        e += 1;
                                        const double choice = u1 * mdl.term_from[ix];
                                        ends = choice <= mdl.term_strength[ix];
                                    }
                                    if (ends) {
                                        for (int i = i0; i < i1; ++i) {
                                            const int s = mdl.prod_species[i];
                                            if ((unsigned)s < (unsigned)mdl.n_species) counts[(int64_t)s * ld + a] += 1;
                                        }
                                        free_r += 1;
                                        terminated += 1;
                                        keep = false;
                                    } else {
                                        ti += 1;
                                    }
                                }
                            }
                        }
                    }
                }
                if (keep) {
                    slot[w * TX_LANES + lane] = (int32_t)((p << 9) | (ti << 7) | (v & 127u));
                    ++w;
                }
            }
            n_r = w;
        }
        // 3 initiation: the direct method over the sub-interval, each lane on her own clock
        double t_now = 0.0;
        bool active = initiates && rnaps >= 1;           // no free RNAP: nothing binds, no draw
        while (__any(active)) {
            const double rn = rnaps < 1 ? 0.0 : (double)rnaps;
            double total = 0.0;
            for (int i = 0; i < P; ++i) {
                const uint32_t word = (uint32_t)pw[i * TX_LANES + lane];
                const int32_t x = ldc(mdl.copy, i) - (int32_t)(word >> 16);
                double a_i = aff[word & 0xffffu];
                a_i = a_i * (x < 1 ? 0.0 : (double)x);
                a_i = a_i * rn;
                total = total + a_i;
            }
            if (active) {
                if (total == 0.0) {
                    active = false;                      // nothing can bind: no draw is consumed
                } else if (!isfinite(total)) {
                    bits |= VK_TX_NONFINITE;
                    active = initiates = false;
                }
            }
            double u1, u2;
            philox_uniform_pair(seed, step, (int32_t)key, 0, e, u1, u2);
            if (active) e += 1;
            const double tau = -log(1.0 - u1) / total;
            if (active && t_now + tau > interval) active = false;     // the overshooting event is discarded
            const double thr = u2 * total;
            int q = -1;
            double cum = 0.0;
            for (int i = 0; i < P; ++i) {
                const uint32_t word = (uint32_t)pw[i * TX_LANES + lane];
                const int32_t x = ldc(mdl.copy, i) - (int32_t)(word >> 16);
                double a_i = aff[word & 0xffffu];
                a_i = a_i * (x < 1 ? 0.0 : (double)x);
                a_i = a_i * rn;
                cum = cum + a_i;
                if (q < 0 && cum > thr) q = i;
            }
            // u2 < 1 and cum_(P-1) == total > 0, so u2 * total rounds below total and a q is found
            if (q < 0) q = P - 1;
            if (active) {
                if (n_r >= cap) {
                    bits |= VK_TX_SLOTS_FULL;
                    active = initiates = false;
                } else {
                    t_now = t_now + tau;
                    pw[q * TX_LANES + lane] += 1 << 16;
                    rnaps -= 1;
                    slot[n_r * TX_LANES + lane] = VK_TX_PACK(0, 0, q, 1);
                    ++n_r;
                    if (++events >= max_events) {
                        bits |= VK_TX_MAX_EVENTS;
                        active = initiates = false;
                    }
                    if (rnaps < 1) active = false;
                }
            }
        }
        free_r = rnaps + terminated;
        // 4 unocclusion: the occluding RNAPs that have cleared their promoter reopen it
        for (int j = 0; __any(run && j < n_r); ++j) {
            if (!run || j >= n_r) continue;
            const uint32_t v = (uint32_t)slot[j * TX_LANES + lane];
            if ((v & 1u) && (int)(v >> 9) >= mdl.occlusion) {
                slot[j * TX_LANES + lane] = (int32_t)(v & ~1u);
                const int t = (int)((v >> 1) & 63u);
                if (t < P) pw[t * TX_LANES + lane] -= 1 << 16;
            }
        }
    }
    if (!live) return;
    events_out[a] = events;
    if (bits) status[a] |= bits;
    if (!stepped) return;
    // the books: the list, the free RNAPs, the monomers, ATP and ADP (transcription.py:504-516)
    for (int j = 0; j < n_r; ++j) slots[(int64_t)j * ld + a] = slot[j * TX_LANES + lane];
    length[a] = n_r;
    counts[(int64_t)mdl.rnap_species * ld + a] = free_r;
    int64_t used = 0;
    for (int m = 0; m < M; ++m) {
        const int32_t now = m == 0 ? l0 : m == 1 ? l1 : m == 2 ? l2 : l3, was = molecules[(int64_t)m * ld + a];
        used += (int64_t)was - now;
        if (now != was && m != mdl.atp_row) molecules[(int64_t)m * ld + a] = now;
    }
    if (used) {
        // ATP's own monomer entry is overwritten by the hydrolysis cost: minus the sum, once
        const int64_t atp = (int64_t)molecules[(int64_t)mdl.atp_row * ld + a] - used;
        const int64_t adp = (int64_t)molecules[(int64_t)mdl.adp_row * ld + a] + used;
        if (atp < (int64_t)INT32_MIN || adp > (int64_t)INT32_MAX) status[a] |= VK_TX_OVERFLOW;
        molecules[(int64_t)mdl.atp_row * ld + a] = (int32_t)max(atp, (int64_t)INT32_MIN);
        molecules[(int64_t)mdl.adp_row * ld + a] = (int32_t)min(adp, (int64_t)INT32_MAX);
    }
}

static bool tx_model_ok(const vk_tx_model *m) {
    return m && m->n_templates >= 1 && m->n_templates <= VK_TX_MAX_TEMPLATES && m->n_monomers >= 1 &&
           m->n_monomers <= VK_TX_MAX_MONOMERS && m->n_species >= 1 && m->max_slots >= 1 &&
           m->max_slots <= VK_TX_MAX_SLOTS && m->rnap_species >= 0 && m->rnap_species < m->n_species &&
           m->n_plan >= 0 && m->n_affinities >= 1 && m->n_affinities <= VK_TX_MAX_AFFINITIES &&
           m->atp_row >= 0 && m->atp_row <= m->n_monomers && m->adp_row == (m->atp_row < m->n_monomers ? m->n_monomers : m->n_monomers + 1) &&
           (m->sequence == VK_TX_SEQUENCE_AUTO || m->sequence == VK_TX_SEQUENCE_GLOBAL || m->sequence == VK_TX_SEQUENCE_LDS) && m->copy && m->n_term &&
           m->term_pos && m->prod_ptr && m->prod_species && m->seq_ptr && m->site_ptr && m->thr_ptr && m->thr_species &&
           m->aff_ptr && m->seq && m->seq2 && m->term_strength && m->term_from && m->thr_value && m->affinity &&
           (m->n_plan == 0 || (m->interval && m->elongate));
}

extern "C" int vk_transcription_step(const vk_tx_model *model, int64_t n, int64_t ld, int32_t *slots, int32_t *length,
                                     int32_t *molecules, int32_t *counts, const double *mmol_to_counts,
                                     const int64_t *keys, uint64_t seed, int64_t *step_counter, int32_t advance,
                                     int32_t max_events, int32_t *events_out, int32_t *status, vk_stream_t stream) {
    if (!tx_model_ok(model) || n < 0 || ld < n || max_events < 1 || !step_counter || model->n_bases < 1 ||
        (n > 0 && (!slots || !length || !molecules || !counts || !mmol_to_counts || !keys || !events_out || !status))) {
        vk::set_error("vk_transcription_step: bad arguments (slots <= %d, templates <= %d, monomers <= %d, "
                      "affinities <= %d, n <= ld)",
                      VK_TX_MAX_SLOTS, VK_TX_MAX_TEMPLATES, VK_TX_MAX_MONOMERS, VK_TX_MAX_AFFINITIES);
        return VK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        // n_bases: the bases of all templates (seq_ptr[P]), which the host knows
        const size_t P = (size_t)model->n_templates;
        size_t lds = sizeof(double) * (size_t)model->n_affinities +
                     (size_t)TX_LANES * sizeof(int32_t) * ((size_t)model->max_slots + P) +
                     sizeof(int32_t) * (P + 1 + TX_NT * P);
        const size_t words = ((size_t)model->n_bases + 15) / 16;
        int seq_words = 0;
        // AUTO: only where the staged words cost no workgroup per CU (measured: profiles/transcription_timing.json)
        const bool fits = lds + 4 * words <= TX_LDS_BYTES;
        const bool free_of_cost = TX_CU_LDS_BYTES / (lds + 4 * words) == TX_CU_LDS_BYTES / lds;
        if (fits && (model->sequence == VK_TX_SEQUENCE_LDS || (model->sequence == VK_TX_SEQUENCE_AUTO && free_of_cost))) {
            seq_words = (int)words;
            lds += 4 * words;
        }
        hipLaunchKernelGGL(k_transcription_step, dim3((unsigned)((n + TX_LANES - 1) / TX_LANES)), dim3(TX_LANES), lds, s,
                           *model, seq_words, n, ld, slots, length, molecules, counts, mmol_to_counts, keys,
                           seed ^ VK_TX_DOMAIN, step_counter, (int)max_events, events_out, status);
        const int rc = vk::launch_check("k_transcription_step");
        if (rc) return rc;
    }
    return advance ? pz_advance(step_counter, s) : VK_OK;
}
