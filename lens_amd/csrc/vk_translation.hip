// Stochastic translation on MI355X (gfx950): a bounded, ordered ribosome list per agent, one
// agent per lane, one wavefront per workgroup.
//
//   k_translation_step   stands where the reference runs Translation.next_update
//                        (vivarium/processes/translation.py:423-579) with polymerize_step
//                        (vivarium/library/polymerize.py:205-259).  The step is the one
//                        include/vk_kinetics.h states above vk_translation_step, restated as
//                        Python loops by tests/translation_ref.py.
//   k_divide_ribosomes   the engine's own divider of the list: a coin per (mother, entry).
//
// The list's staging and write-back, initiation and the release sweep are vk_polymerize.h's, shared
// with transcription; this file keeps elongation (batches of four, the monomers' limits in LDS), the
// transcripts' unbound copies, the books of the monomers and the LDS layout.
//
// Layout.  The template a ribosome reads, the monomer it takes and the length of the list differ
// from lane to lane, so nothing of it can sit in registers without run-time indexing.  Each wave
// stages slot[j][lane] (the packed ribosomes), limit[monomer][lane] and unbound[template][lane]
// in LDS (and, once for the wave, the templates' offsets into the sequence table): a lane only ever touches its own column, so every access is conflict-free, and one
// wave per workgroup means no barrier anywhere.  The list crosses HBM once per launch ([slot][ld]:
// a wave's loads coalesce), not once per sub-interval.
//
// The running propensity sums are NOT staged: cum[template][lane] in FP64 would take another
// 32 KiB at 64 templates and push the workgroup past 64 KiB.  The search for the fired template
// sums the same products again in the same order, which gives the same bits (-ffp-contract=off).
//
// Affinities, operon rows and the plan are read through wave-uniform addresses (ldc: the scalar
// cache).  The sequence byte and, at a completion, the product rows are per lane (vector loads
// of small, cached tables); the sequence loads of four ribosomes are issued together.  The slot loops run to the wave's longest list; compaction is
// an in-place stable write behind the read.

#include <math.h>
#include <stdint.h>

#include "vk_internal.h"
#include "vk_philox.h"
#include "vk_polymerize.h"

#define TL_LANES PZ_LANES
#define TL_BATCH 4

__global__ __launch_bounds__(TL_LANES) void k_translation_step(vk_tl_model mdl, int64_t n, int64_t ld,
                                                               int32_t *__restrict__ slots,
                                                               int32_t *__restrict__ length,
                                                               int32_t *__restrict__ molecules,
                                                               int32_t *__restrict__ counts,
                                                               const int64_t *__restrict__ keys, uint64_t seed,
                                                               const int64_t *__restrict__ step_counter,
                                                               int max_events, int32_t *__restrict__ events_out,
                                                               int32_t *__restrict__ status) {
    extern __shared__ __align__(16) unsigned char tl_lds[];
    const int T = mdl.n_templates, M = mdl.n_monomers, cap = mdl.max_slots;
    int32_t *slot = (int32_t *)tl_lds;                  // [cap][64]
    int32_t *limit = slot + (size_t)cap * TL_LANES;     // [M][64]
    int32_t *unbound = limit + (size_t)M * TL_LANES;    // [T][64]
    int32_t *sp = unbound + (size_t)T * TL_LANES;       // [T + 1]: the templates' offsets, the wave's
    const int lane = threadIdx.x;
    const int64_t a = (int64_t)blockIdx.x * TL_LANES + lane;
    const bool live = a < n;
    int64_t key;
    int bits;
    bool run;
    int n_r = pz_stage_list(slot, lane, a, live, ld, cap, keys, slots, length, key, bits, run);
    for (int m = 0; m < M; ++m) limit[m * TL_LANES + lane] = run ? molecules[(int64_t)m * ld + a] : 0;
    for (int i = 0; i < T; ++i) {
        const int s = ldc(mdl.operon_species, i);
        unbound[i * TL_LANES + lane] = run && (unsigned)s < (unsigned)mdl.n_species ? counts[(int64_t)s * ld + a] : 0;
    }
    int32_t free_r = run ? counts[(int64_t)mdl.ribosome_species * ld + a] : 0;
    for (int i = lane; i <= T; i += TL_LANES) sp[i] = mdl.seq_ptr[i];
    __syncthreads();                         // one wave: orders the staging before the lanes' reads
    const uint64_t step = (uint64_t)step_counter[0];
    const bool stepped = run;
    bool initiates = run;                    // false: no more initiation this step
    int events = 0;
    uint64_t e = 0;
    for (int k = 0; k < mdl.n_plan; ++k) {
        const double interval = ldc(mdl.interval, k);
        // 1 the substrate: the free ribosomes before elongation
        int32_t ribosomes = free_r, terminated = 0;
        // 2 elongation, in list order, compacting behind the read.  A batch's words and monomers are
        // fetched before any of it is processed (the write index never passes the batch's first
        // slot), so the sequence loads of TL_BATCH ribosomes are in flight together
        if (ldc(mdl.elongate, k)) {
            int w = 0;
            for (int j0 = 0; __any(j0 < n_r); j0 += TL_BATCH) {
                uint32_t v[TL_BATCH];
                int len[TL_BATCH], mono[TL_BATCH];
#pragma unroll
                for (int b = 0; b < TL_BATCH; ++b) {
                    const int j = j0 + b;
                    v[b] = j < n_r ? (uint32_t)slot[j * TL_LANES + lane] : 0u;
                    const int t = (int)((v[b] >> 1) & 63u), p = (int)(v[b] >> 7);
                    len[b] = 0;
                    mono[b] = M;             // M: stalls (no such template, or past its end)
                    if (j < n_r && t < T) {
                        const int o = sp[t];
                        len[b] = sp[t + 1] - o;
                        if (p < len[b]) mono[b] = mdl.seq[o + p];
                    }
                }
#pragma unroll
                for (int b = 0; b < TL_BATCH; ++b) {
                    if (j0 + b >= n_r) continue;
                    uint32_t p = v[b] >> 7;
                    const int t = (int)((v[b] >> 1) & 63u), m = mono[b];
                    bool keep = true;
                    if (run && m < M && limit[m * TL_LANES + lane] > 0) {
                        const int j1 = (int)p + 1 == len[b] ? mdl.prod_ptr[t + 1] : 0;
                        const int i0 = (int)p + 1 == len[b] ? mdl.prod_ptr[t] : 0;
                        if ((int)p + 1 == len[b]) {
                            bool over = free_r == INT32_MAX;
                            for (int i = i0; i < j1; ++i) {
                                const int s = mdl.prod_species[i];
                                if ((unsigned)s < (unsigned)mdl.n_species && counts[(int64_t)s * ld + a] == INT32_MAX)
                                    over = true;
                            }
                            if (over) {
                                bits |= VK_TL_OVERFLOW;
                                run = false;
                                initiates = false;
                            }
                        }
                        if (run) {
                            limit[m * TL_LANES + lane] -= 1;
                            p += 1;
                            if ((int)p == len[b]) {
                                for (int i = i0; i < j1; ++i) {
                                    const int s = mdl.prod_species[i];
                                    if ((unsigned)s < (unsigned)mdl.n_species) counts[(int64_t)s * ld + a] += 1;
                                }
                                free_r += 1;
                                terminated += 1;
                                keep = false;
                            }
                        }
                    }
                    if (keep) {
                        slot[w * TL_LANES + lane] = (int32_t)((p << 7) | (v[b] & 127u));
                        ++w;
                    }
                }
            }
            n_r = w;
        }
        // 3 initiation (vk_polymerize.h): a transcript's propensity is affinity x unbound copies x
        // free ribosomes, and a binding takes one unbound copy
        const pz_state st = pz_initiate(
            slot, lane, T, cap, interval, seed, step, key, max_events,
            pz_state{ribosomes, n_r, events, bits, e, initiates},
            [affinity = mdl.affinity, unbound, lane](int i) {
                return pz_factors{ldc(affinity, i), unbound[i * TL_LANES + lane]};
            },
            [unbound, lane](int q) {
                unbound[q * TL_LANES + lane] -= 1;
                return (int32_t)VK_TL_PACK(0, q, 1);
            });
        n_r = st.n_r, events = st.events, bits = st.bits, e = st.e, initiates = st.initiates;
        free_r = st.pol + terminated;
        // 4 release: the occluding ribosomes that have cleared the start give a transcript back
        pz_unocclude<7>(slot, lane, run, n_r, mdl.occlusion, [release = mdl.release, unbound, lane, T](int t) {
            const int r = release == VK_TL_RELEASE_TEMPLATE ? t : 0;
            if (r < T) unbound[r * TL_LANES + lane] += 1;
        });
    }
    if (!live) return;
    events_out[a] = events;
    if (bits) status[a] |= bits;
    if (!stepped) return;
    // the books: the list, the free ribosomes, the monomers, ATP and ADP
    pz_store_list(slot, lane, a, ld, n_r, free_r, slots, length, counts + (int64_t)mdl.ribosome_species * ld);
    int64_t used = 0;
    for (int m = 0; m < M; ++m) {
        const int32_t now = limit[m * TL_LANES + lane], was = molecules[(int64_t)m * ld + a];
        if (now != was) {
            used += (int64_t)was - now;
            molecules[(int64_t)m * ld + a] = now;
        }
    }
    if (used) {
        const int64_t atp = (int64_t)molecules[(int64_t)M * ld + a] - 2 * used;
        const int64_t adp = (int64_t)molecules[(int64_t)(M + 1) * ld + a] + 2 * used;
        if (atp < (int64_t)INT32_MIN || adp > (int64_t)INT32_MAX) status[a] |= VK_TL_OVERFLOW;
        molecules[(int64_t)M * ld + a] = (int32_t)max(atp, (int64_t)INT32_MIN);
        molecules[(int64_t)(M + 1) * ld + a] = (int32_t)min(adp, (int64_t)INT32_MAX);
    }
}

static bool tl_model_ok(const vk_tl_model *m) {
    return m && m->n_templates >= 1 && m->n_templates <= VK_TL_MAX_TEMPLATES && m->n_monomers >= 1 &&
           m->n_monomers <= VK_TL_MAX_MONOMERS && m->n_species >= 1 && m->max_slots >= 1 &&
           m->max_slots <= VK_TL_MAX_SLOTS && m->ribosome_species >= 0 && m->ribosome_species < m->n_species &&
           m->n_plan >= 0 && (m->release == VK_TL_RELEASE_REFERENCE || m->release == VK_TL_RELEASE_TEMPLATE) &&
           m->operon_species && m->seq_ptr && m->seq && m->prod_ptr && m->prod_species && m->affinity &&
           (m->n_plan == 0 || (m->interval && m->elongate));
}

extern "C" int vk_translation_step(const vk_tl_model *model, int64_t n, int64_t ld, int32_t *slots, int32_t *length,
                                   int32_t *molecules, int32_t *counts, const int64_t *keys, uint64_t seed,
                                   int64_t *step_counter, int32_t advance, int32_t max_events, int32_t *events_out,
                                   int32_t *status, vk_stream_t stream) {
    if (!tl_model_ok(model) || n < 0 || ld < n || max_events < 1 || !step_counter ||
        (n > 0 && (!slots || !length || !molecules || !counts || !keys || !events_out || !status))) {
        vk::set_error("vk_translation_step: bad arguments (slots <= %d, templates <= %d, monomers <= %d, n <= ld)",
                      VK_TL_MAX_SLOTS, VK_TL_MAX_TEMPLATES, VK_TL_MAX_MONOMERS);
        return VK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        const size_t lds = (size_t)TL_LANES * sizeof(int32_t) *
                               ((size_t)model->max_slots + (size_t)model->n_monomers + (size_t)model->n_templates) +
                           sizeof(int32_t) * ((size_t)model->n_templates + 1);
        hipLaunchKernelGGL(k_translation_step, dim3((unsigned)((n + TL_LANES - 1) / TL_LANES)), dim3(TL_LANES), lds, s,
                           *model, n, ld, slots, length, molecules, counts, keys, seed ^ VK_TL_DOMAIN, step_counter,
                           (int)max_events, events_out, status);
        const int rc = vk::launch_check("k_translation_step");
        if (rc) return rc;
    }
    return advance ? pz_advance(step_counter, s) : VK_OK;
}

__global__ __launch_bounds__(256) void k_divide_ribosomes(int64_t n_out, int64_t n_src,
                                                          const int32_t *__restrict__ src_index,
                                                          const int32_t *__restrict__ kind,
                                                          const int32_t *__restrict__ slots_src,
                                                          const int32_t *__restrict__ length_src, int64_t ld_src,
                                                          const int64_t *__restrict__ key_src,
                                                          int32_t *__restrict__ slots_dst,
                                                          int32_t *__restrict__ length_dst, int64_t ld_dst, int cap,
                                                          uint64_t seed, uint64_t step) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    const int64_t a = src_index[j];
    if (a < 0 || a >= n_src) return;                 // not a plan of these arrays: touch nothing
    const int k = kind[j];
    const int32_t key = (int32_t)key_src[a];
    const int n_r = min(max(length_src[a], 0), cap);
    int w = 0;
    for (int i = 0; i < n_r; ++i) {
        const int32_t v = slots_src[(int64_t)i * ld_src + a];
        bool mine = true;
        if (k >= 0) {
            const double u = philox_uniform(seed, step, key, 0, (uint64_t)i << 32);
            mine = (u < 0.5 ? 0 : 1) == k;
        }
        if (mine) {
            slots_dst[(int64_t)w * ld_dst + j] = v;
            ++w;
        }
    }
    length_dst[j] = w;
    for (; w < cap; ++w) slots_dst[(int64_t)w * ld_dst + j] = 0;
}

extern "C" int vk_divide_ribosomes(int64_t n_out, int64_t n_src, const int32_t *src_index, const int32_t *kind,
                                   const int32_t *slots_src, const int32_t *length_src, int64_t ld_src,
                                   const int64_t *key_src, int32_t *slots_dst, int32_t *length_dst, int64_t ld_dst,
                                   int32_t max_slots, uint64_t seed, uint64_t step, vk_stream_t stream) {
    if (n_out < 0 || n_src < 0 || ld_src < n_src || ld_dst < n_out || max_slots < 1 || max_slots > VK_TL_MAX_SLOTS ||
        (n_out > 0 && (!src_index || !kind || !slots_src || !length_src || !key_src || !slots_dst || !length_dst))) {
        vk::set_error("vk_divide_ribosomes: bad arguments (slots <= %d)", VK_TL_MAX_SLOTS);
        return VK_ERR_ARG;
    }
    if (n_out == 0) return VK_OK;
    hipLaunchKernelGGL(k_divide_ribosomes, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       n_out, n_src, src_index, kind, slots_src, length_src, ld_src, key_src, slots_dst, length_dst,
                       ld_dst, (int)max_slots, seed ^ VK_TL_DIVIDE_DOMAIN, step);
    return vk::launch_check("k_divide_ribosomes");
}
