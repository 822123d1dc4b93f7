// RNA degradation on MI355X (gfx950): Michaelis-Menten in the endoRNAse and the transcript with a
// fractional carry, one agent per lane.
//
//   k_rna_degradation_step  stands where the reference runs RnaDegradation.next_update
//                           (vivarium/processes/degradation.py:136-182).  The step is the one
//                           include/vk_kinetics.h states above vk_rna_degradation_step, restated
//                           as Python loops by tests/degradation_ref.py.  The rate law, the carry
//                           and the books with their signs are the reference's; the clamp at the
//                           transcript's count and the in-place process order are THE ENGINE'S OWN.
//
// Layout.  The network is the same for every lane: rows, the pair CSR, kcat, km and the compositions
// are read through wave-uniform addresses (ldc: the scalar cache).  Every count, partial and pool
// access is row * ld + a: a wave's loads and stores coalesce.  No LDS, no atomics.
//
// A failing agent (VK_DEG_NONFINITE, VK_DEG_OVERFLOW) must have nothing written, and whether she
// fails is known only once every transcript's d is: the pools' deltas are sums over all of them.
// The transcripts go in chunks of DEG_CHUNK, whose loads are all issued before the chunk's
// arithmetic, so a lane has 2 x DEG_CHUNK loads in flight, not one dependent load after another.
// A model of at most DEG_CHUNK transcripts (the flagella chromosome has 15) keeps every d and carry
// in registers between the decision and the stores: each byte crosses HBM once.  A longer model
// runs the chunks twice, once to decide and once to store; the second pass repeats the first's
// arithmetic on the same inputs (nothing was written in between), so it stores the same bits.

#include <math.h>
#include <stdint.h>

#include "vk_internal.h"

#define DEG_THREADS 256
#define DEG_CHUNK 16
#define DEG_NM VK_DEG_MAX_MONOMERS
#define DEG_NE VK_DEG_MAX_ENZYMES

struct deg_chunk {
    int32_t x[DEG_CHUNK];     // the transcript's count, as loaded
    int32_t d[DEG_CHUNK];     // what she loses
    double carry[DEG_CHUNK];  // the partial: loaded, then the new one
};

// transcripts [t0, t0 + DEG_CHUNK) of agent a: loads, then arithmetic.  bad: a total was not finite
__device__ __forceinline__ void deg_eval(const vk_deg_model &mdl, int t0, int64_t a, int64_t ld,
                                         const int32_t *__restrict__ counts, const double *__restrict__ partial,
                                         double m, double T, const double (&level_e)[DEG_NE], deg_chunk &c, bool &bad) {
    const int NT = mdl.n_transcripts;
#pragma unroll
    for (int i = 0; i < DEG_CHUNK; ++i) {
        c.x[i] = 0;
        c.carry[i] = 0.0;
        if (t0 + i < NT) {
            const int row = ldc(mdl.transcript_row, t0 + i);
            if ((unsigned)row < (unsigned)mdl.n_rows) c.x[i] = counts[(int64_t)row * ld + a];
            c.carry[i] = partial[(int64_t)(t0 + i) * ld + a];
        }
    }
#pragma unroll
    for (int i = 0; i < DEG_CHUNK; ++i) {
        c.d[i] = 0;
        if (t0 + i >= NT) continue;
        const double S = (double)c.x[i] / m;
        double level = 0.0;
        for (int j = ldc(mdl.pair_ptr, t0 + i); j < ldc(mdl.pair_ptr, t0 + i + 1); ++j) {
            const int k = ldc(mdl.pair_enzyme, j);
            double E = 0.0;
#pragma unroll
            for (int q = 0; q < DEG_NE; ++q)
                if (k == q) E = level_e[q];
            level = level + ((ldc(mdl.kcat, j) * E) * S) / (S + ldc(mdl.km, j));
        }
        const double total = (level * m) * T + c.carry[i];
        if (!isfinite(total)) {
            bad = true;
            continue;
        }
        const double whole = trunc(total);
        c.carry[i] = total - whole;
        // (int) trunc(total), saturated where it leaves int32; the clamp then brings it to the count
        const int32_t d = whole >= 2147483648.0 ? INT32_MAX : whole <= -2147483649.0 ? INT32_MIN : (int32_t)whole;
        c.d[i] = min(d, c.x[i]);
    }
}

// the chunk's share of the pools' deltas: monomers by composition, and the bases (ATP up, ADP down)
__device__ __forceinline__ void deg_books(const vk_deg_model &mdl, int t0, const deg_chunk &c, int64_t (&delta)[DEG_NM],
                                          int64_t &bases, int64_t &lost) {
#pragma unroll
    for (int i = 0; i < DEG_CHUNK; ++i) {
        if (t0 + i >= mdl.n_transcripts) continue;
        const int64_t d = c.d[i];
#pragma unroll
        for (int q = 0; q < DEG_NM; ++q) delta[q] += d * ldc(mdl.composition, DEG_NM * (t0 + i) + q);
        bases += d * ldc(mdl.length, t0 + i);
        lost += d;
    }
}

__device__ __forceinline__ void deg_store(const vk_deg_model &mdl, int t0, int64_t a, int64_t ld,
                                          int32_t *__restrict__ counts, double *__restrict__ partial, const deg_chunk &c) {
#pragma unroll
    for (int i = 0; i < DEG_CHUNK; ++i) {
        if (t0 + i >= mdl.n_transcripts) continue;
        partial[(int64_t)(t0 + i) * ld + a] = c.carry[i];
        const int row = ldc(mdl.transcript_row, t0 + i);
        if (c.d[i] != 0 && (unsigned)row < (unsigned)mdl.n_rows) counts[(int64_t)row * ld + a] = c.x[i] - c.d[i];
    }
}

__global__ __launch_bounds__(DEG_THREADS) void k_rna_degradation_step(
    vk_deg_model mdl, int64_t n, int64_t ld, double T, int32_t *__restrict__ counts, double *__restrict__ partial,
    int32_t *__restrict__ molecules, const double *__restrict__ m2c, int32_t *__restrict__ degraded_out,
    int32_t *__restrict__ status) {
    const int64_t a = (int64_t)blockIdx.x * DEG_THREADS + threadIdx.x;
    if (a >= n) return;
    const int NT = mdl.n_transcripts, M = mdl.n_monomers;
    const double m = m2c[a];
    int32_t pool[DEG_NM], atp = 0, adp;
#pragma unroll
    for (int q = 0; q < DEG_NM; ++q) pool[q] = q < M ? molecules[(int64_t)q * ld + a] : 0;
    if (mdl.atp_row >= M) atp = molecules[(int64_t)mdl.atp_row * ld + a];
    adp = molecules[(int64_t)mdl.adp_row * ld + a];
    double level_e[DEG_NE];
#pragma unroll
    for (int q = 0; q < DEG_NE; ++q) {
        level_e[q] = 0.0;
        if (q < mdl.n_enzymes) {
            const int row = ldc(mdl.enzyme_row, q);
            const int32_t x = (unsigned)row < (unsigned)mdl.n_rows ? counts[(int64_t)row * ld + a] : 0;
            level_e[q] = (double)x / m;
        }
    }
    bool bad = !(isfinite(m) && m > 0.0);
    int64_t delta[DEG_NM] = {0, 0, 0, 0}, bases = 0, lost = 0;
    deg_chunk c;
    const bool once = NT <= DEG_CHUNK;
    for (int t0 = 0; t0 < NT; t0 += DEG_CHUNK) {
        deg_eval(mdl, t0, a, ld, counts, partial, m, T, level_e, c, bad);
        deg_books(mdl, t0, c, delta, bases, lost);
    }
    int bits = bad ? VK_DEG_NONFINITE : 0;
    // the pools after the books, in int64 before any write: monomers (ATP among them gains the bases
    // too), then ATP where it is no monomer, then ADP
    int64_t after[DEG_NM], atp_after = (int64_t)atp + bases;
    const int64_t adp_after = (int64_t)adp - bases;
    bool over = false;
#pragma unroll
    for (int q = 0; q < DEG_NM; ++q) {
        after[q] = (int64_t)pool[q] + delta[q] + (q == mdl.atp_row ? bases : 0);
        if (q < M && (after[q] > (int64_t)INT32_MAX || after[q] < (int64_t)INT32_MIN)) over = true;
    }
    if (mdl.atp_row >= M && (atp_after > (int64_t)INT32_MAX || atp_after < (int64_t)INT32_MIN)) over = true;
    if (adp_after > (int64_t)INT32_MAX || adp_after < (int64_t)INT32_MIN) over = true;
    if (!bad && over) bits = VK_DEG_OVERFLOW;
    if (bits) {
        status[a] |= bits;
        degraded_out[a] = 0;
        return;                              // nothing of her is written
    }
    degraded_out[a] = (int32_t)min(max(lost, (int64_t)INT32_MIN), (int64_t)INT32_MAX);
    if (once) {
        deg_store(mdl, 0, a, ld, counts, partial, c);
    } else {
        for (int t0 = 0; t0 < NT; t0 += DEG_CHUNK) {
            deg_eval(mdl, t0, a, ld, counts, partial, m, T, level_e, c, bad);
            deg_store(mdl, t0, a, ld, counts, partial, c);
        }
    }
#pragma unroll
    for (int q = 0; q < DEG_NM; ++q)
        if (q < M && after[q] != (int64_t)pool[q]) molecules[(int64_t)q * ld + a] = (int32_t)after[q];
    if (bases != 0) {
        if (mdl.atp_row >= M) molecules[(int64_t)mdl.atp_row * ld + a] = (int32_t)atp_after;
        molecules[(int64_t)mdl.adp_row * ld + a] = (int32_t)adp_after;
    }
}

static bool deg_model_ok(const vk_deg_model *m) {
    return m && m->n_transcripts >= 1 && m->n_transcripts <= VK_DEG_MAX_TRANSCRIPTS && m->n_enzymes >= 1 &&
           m->n_enzymes <= VK_DEG_MAX_ENZYMES && m->n_pairs >= 0 && m->n_pairs <= VK_DEG_MAX_PAIRS &&
           m->n_monomers >= 1 && m->n_monomers <= VK_DEG_MAX_MONOMERS && m->n_rows >= 1 && m->atp_row >= 0 &&
           m->atp_row <= m->n_monomers &&
           m->adp_row == (m->atp_row < m->n_monomers ? m->n_monomers : m->n_monomers + 1) && m->transcript_row &&
           m->enzyme_row && m->pair_ptr && m->pair_enzyme && m->composition && m->length && m->kcat && m->km;
}

extern "C" int vk_rna_degradation_step(const vk_deg_model *model, int64_t n, int64_t ld, double timestep,
                                       int32_t *counts, double *partial, int32_t *molecules,
                                       const double *mmol_to_counts, int32_t *degraded_out, int32_t *status,
                                       vk_stream_t stream) {
    if (!deg_model_ok(model) || n < 0 || ld < n || !(timestep >= 0.0) || !isfinite(timestep) ||
        (n > 0 && (!counts || !partial || !molecules || !mmol_to_counts || !degraded_out || !status))) {
        vk::set_error("vk_rna_degradation_step: bad arguments (transcripts <= %d, enzymes <= %d, pairs <= %d, "
                      "monomers <= %d, n <= ld, timestep finite and >= 0)",
                      VK_DEG_MAX_TRANSCRIPTS, VK_DEG_MAX_ENZYMES, VK_DEG_MAX_PAIRS, VK_DEG_MAX_MONOMERS);
        return VK_ERR_ARG;
    }
    if (n == 0) return VK_OK;
    hipLaunchKernelGGL(k_rna_degradation_step, dim3((unsigned)((n + DEG_THREADS - 1) / DEG_THREADS)), dim3(DEG_THREADS),
                       0, (hipStream_t)stream, *model, n, ld, timestep, counts, partial, molecules, mmol_to_counts,
                       degraded_out, status);
    return vk::launch_check("k_rna_degradation_step");
}
