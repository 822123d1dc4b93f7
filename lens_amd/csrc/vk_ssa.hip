// Stochastic mass-action kinetics on MI355X (gfx950): the Gillespie direct method, one agent
// per lane, one wavefront per workgroup.
//
//   k_ssa_step           stands where the reference calls arrow.StochasticSystem.evolve
//                        (vivarium/processes/complexation.py:74,120).  NOT arrow's arithmetic
//                        and not its random stream: the step is the one include/vk_kinetics.h
//                        states above vk_ssa_step, restated in NumPy by tests/ssa_ref.py.
//   k_ssa_propensities   the propensities alone (the same device function).
//   k_divide_counts      divide_split on int counts (core/registry.py:205-227), a coin per
//                        (mother, species).
//   k_ssa_flagella_target  the flagella count the motor reads, from the int complex count.
//
// Layout.  The reaction an agent fires differs from lane to lane, so a count vector held in
// registers would be indexed at run time and land in scratch.  Each wave stages its counts in
// LDS as x[species][lane] (int32) and its running propensity sums as cum[reaction][lane]
// (double): a lane only ever touches its own column, so every access is conflict-free, and
// one wave per workgroup means no barrier anywhere.  S = 64, R = 32 take 16 + 16 KiB.
//
// The network is the same for every lane: rates, CSR arrays and inv[] are read through
// wave-uniform addresses (ldc: the scalar cache) while the propensities are evaluated, a loop
// nest whose trip counts depend on the network alone.  Only the firing is per lane: lane l
// walks the stoichiometry CSR row of her own reaction q_l with vector loads.
//
// The event loop runs while any lane of the wave is active and at most max_events + 1 times;
// finished lanes are masked off.  Nothing waits on another workgroup.

#include <math.h>
#include <stdint.h>

#include "vk_internal.h"
#include "vk_philox.h"
#include "vk_polymerize.h"     // the step word's advance, shared with the polymerase steps

#define SSA_LANES 64

// C(n, k) as the header states it: two multiplies per factor, no divide (-ffp-contract=off)
__device__ __forceinline__ double ssa_choose(int32_t n, int k, const double *inv) {
    double c = 1.0;
    for (int i = 0; i < k; ++i) {
        c = c * (double)((int64_t)n - i);
        c = c * ldc(inv, i);
    }
    return n < k ? 0.0 : c;
}

// a_r of one agent; count(s) is her count of species s
template <class Count>
__device__ __forceinline__ double ssa_propensity(const vk_ssa_net &net, int r, Count count) {
    double a = ldc(net.rates, r);
    const int j1 = ldc(net.react_ptr, r + 1);
    for (int j = ldc(net.react_ptr, r); j < j1; ++j) {
        const int k = min(ldc(net.react_order, j), net.max_order);       // inv[] holds max_order entries
        a = a * ssa_choose(count(ldc(net.react_species, j)), k, net.inv);
    }
    return a;
}

__global__ __launch_bounds__(SSA_LANES) void k_ssa_step(vk_ssa_net net, int64_t n, int64_t ld, double T,
                                                        int32_t *__restrict__ counts,
                                                        const int64_t *__restrict__ keys, uint64_t seed,
                                                        const int64_t *__restrict__ step_counter, int max_events,
                                                        int32_t *__restrict__ events_out,
                                                        int32_t *__restrict__ status) {
    extern __shared__ __align__(16) unsigned char ssa_lds[];
    const int S = net.n_species, R = net.n_reactions;
    int32_t *x = (int32_t *)ssa_lds;                                        // [S][64]
    double *cum = (double *)(ssa_lds + (size_t)S * SSA_LANES * sizeof(int32_t));   // [R][64]
    const int lane = threadIdx.x;
    const int64_t a = (int64_t)blockIdx.x * SSA_LANES + lane;
    const bool live = a < n;
    for (int s = 0; s < S; ++s) x[s * SSA_LANES + lane] = live ? counts[(int64_t)s * ld + a] : 0;
    const int64_t key = live ? keys[a] : 0;
    int bits = 0;
    if (key < 0 || key > (int64_t)INT32_MAX) bits = VK_SSA_BAD_KEY;
    bool active = live && bits == 0;
    const uint64_t step = (uint64_t)step_counter[0];
    double t = 0.0;
    int events = 0;
    for (int it = 0; it <= max_events && __any(active); ++it) {
        // propensities and their running sums: wave-uniform control flow
        double total = 0.0;
        for (int r = 0; r < R; ++r) {
            const double a_r = ssa_propensity(net, r, [&](int s) { return x[s * SSA_LANES + lane]; });
            total = total + a_r;
            cum[r * SSA_LANES + lane] = total;
        }
        if (active) {
            if (total == 0.0) {
                active = false;                          // nothing can fire: no draw is consumed
            } else if (!isfinite(total)) {
                bits |= VK_SSA_NONFINITE;
                active = false;
            }
        }
        // draw e of this agent-step is her e-th event's: every earlier draw fired
        double u1, u2;
        philox_uniform_pair(seed, step, (int32_t)key, 0, (uint64_t)events, u1, u2);
        const double tau = -log(1.0 - u1) / total;
        if (active && t + tau > T) active = false;       // the overshooting event is discarded
        const double thr = u2 * total;
        int q = -1;
        for (int r = 0; r < R; ++r)
            if (q < 0 && cum[r * SSA_LANES + lane] > thr) q = r;
        // u2 < 1 and cum[R - 1] == total > 0, so u2 * total rounds below total and a q is found
        if (q < 0) q = R - 1;
        if (active) {
            t = t + tau;
            // per lane: the stoichiometry row of her own reaction
            const int j0 = net.stoich_ptr[q], j1 = net.stoich_ptr[q + 1];
            bool over = false;
            for (int j = j0; j < j1; ++j) {
                const int s = net.stoich_species[j];
                if ((unsigned)s < (unsigned)S &&
                    (int64_t)x[s * SSA_LANES + lane] + net.stoich_delta[j] > (int64_t)INT32_MAX)
                    over = true;
            }
            if (over) {
                bits |= VK_SSA_OVERFLOW;
                active = false;
            } else {
                for (int j = j0; j < j1; ++j) {
                    const int s = net.stoich_species[j];
                    if ((unsigned)s < (unsigned)S) x[s * SSA_LANES + lane] += net.stoich_delta[j];
                }
                if (++events >= max_events) {
                    bits |= VK_SSA_MAX_EVENTS;
                    active = false;
                }
            }
        }
    }
    if (!live) return;
    events_out[a] = events;
    if (events > 0)
        for (int s = 0; s < S; ++s) counts[(int64_t)s * ld + a] = x[s * SSA_LANES + lane];
    if (bits) status[a] |= bits;
}

__global__ __launch_bounds__(256) void k_ssa_propensities(vk_ssa_net net, int64_t n, int64_t ld,
                                                          const int32_t *__restrict__ counts,
                                                          double *__restrict__ out) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    for (int r = 0; r < net.n_reactions; ++r)
        out[(int64_t)r * ld + a] = ssa_propensity(net, r, [&](int s) { return counts[(int64_t)s * ld + a]; });
}

static bool ssa_net_ok(const vk_ssa_net *net) {
    return net && net->n_species >= 1 && net->n_species <= VK_SSA_MAX_SPECIES && net->n_reactions >= 1 &&
           net->n_reactions <= VK_SSA_MAX_REACTIONS && net->max_order >= 0 && net->max_order <= VK_SSA_MAX_ORDER &&
           net->n_inv >= net->max_order && net->react_ptr && net->react_species && net->react_order &&
           net->stoich_ptr && net->stoich_species && net->stoich_delta && net->rates && net->inv;
}

extern "C" int vk_ssa_step(const vk_ssa_net *net, int64_t n, int64_t ld, double duration, int32_t *counts,
                           const int64_t *keys, uint64_t seed, int64_t *step_counter, int32_t max_events,
                           int32_t *events_out, int32_t *status, vk_stream_t stream) {
    if (!ssa_net_ok(net) || n < 0 || ld < n || !(duration >= 0.0) || !isfinite(duration) || max_events < 1 ||
        !step_counter || (n > 0 && (!counts || !keys || !events_out || !status))) {
        vk::set_error("vk_ssa_step: bad arguments (species <= %d, reactions <= %d, order <= %d, n <= ld)",
                      VK_SSA_MAX_SPECIES, VK_SSA_MAX_REACTIONS, VK_SSA_MAX_ORDER);
        return VK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        const size_t lds = (size_t)SSA_LANES * ((size_t)net->n_species * sizeof(int32_t) +
                                                (size_t)net->n_reactions * sizeof(double));
        hipLaunchKernelGGL(k_ssa_step, dim3((unsigned)((n + SSA_LANES - 1) / SSA_LANES)), dim3(SSA_LANES), lds, s,
                           *net, n, ld, duration, counts, keys, seed ^ VK_SSA_DOMAIN, step_counter, (int)max_events,
                           events_out, status);
        const int rc = vk::launch_check("k_ssa_step");
        if (rc) return rc;
    }
    // the step word advances for an empty colony too: it counts steps, not agents
    return pz_advance(step_counter, s);
}

extern "C" int vk_ssa_propensities(const vk_ssa_net *net, int64_t n, int64_t ld, const int32_t *counts, double *out,
                                   vk_stream_t stream) {
    if (!ssa_net_ok(net) || n < 0 || ld < n || (n > 0 && (!counts || !out))) {
        vk::set_error("vk_ssa_propensities: bad arguments (species <= %d, reactions <= %d, order <= %d, n <= ld)",
                      VK_SSA_MAX_SPECIES, VK_SSA_MAX_REACTIONS, VK_SSA_MAX_ORDER);
        return VK_ERR_ARG;
    }
    if (n == 0) return VK_OK;
    hipLaunchKernelGGL(k_ssa_propensities, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *net,
                       n, ld, counts, out);
    return vk::launch_check("k_ssa_propensities");
}

__global__ __launch_bounds__(256) void k_divide_counts(int64_t n_out, int64_t n_keep, int64_t n_src,
                                                       const int32_t *__restrict__ src_index,
                                                       const int32_t *__restrict__ kind,
                                                       const int32_t *__restrict__ x_src, int64_t ld_src,
                                                       const int64_t *__restrict__ key_src,
                                                       int32_t *__restrict__ x_dst, int64_t ld_dst,
                                                       int64_t *__restrict__ key_dst, int S, uint64_t seed,
                                                       uint64_t step, int64_t key_base) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    const int64_t a = src_index[j];
    if (a < 0 || a >= n_src) return;                 // not a plan of these arrays: touch nothing
    const int k = kind[j];
    const int64_t key = key_src[a];
    key_dst[j] = k < 0 ? key : key_base + (j - n_keep);
    for (int s = 0; s < S; ++s) {
        int32_t v = x_src[(int64_t)s * ld_src + a];
        if (k >= 0) {
            // divide_split on an int: half = int(state / 2), the odd one by a coin per (mother, species)
            const int32_t half = v / 2, rest = v - 2 * half;
            const double u = philox_uniform(seed, step, (int32_t)key, 0, (uint64_t)s);
            const int lucky = u < 0.5 ? 0 : 1;
            v = half + (k == lucky ? rest : 0);
        }
        x_dst[(int64_t)s * ld_dst + j] = v;
    }
}

extern "C" int vk_divide_counts(int64_t n_out, int64_t n_keep, int64_t n_src, const int32_t *src_index,
                                const int32_t *kind, const int32_t *counts_src, int64_t ld_src, const int64_t *key_src,
                                int32_t *counts_dst, int64_t ld_dst, int64_t *key_dst, int32_t n_species,
                                uint64_t seed, uint64_t step, int64_t key_base, vk_stream_t stream) {
    if (n_out < 0 || n_keep < 0 || n_keep > n_out || n_src < 0 || ld_src < n_src || ld_dst < n_out ||
        n_species < 1 || n_species > VK_SSA_MAX_SPECIES || key_base < 0 ||
        key_base + (n_out - n_keep) > (int64_t)INT32_MAX + 1 ||
        (n_out > 0 && (!src_index || !kind || !counts_src || !key_src || !counts_dst || !key_dst))) {
        vk::set_error("vk_divide_counts: bad arguments");
        return VK_ERR_ARG;
    }
    if (n_out == 0) return VK_OK;
    hipLaunchKernelGGL(k_divide_counts, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       n_out, n_keep, n_src, src_index, kind, counts_src, ld_src, key_src, counts_dst, ld_dst, key_dst,
                       (int)n_species, seed ^ VK_SSA_DIVIDE_DOMAIN, step, key_base);
    return vk::launch_check("k_divide_counts");
}

__global__ __launch_bounds__(256) void k_ssa_flagella_target(int64_t n, const int32_t *__restrict__ row,
                                                             int32_t *__restrict__ target,
                                                             int32_t *__restrict__ flags) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const int32_t c = row[a];
    // the reference would hold a negative count or grow a 33rd flagellum here; every lane that
    // sees it stores the same word
    if (c < 0 || c > 32) flags[0] = 1;
    target[a] = min(max(c, 0), 32);
}

extern "C" int vk_ssa_flagella_target(int64_t n, const int32_t *counts_row, int32_t *target, int32_t *flags,
                                      vk_stream_t stream) {
    if (n < 0 || !flags || (n > 0 && (!counts_row || !target))) {
        vk::set_error("vk_ssa_flagella_target: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0) return VK_OK;
    hipLaunchKernelGGL(k_ssa_flagella_target, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       counts_row, target, flags);
    return vk::launch_check("k_ssa_flagella_target");
}
