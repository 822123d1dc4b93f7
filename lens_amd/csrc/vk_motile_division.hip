// Motile agents that grow and divide on MI355X (gfx950): the flagella count derived from
// the expressed protein, and the dividers of the motile state.  One thread per agent (slot).
//
//   k_flagella_counts    DeriveCounts.next_update for the flagella protein
//                        vivarium/processes/derive_counts.py:42-51
//                        counts = int(concentration * mmol_to_counts): one FP64 multiply
//                        (-ffp-contract=off) truncated toward zero, read by FlagellaActivity
//                        as n_flagella (flagella_activity.py:138,155).
//   k_divide_flagella    the `_divide` branch of Store.apply_update
//                        vivarium/core/experiment.py:664-697 for the motile state, with
//                        divide_split on the int count (core/registry.py:205-227) and, for the
//                        flagella themselves, either what deep_merge leaves of the declared
//                        split_dict (library/dict_utils.py:51-66: every key of the mother
//                        survives in both daughters, VK_FLAGELLA_MERGED) or split_dict itself
//                        (core/registry.py:246-262, VK_FLAGELLA_SPLIT_DICT).
//
// The remainder of an odd count goes to daughter 0 when u < 0.5, else to daughter 1
// (registry.py:217-224: one random.choice per mother).  u = philox_uniform(seed ^
// VK_DIVIDE_FLAGELLA_DOMAIN, step, root, depth, path) of the MOTHER's lineage: the counter
// layout of the growth draw (vk_cells.hip), under another key.  The domain constant keeps the
// draw apart from the growth draw when both seeds are equal, and from the motility kernels'
// draws, which put (inner update, agent key, draw index) into the same counter words -- a
// mother with depth 0 and path 0 would otherwise repeat the coarse motor's switch draw.
//
// NOT the reference: flagella are bits, not uuid-named dict entries, so "the items [len // 2:]"
// are the bits at and above have / 2; daughters are named by fresh integer keys (key_base + the
// daughter's rank among this division's daughters), where the reference's agents carry a
// phylogeny string.  A survivor keeps her key, so her draws do not depend on who else divides.

#include <math.h>
#include <stdint.h>

#include "vk_internal.h"
#include "vk_philox.h"

__global__ __launch_bounds__(256) void k_flagella_counts(int64_t n, const double *__restrict__ conc,
                                                         const double *__restrict__ m2c, int32_t *__restrict__ target,
                                                         int32_t *__restrict__ flags) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const double counts = conc[a] * m2c[a];
    int32_t t = 0;                                   // NaN and everything below 1 truncate or clamp to 0
    if (counts >= 1.0) t = counts >= 32.0 ? 32 : (int32_t)counts;
    // the reference would fail (NaN, a negative count) or grow a 33rd flagellum here; every
    // lane that sees it stores the same word
    if (!(counts >= 0.0 && counts < 33.0)) flags[0] = 1;
    target[a] = t;
}

extern "C" int vk_flagella_counts(int64_t n, const double *conc, const double *m2c, int32_t *target, int32_t *flags,
                                  vk_stream_t stream) {
    if (n < 0 || !flags || (n > 0 && (!conc || !m2c || !target))) {
        vk::set_error("vk_flagella_counts: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0) return VK_OK;
    hipLaunchKernelGGL(k_flagella_counts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       conc, m2c, target, flags);
    return vk::launch_check("k_flagella_counts");
}

__global__ __launch_bounds__(256) void k_divide_flagella(
    int64_t n_out, int64_t n_keep, int64_t n_src, const int32_t *__restrict__ src_index,
    const int32_t *__restrict__ kind, const int32_t *__restrict__ fi_src, int64_t ld_src,
    const int64_t *__restrict__ key_src, const int32_t *__restrict__ root, const int32_t *__restrict__ depth,
    const uint64_t *__restrict__ path, int32_t *__restrict__ fi_dst, int64_t ld_dst, int64_t *__restrict__ key_dst,
    int mode, uint64_t seed, uint64_t step, int64_t key_base) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    const int64_t a = src_index[j];
    if (a < 0 || a >= n_src) return;                 // not a plan of these arrays: touch nothing
    const int k = kind[j];
    key_dst[j] = k < 0 ? key_src[a] : key_base + (j - n_keep);
    if (!fi_src) return;                             // the coarse motor: keys only
    int32_t target = fi_src[(int64_t)VK_FLAGI_TARGET * ld_src + a];
    int32_t have = fi_src[(int64_t)VK_FLAGI_HAVE * ld_src + a];
    int32_t mask = fi_src[(int64_t)VK_FLAGI_MASK * ld_src + a];
    if (k >= 0) {
        // divide_split on an int: half = int(state / 2), the odd one by a coin flip per mother
        const int32_t half = target / 2, rest = target - 2 * half;
        const double u = philox_uniform(seed, step, root[a], depth[a], path[a]);
        const int lucky = u < 0.5 ? 0 : 1;
        target = half + (k == lucky ? rest : 0);
        if (mode == VK_FLAGELLA_SPLIT_DICT) {
            // the stored values as the motor kernel reads them: have in 0..32, no bit above it
            const int32_t hv = min(max(have, 0), 32);
            uint32_t m = (uint32_t)mask;
            if (hv < 32) m &= (1u << hv) - 1u;
            const int32_t h = hv / 2;                // <= 16: the shifts below are defined
            if (k == 0) {
                have = hv - h;                       // the items [len // 2:]
                m >>= h;
            } else {
                have = h;                            // the items [:len // 2]
                m &= (1u << h) - 1u;
            }
            mask = (int32_t)m;
        }
    }
    fi_dst[(int64_t)VK_FLAGI_TARGET * ld_dst + j] = target;
    fi_dst[(int64_t)VK_FLAGI_HAVE * ld_dst + j] = have;
    fi_dst[(int64_t)VK_FLAGI_MASK * ld_dst + j] = mask;
}

extern "C" int vk_divide_flagella(int64_t n_out, int64_t n_keep, int64_t n_src, const int32_t *src_index,
                                  const int32_t *kind, const int32_t *flag_int_src, int64_t ld_src,
                                  const int64_t *key_src, const int32_t *root_src, const int32_t *depth_src,
                                  const uint64_t *path_src, int32_t *flag_int_dst, int64_t ld_dst, int64_t *key_dst,
                                  int32_t mode, uint64_t seed, uint64_t step, int64_t key_base, vk_stream_t stream) {
    if (n_out < 0 || n_keep < 0 || n_keep > n_out || n_src < 0 || ld_src < n_src || ld_dst < n_out ||
        (mode != VK_FLAGELLA_MERGED && mode != VK_FLAGELLA_SPLIT_DICT) || key_base < 0 ||
        key_base + (n_out - n_keep) > (int64_t)INT32_MAX + 1 || (flag_int_src == nullptr) != (flag_int_dst == nullptr) ||
        (n_out > 0 && (!src_index || !kind || !key_src || !key_dst)) ||
        (n_out > 0 && flag_int_src && n_out > n_keep && (!root_src || !depth_src || !path_src))) {
        vk::set_error("vk_divide_flagella: bad arguments");
        return VK_ERR_ARG;
    }
    if (n_out == 0) return VK_OK;
    hipLaunchKernelGGL(k_divide_flagella, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       n_out, n_keep, n_src, src_index, kind, flag_int_src, ld_src, key_src, root_src, depth_src,
                       path_src, flag_int_dst, ld_dst, key_dst, (int)mode, seed ^ VK_DIVIDE_FLAGELLA_DOMAIN, step,
                       key_base);
    return vk::launch_check("k_divide_flagella");
}
