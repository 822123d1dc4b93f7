// Philox4x32-10 (Salmon et al., SC'11), counter-based: u depends only on
// (seed, step, lineage), never on agent order or launch geometry.  Shared by the
// growth process (vk_cells.hip) and the motile-agent kernels (vk_motility.hip, vk_flagella.hip);
// restated on the host by oracle.colony.philox_uniform.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], const uint32_t (&k)[2]) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c[0] = hi1 ^ c[1] ^ k[0];
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k[1];
    c[3] = lo0;
}

// uniform double in [0, 1) with 53 random bits, numpy's (a >> 5, b >> 6) construction
__device__ __forceinline__ double philox_uniform(uint64_t seed, uint64_t step, int32_t root, int32_t depth,
                                                 uint64_t path) {
    uint32_t c[4] = {(uint32_t)step, (uint32_t)root, (uint32_t)path, (uint32_t)(path >> 32)};
    uint32_t k[2] = {(uint32_t)seed + (uint32_t)depth, (uint32_t)(seed >> 32)};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k[0] += 0x9E3779B9u;
            k[1] += 0xBB67AE85u;
        }
        philox_round(c, k);
    }
    const double a = (double)(c[0] >> 5), b = (double)(c[1] >> 6);
    return (a * 67108864.0 + b) / 9007199254740992.0;
}

// two uniform doubles of ONE block: u1 from words 0 and 1 (what philox_uniform returns for the
// same arguments), u2 from words 2 and 3 by the same construction (vk_ssa.hip: the waiting time
// and the reaction of one Gillespie event)
__device__ __forceinline__ void philox_uniform_pair(uint64_t seed, uint64_t step, int32_t root, int32_t depth,
                                                    uint64_t path, double &u1, double &u2) {
    uint32_t c[4] = {(uint32_t)step, (uint32_t)root, (uint32_t)path, (uint32_t)(path >> 32)};
    uint32_t k[2] = {(uint32_t)seed + (uint32_t)depth, (uint32_t)(seed >> 32)};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k[0] += 0x9E3779B9u;
            k[1] += 0xBB67AE85u;
        }
        philox_round(c, k);
    }
    const double a = (double)(c[0] >> 5), b = (double)(c[1] >> 6);
    const double d = (double)(c[2] >> 5), e = (double)(c[3] >> 6);
    u1 = (a * 67108864.0 + b) / 9007199254740992.0;
    u2 = (d * 67108864.0 + e) / 9007199254740992.0;
}
