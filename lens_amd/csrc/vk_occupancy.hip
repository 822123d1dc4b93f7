// Device-side bin occupancy of a lattice colony (gfx950): what lens_amd.lattice.occupancy
// computes with two torch sorts and a unique_consecutive, as one radix sort that takes no
// host decision -- so a step that moves agents can re-bin them inside a captured graph.
//
// The key of agent column a is (bin_lin[a] << 32) | key32[a]: ascending keys list each
// bin's agents in reference agent order (key32 = the agent's reference-order key, its
// column index when null).  Keys are distinct, so the sorted order is unique and does not
// depend on the sort's internals.  order[k] is the column of the k-th key, sorted_bin[k]
// its bin; vk_exchange_ordered (vk_lattice.hip) finds the bin segments from sorted_bin.

#include <stdint.h>

#include <cstring>   // before rocprim: its headers use std::memcpy without including it

#include <rocprim/rocprim.hpp>

#include "vk_internal.h"

static inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// rocprim's temporary storage for n (key, value) pairs sorted on bits [0, end_bit); 0 on error
static size_t sort_temp_bytes(int64_t n, unsigned end_bit) {
    size_t bytes = 0;
    const hipError_t e = rocprim::radix_sort_pairs((void *)nullptr, bytes, (uint64_t *)nullptr, (uint64_t *)nullptr,
                                                   (int32_t *)nullptr, (int32_t *)nullptr, (size_t)n, 0u, end_bit,
                                                   (hipStream_t) nullptr, false);
    return e == hipSuccess ? bytes : 0;
}

// scratch layout: keys_in[n] u64 | keys_out[n] u64 | cols_in[n] i32 | rocprim temp (sized
// for whole 64-bit keys: a sort on fewer bits needs no more, and the call checks it)
extern "C" int64_t vk_occupancy_scratch_bytes(int64_t n) {
    if (n <= 0) return 0;
    return 2 * align256(n * 8) + align256(n * 4) + align256((int64_t)sort_temp_bytes(n, 64u)) + 256;
}

__global__ __launch_bounds__(256) void k_occupancy_keys(const int32_t *__restrict__ bin_lin,
                                                        const int64_t *__restrict__ key, int n,
                                                        uint64_t *__restrict__ keys, int32_t *__restrict__ cols) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const uint32_t k32 = key ? (uint32_t)key[a] : (uint32_t)a;
    keys[a] = ((uint64_t)(uint32_t)bin_lin[a] << 32) | k32;
    cols[a] = a;
}

__global__ __launch_bounds__(256) void k_occupancy_bins(const uint64_t *__restrict__ keys, int n,
                                                        int32_t *__restrict__ sorted_bin) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) sorted_bin[k] = (int32_t)(keys[k] >> 32);
}

extern "C" int vk_occupancy_sort(const int32_t *bin_lin, const int64_t *key, int64_t n, int64_t n_bins,
                                 int32_t *order, int32_t *sorted_bin, void *scratch, int64_t scratch_bytes,
                                 vk_stream_t stream) {
    if (n < 0 || n >= INT32_MAX || n_bins < 1 || n_bins > INT32_MAX ||
        (n > 0 && (!bin_lin || !order || !sorted_bin || !scratch))) {
        vk::set_error("vk_occupancy_sort: bad arguments");
        return VK_ERR_ARG;
    }
    if (n == 0) return VK_OK;
    // only the bits a key can have set take part: 32 key bits + the bits of n_bins - 1
    unsigned bin_bits = 0;
    while (bin_bits < 32 && ((int64_t)1 << bin_bits) < n_bins) ++bin_bits;
    size_t temp = sort_temp_bytes(n, 32u + bin_bits);
    const int64_t fixed = 2 * align256(n * 8) + align256(n * 4);
    if (scratch_bytes < vk_occupancy_scratch_bytes(n) || scratch_bytes - fixed < (int64_t)temp ||
        ((uintptr_t)scratch & 255)) {
        vk::set_error("vk_occupancy_sort: scratch must be 256-B aligned and hold vk_occupancy_scratch_bytes(n)");
        return VK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    char *base = (char *)scratch;
    uint64_t *keys_in = (uint64_t *)base;
    uint64_t *keys_out = (uint64_t *)(base + align256(n * 8));
    int32_t *cols_in = (int32_t *)(base + 2 * align256(n * 8));
    void *tmp = base + fixed;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipLaunchKernelGGL(k_occupancy_keys, grid, block, 0, s, bin_lin, key, (int)n, keys_in, cols_in);
    int rc = vk::launch_check("k_occupancy_keys");
    if (rc) return rc;
    rc = vk::hip_check(rocprim::radix_sort_pairs(tmp, temp, keys_in, keys_out, cols_in, order, (size_t)n, 0u,
                                                 32u + bin_bits, s, false),
                       "rocprim::radix_sort_pairs");
    if (rc) return rc;
    hipLaunchKernelGGL(k_occupancy_bins, grid, block, 0, s, keys_out, (int)n, sorted_bin);
    return vk::launch_check("k_occupancy_bins");
}
