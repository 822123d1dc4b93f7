// Body of the streaming-store stencil units (vk_stencil_wl6nt*.hip): the
// including unit defines VK_NT_NS (a namespace of its own, so instantiations do
// not collide with the plain ones) and VK_WL_NT_STORE.
namespace VK_NT_NS {
#include "vk_stencil_kernels.h"

namespace {

template <int K, int PD>
void launch(hipStream_t st, const double *src, double *dst, const double *f0, int nf, int64_t fs, int ny,
            int out_lo, int out_hi, int in_lo, int in_hi, int top, int bot, double coef, const double *mm,
            const VkPsCouple *cp, int tile_rows) {
    VkPsCouple none = {};
    const VkPsCouple &c = cp ? *cp : none;
    constexpr int KH = K + (K & 1);
    constexpr int W = WT_COLS - 2 * KH;
    const int tiles_x = (ny + W - 1) / W;
    const int rch = chunk_rows(tile_rows, out_hi - out_lo, tiles_x, nf);
    const int chunks_y = (out_hi - out_lo + rch - 1) / rch;
    const int waves = tiles_x * chunks_y * nf;
    int ea = 0, eb = 0;
    vk_edge_chunks(K, out_lo, out_hi, rch, chunks_y, top, bot, ea, eb);
    if (f0)
        hipLaunchKernelGGL((k_diffuse_wl<K, 3, true>), dim3((waves + 3) / 4), dim3(256), 0, st, src, dst, f0, fs,
                           ny, out_lo, out_hi, in_lo, in_hi, top, bot, rch, tiles_x, chunks_y, nf, coef, mm, c, ea, eb);
    else
        hipLaunchKernelGGL((k_diffuse_wl<K, PD, false>), dim3((waves + 3) / 4), dim3(256), 0, st, src, dst, f0, fs,
                           ny, out_lo, out_hi, in_lo, in_hi, top, bot, rch, tiles_x, chunks_y, nf, coef, mm, c, ea, eb);
}

}  // namespace
}  // namespace VK_NT_NS
