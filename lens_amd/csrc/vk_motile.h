// What the two motile-agent kernels share (vk_motility.hip: the coarse two-state motor,
// vk_flagella.hip: the multi-flagellar motor): the chemoreceptor cluster, the tumble's heading
// change, the move with its reflecting walls, and the launch that advances the Philox
// counter.  One statement of each, so both kernels sense and move alike; every function is
// forced inline and keeps the operation order the coarse kernel had when they lived in it
// (its results and its register use are unchanged).
#pragma once

#include <math.h>
#include <stdint.h>

#include "vk_bin.h"
#include "vk_gradient.h"
#include "vk_internal.h"
#include "vk_philox.h"

// What an agent senses at an inner update, the kernels' one template parameter: the ligand
// plane ([nx][ny], whole and unbanded, not written here) at the agent's bin, or an analytic
// gradient at the agent's own position (the reference's StaticField deriver, which runs after
// every update of receptor, motor and body: the value is the field where the previous inner
// update left the agent).  The plane stays a plain restrict pointer in the kernel's
// arguments, as it was before there was a choice.
typedef const double *__restrict__ sense_plane;
typedef vk_gradient_spec sense_static;
__device__ __forceinline__ double motile_sense(sense_plane ligand, int32_t bin, double, double) { return ligand[bin]; }
__device__ __forceinline__ double motile_sense(const sense_static &g, int32_t, double x, double y) {
    return gradient_value(g, x, y);
}

// ReceptorCluster.next_update (vivarium/processes/chemoreceptor_cluster.py:166-209) at ligand
// concentration L over h seconds; CheR / CheB already in uM.  The reference's quirk is kept:
// an out-of-range n_methyl is clamped and not advanced in that update.
__device__ __forceinline__ void motile_receptor(const vk_motility_params &p, double CheR, double CheB, double L,
                                                double h, double &n_methyl, double &P_on) {
    if (n_methyl < 0.0) {
        n_methyl = 0.0;
    } else if (n_methyl > 8.0) {
        n_methyl = 8.0;
    } else {
        const double d_methyl = p.adapt_rate * (p.k_meth * CheR * (1.0 - P_on) - p.k_demeth * CheB * P_on) * h;
        n_methyl += d_methyl;
    }
    double offset_energy;
    if (n_methyl < 0.0) offset_energy = 1.0;
    else if (n_methyl < 2.0) offset_energy = 1.0 - 0.5 * n_methyl;
    else if (n_methyl < 4.0) offset_energy = -0.3 * (n_methyl - 2.0);
    else if (n_methyl < 6.0) offset_energy = -0.6 - 0.25 * (n_methyl - 4.0);
    else if (n_methyl < 7.0) offset_energy = -1.1 - 0.9 * (n_methyl - 6.0);
    else if (n_methyl < 8.0) offset_energy = -2.0 - (n_methyl - 7.0);
    else offset_energy = -3.0;
    const double Tar = p.n_Tar * (offset_energy + log((1.0 + L / p.K_Tar_off) / (1.0 + L / p.K_Tar_on)));
    const double Tsr = p.n_Tsr * (offset_energy + log((1.0 + L / p.K_Tsr_off) / (1.0 + L / p.K_Tsr_on)));
    P_on = 1.0 / (1.0 + exp(Tar + Tsr));
}

// A standard normal from the Philox draws `path` and `path + 1` of (seed, step, k): Box-Muller
__device__ __forceinline__ double motile_normal(uint64_t seed, uint64_t step, int32_t k, uint64_t path) {
    const double u1 = philox_uniform(seed, step, k, 0, path);
    const double u2 = philox_uniform(seed, step, k, 0, path + 1);
    return sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
}

// The tumble's Gaussian heading change (draws 1 and 2); returns d_angle / h, the torque emitted
__device__ __forceinline__ double motile_tumble(const vk_motility_params &p, uint64_t step, int32_t k, double h,
                                                double &angle) {
    const double z = motile_normal(p.seed, step, k, 1);
    const double d_angle = p.tumble_sigma * h * z;
    angle += d_angle;
    return d_angle / h;
}

// speed * h along the heading; reflecting walls mirror the coordinate and the heading, then the
// coordinate is clamped into [0, bound).  Returns the linear bin of the place reached.
__device__ __forceinline__ int32_t motile_move(double speed, double h, double &angle, double &x, double &y, int nx,
                                               int ny, double bx, double by, double bx_below, double by_below,
                                               int *ix) {
    x += speed * h * cos(angle);
    y += speed * h * sin(angle);
    if (x < 0.0) {
        x = -x;
        angle = M_PI - angle;
    } else if (x >= bx) {
        x = 2.0 * bx - x;
        angle = M_PI - angle;
    }
    if (y < 0.0) {
        y = -y;
        angle = -angle;
    } else if (y >= by) {
        y = 2.0 * by - y;
        angle = -angle;
    }
    x = fmin(fmax(x, 0.0), bx_below);
    y = fmin(fmax(y, 0.0), by_below);
    return bin_site_lin(x, y, nx, ny, bx, by, 0, ix);
}

// after the agents' kernel, in stream order: the next call's first inner update
static __global__ void k_motile_advance(uint64_t *counter, uint64_t by) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counter[0] += by;
}
