// The neighbour grid of capsules and the closest points of two spines (gfx950): what the
// contact launch (vk_contact.hip) and the colony metrics (vk_colonies.hip) share.  Both units
// include this header, so an agent lands in the same cell, the sorted slots hold the same
// snapshot and a pair has the same distance d in both, operation for operation.
//
// A capsule: centre (x, y), axis angle theta, total length L, width w; radius r = w / 2, spine
// half-length h = max(L - w, 0) / 2, spine direction u = (cos, sin) theta.
//   k_contact_cells   linear cell cx * gy + cy per agent; ORs bit 0 into the flag word for an
//                     agent longer than a cell edge
//   k_contact_pack    sorted slot k := {x, y, theta, L} and {cos, sin} of agent order[k], its
//                     key, and the cell_start / cell_end tables where sorted_cell changes
//   contact_closest   the closest points of two spines and their distance
// The kernels are static: each unit that includes the header gets its own.
#pragma once

#include <math.h>
#include <stdint.h>

#include "vk_internal.h"

static inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct contact_slot {   // 32 B: one agent of the snapshot, in sorted order
    double x, y, theta, L;
};

// cell index along one axis: min(g - 1, floor(x / edge)); anything else (a location outside
// [0, bound), a NaN) lands in an end cell instead of outside the tables
__device__ __forceinline__ int contact_cell_axis(double x, double edge, int g) {
    const double v = floor(x / edge);
    if (!(v >= 0.0)) return 0;
    return v < (double)g ? (int)v : g - 1;
}

static __global__ __launch_bounds__(256) void k_contact_cells(int n, int64_t ld, const double *__restrict__ loc,
                                                              const double *__restrict__ length,
                                                              double length_const, double edge_x, double edge_y,
                                                              int gx, int gy, int32_t *__restrict__ cell,
                                                              int32_t *__restrict__ flags) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    const int cx = contact_cell_axis(loc[a], edge_x, gx);
    const int cy = contact_cell_axis(loc[ld + a], edge_y, gy);
    cell[a] = cx * gy + cy;
    const double L = length ? length[a] : length_const;
    if (L > edge_x || L > edge_y) atomicOr(flags, 1);
}

static __global__ __launch_bounds__(256) void k_contact_pack(
    int n, int64_t ld, const double *__restrict__ loc, const double *__restrict__ angle,
    const double *__restrict__ length, double length_const, const int64_t *__restrict__ key,
    const int32_t *__restrict__ order, const int32_t *__restrict__ sorted_cell, contact_slot *__restrict__ packed,
    double2 *__restrict__ dir, uint32_t *__restrict__ skey, int32_t *__restrict__ cell_start,
    int32_t *__restrict__ cell_end) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int a = order[k];
    contact_slot s;
    s.x = loc[a];
    s.y = loc[ld + a];
    s.theta = angle[a];
    s.L = length ? length[a] : length_const;
    packed[k] = s;
    dir[k] = make_double2(cos(s.theta), sin(s.theta));
    skey[k] = key ? (uint32_t)key[a] : (uint32_t)a;
    const int c = sorted_cell[k];
    if (k == 0 || sorted_cell[k - 1] != c) cell_start[c] = k;
    if (k == n - 1 || sorted_cell[k + 1] != c) cell_end[c] = k + 1;
}

__device__ __forceinline__ double clampd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// Closest points of the spines of `me` (direction ui, half-length hi) and `o` (uj, hj): returns
// their distance d (0 for coincident spines); (rx, ry) is the centre difference me - o, s the
// closest point's coordinate along me's spine, (vx, vy) the vector from o's closest point to
// me's.  Nearly parallel spines (den <= 1e-12) start from s = 0.
__device__ __forceinline__ double contact_closest(const contact_slot &me, const double2 ui, const double hi,
                                                  const contact_slot &o, const double2 uj, const double hj,
                                                  double &rx, double &ry, double &s, double &vx, double &vy) {
    rx = me.x - o.x;
    ry = me.y - o.y;
    const double b = ui.x * uj.x + ui.y * uj.y;
    const double cp = ui.x * rx + ui.y * ry;
    const double f = uj.x * rx + uj.y * ry;
    const double den = 1.0 - b * b;
    s = den > 1e-12 ? clampd((b * f - cp) / den, -hi, hi) : 0.0;
    double t = b * s + f;
    if (t < -hj) {
        t = -hj;
        s = clampd(-b * hj - cp, -hi, hi);
    } else if (t > hj) {
        t = hj;
        s = clampd(b * hj - cp, -hi, hi);
    }
    vx = (me.x + s * ui.x) - (o.x + t * uj.x);
    vy = (me.y + s * ui.y) - (o.y + t * uj.y);
    return sqrt(vx * vx + vy * vy);
}
