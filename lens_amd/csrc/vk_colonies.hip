// Colony metrics on MI355X (gfx950): which capsules form a colony, and each colony's cell
// count, mass, area, centroid, orientation and axes.
//
// THIS ENGINE'S OWN definition, not the reference's.  The reference's ColonyShapeDeriver
// (vivarium/processes/derive_colony_shape.py) builds an alpha shape of the cell centres
// (a Delaunay triangulation), takes each polygon's area, its minimum rotated rectangle's sides
// and its circumference, and sums the mass of the cells inside.  Nothing here builds a
// polygon: no parity with its areas or axes is claimed, and there is no circumference.  What
// agrees is the colony count and the colony masses on the reference's own test scenarios.
//
// Agents are the capsules of vk_contact_step: centre (x, y), axis angle theta, length L, width
// w; r = w / 2, spine half-length h = max(L - w, 0) / 2, u = (cos, sin) theta.
//
// Link.  Agents i != j are linked when (2 r + link_gap) - d_ij >= 0, d_ij the distance of the
// closest points of the two spines as contact_closest (vk_capsule_grid.h) computes it for the
// ordered pair (i, j): the contact kernel's own solve and clamps, the den > 1e-12 parallel
// branch and d = 0 for coincident spines included.  Every agent evaluates every neighbour, so
// a pair is linked when either ordered evaluation says so.  An agent whose x or y is not
// finite links to nobody and belongs to no colony.
//
// Colony.  A connected component of the link graph with at least min_cells members (and a
// finite location).  Colonies are numbered 0 .. C - 1 in the order of their first member in
// ascending (grid cell, key) order; colony_key[c] is the smallest key among the members.
// Agents of no colony get colony = -1.
//
// Per colony c, members m_0, m_1, ... in ascending (grid cell, key) order, size of them:
//   cells      size
//   mass       sum of the members' mass (the constant when the array is NULL)
//   cell_area  sum of w * max(L - w, 0) + pi * w * w / 4: the capsules' own area, so where two
//              capsules overlap the overlap counts twice
//   cx, cy     sum x / size, sum y / size
//   sxx, syy, sxy   sums of dx dx, dy dy, dx dy with dx = x - cx, dy = y - cy
//   angle      phi = 0.5 * atan2(2 sxy, sxx - syy)   (isotropic: atan2(0, 0) = 0)
//   major, minor    with e1 = (cos phi, sin phi), e2 = (-sin phi, cos phi) and, along e,
//              hi_e = max over members of ((dx, dy).e + h |u.e|) + r,
//              lo_e = min over members of ((dx, dy).e - h |u.e|) - r  (capsule ends included;
//              centred on (cx, cy), which changes no extent): the larger and the smaller of
//              hi_e1 - lo_e1 and hi_e2 - lo_e2
//
// The order of every sum (and min, max) is fixed.  A run of members m_0 .. m_{q-1} is combined
// by one workgroup of 256 threads:
//   thread t:   p_t = (((id op m_t) op m_{t+256}) op m_{t+512}) ...   (id = 0, +inf or -inf;
//               at most ceil(q / 256) terms)
//   wave w:     the butterfly  p = p op shfl_xor(p, o)  for o = 32, 16, 8, 4, 2, 1 over its 64
//               lanes (op is commutative, so every lane ends with the same bits)
//   run:        ((w_0 op w_1) op w_2) op w_3
// A colony of at most COL_SPLIT = 512 members is one run.  A larger one (one giant colony is
// the common case) is COL_PARTS = 64 runs of S = 256 ceil(size / 16384) consecutive members
// each (the last ones may be short or empty: the identity), P_0 .. P_63, combined as
// ((P_0 op P_1) op P_2) ... op P_63 by one thread: no thread loops over more than
// size / 16384 + 1 or 64 terms.  Every result is a function of the member sequence alone: not of
// the storage order, the launch geometry or the other colonies.  No floating-point atomics.
//
// Launches, all on the caller's stream, no host synchronisation (the call can be captured):
//   k_contact_cells, vk_occupancy_sort (bin = cell), k_contact_pack      the contact launch's grid, with
//                     cell edges >= max_length + link_gap so that 3 x 3 cells suffice
//   k_colony_link     one thread per sorted slot visits the three runs of its 3 x 3 cells and
//                     unites itself with every linked neighbour (union-find over slots)
//   k_colony_flatten  root[k] = find(k): the smallest slot of k's component
//   k_colony_census   size[root[k]] += 1 (integer atomics, combined per workgroup and key first)
//   k_colony_count, k_colony_scan_blocks, k_colony_rank     the three-launch exclusive scan
//                     of vk_population_plan over "slot k is the root of a colony"; writes
//                     *n_colonies, cells[c] and the root's key into colony_key[c]
//   k_colony_label    colony[agent], atomicMin into colony_key, the second sort's bin
//   vk_occupancy_sort (bin = colony, agents of none in bin n; key = slot), k_colony_runs
//                     every colony is then one run in (cell, key) order
//   k_colony_reduce<F>, k_colony_reduce_parts<F>, k_colony_reduce_finish<F> for F = colony_sums,
//                     colony_moments, colony_extents: the three passes; small colonies, the
//                     parts of the large ones (listed by k_colony_rank), their combination
// With metrics == NULL the call ends after k_colony_label.
//
// Union-find.  parent[k] <= k always: a root is hooked under a smaller root only, by a
// compare-and-swap parent[a]: a -> b with b < a.  So every find walks strictly downward and
// ends, and a component's final root is its smallest slot.  The compare-and-swap of unite
// fails only when another thread's hook of the same root succeeded in between; at most n - 1
// hooks succeed in a launch, so every retry loop ends under any schedule.  No thread waits
// for another to act and nothing is polled.  The retries are bounded anyway (n + 16 per
// pair): past that the thread ORs VK_COLONIES_GAVE_UP into the flag word and goes on.  Path
// halving writes parent[x] := parent[parent[x]] for a non-root x: a non-root never becomes a
// root again, any ancestor is a valid parent, and a hook's compare-and-swap expects a root,
// so the two cannot undo each other.  Inside k_colony_link parent is read with agent-scope
// relaxed atomic loads (the per-CU caches are not coherent inside a launch, and a plain load
// may stay in a register); k_colony_flatten is a launch of its own and reads it plainly.
//
// Hazards: every loop is bounded by cell_end - cell_start, by the walk to a root (<= n), by
// n + 16 retries, by ceil(size / 256) for a small colony or by the parts of a large one; the
// atomics are integer (Or, Add, Min, CAS).

#include <math.h>
#include <stdint.h>

#include "vk_capsule_grid.h"

#define COL_BLOCK 1024   // slots per workgroup of the scan's launches (4 per thread)
#define COL_SPLIT 512    // a colony of more members is reduced in COL_PARTS parts
#define COL_PARTS 64

// scratch layout: cell[n] i32 | order[n] i32 | sorted_cell[n] i32 | skey[n] u32 |
// packed[n] 32 B | dir[n] 16 B | cell_start[g] i32 | cell_end[g] i32 | parent[n] i32 |
// root[n] i32 | size[n] i32 | rank[n] i32 | bin2[n] i32 | order2[n] i32 | sorted_col[n] i32 |
// col_start[n] i32 | block_count[nb + 2] i32 | n_big i32 | big_list[n / COL_SPLIT + 1] i32 |
// partial[(n / COL_SPLIT + 1) COL_PARTS 4] f64 | the sort's scratch
static inline int64_t colonies_fixed_bytes(int64_t n, int64_t g) {
    const int64_t nb = (n + COL_BLOCK - 1) / COL_BLOCK, mb = n / COL_SPLIT + 1;
    return 12 * align256(n * 4) + align256(n * 32) + align256(n * 16) + 2 * align256(g * 4) +
           align256((nb + 2) * 4) + 256 + align256(mb * 4) + align256(mb * COL_PARTS * 4 * 8);
}

extern "C" int64_t vk_colonies_scratch_bytes(int64_t n, int64_t n_grid_cells) {
    if (n <= 0 || n_grid_cells <= 0) return 0;
    return colonies_fixed_bytes(n, n_grid_cells) + vk_occupancy_scratch_bytes(n) + 256;
}

__device__ __forceinline__ int32_t parent_load(const int32_t *parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x, halving the path on the way (see the header for why that is safe)
__device__ __forceinline__ int colony_find(int32_t *parent, int x) {
    int p = parent_load(parent, x);
    while (p != x) {
        const int gp = parent_load(parent, p);
        if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = gp;
    }
    return x;
}

// join the components of slots a and b: the larger root goes under the smaller
__device__ __forceinline__ void colony_unite(int32_t *parent, int a, int b, int max_tries, int32_t *flags) {
    for (int tries = 0;; ++tries) {
        a = colony_find(parent, a);
        b = colony_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(parent + a, a, b) == a) return;
        // another thread hooked a first: one of at most n - 1 hooks of the launch
        if (tries >= max_tries) {
            atomicOr(flags, VK_COLONIES_GAVE_UP);
            return;
        }
    }
}

__global__ __launch_bounds__(256) void k_colony_init(int n, int32_t *__restrict__ parent) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) parent[k] = k;
}

__global__ __launch_bounds__(256) void k_colony_link(vk_colonies_params p, int n,
                                                     const contact_slot *__restrict__ packed,
                                                     const double2 *__restrict__ dir,
                                                     const int32_t *__restrict__ sorted_cell,
                                                     const int32_t *__restrict__ cell_start,
                                                     const int32_t *__restrict__ cell_end, int32_t *parent,
                                                     int32_t *__restrict__ flags) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const contact_slot me = packed[k];
    if (me.L > p.max_length) atomicOr(flags, VK_COLONIES_TOO_LONG);
    if (!isfinite(me.x) || !isfinite(me.y)) return;      // links to nobody
    const double2 ui = dir[k];
    const double r = p.width / 2.0;
    const double hi = fmax(me.L - p.width, 0.0) / 2.0;
    const double touch = (r + r) + p.link_gap;
    const int c = sorted_cell[k];
    const int cx = c / p.gy, cy = c - cx * p.gy;
    const int y0 = cy > 0 ? cy - 1 : 0, y1 = cy < p.gy - 1 ? cy + 1 : p.gy - 1;
    const int max_tries = n + 16;
    for (int xx = (cx > 0 ? cx - 1 : 0); xx <= (cx < p.gx - 1 ? cx + 1 : p.gx - 1); ++xx) {
        // cells (xx, y0 .. y1) are adjacent in the sorted array (an empty cell has
        // start == end == 0 and contributes nothing)
        for (int cc = xx * p.gy + y0; cc <= xx * p.gy + y1; ++cc) {
            const int j1 = cell_end[cc];
            for (int j = cell_start[cc]; j < j1; ++j) {
                if (j == k) continue;
                const contact_slot o = packed[j];
                if (!isfinite(o.x) || !isfinite(o.y)) continue;
                const double hj = fmax(o.L - p.width, 0.0) / 2.0;
                const double dx = me.x - o.x, dy = me.y - o.y;
                // exact: a spine point is within h of its centre, so d >= |rho| - hi - hj; with
                // |rho| more than 5e-7 of the reach beyond hi + hj + 2 r + gap the margin is
                // negative by far more than rounding
                const double reach = hi + hj + touch;
                if (dx * dx + dy * dy > reach * reach * 1.000001) continue;
                double rx, ry, s, vx, vy;
                const double d = contact_closest(me, ui, hi, o, dir[j], hj, rx, ry, s, vx, vy);
                if (touch - d >= 0.0) colony_unite(parent, k, j, max_tries, flags);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_colony_flatten(int n, const int32_t *__restrict__ parent,
                                                        int32_t *__restrict__ root) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    int x = k, q = parent[x];
    while (q != x) {      // strictly downward
        x = q;
        q = parent[x];
    }
    root[k] = x;
}

// One integer atomic per workgroup for the key its waves lead with, instead of one per lane.
// Almost every slot of a packed plane has the same root and the same colony: a million atomics
// on one address serialise (11 ms each for the census and the key minimum at 1M capsules).
// Each wave combines the lanes that share its first active lane's key (a butterfly over the
// wave; integer add and min, so the result does not depend on the grouping), thread 0 merges
// the four waves' entries of equal key and issues them; lanes with another key go straight to
// their own address.  Every thread of the workgroup must call it (it has a barrier).
struct colony_count_op {
    int32_t *size;
    __device__ static unsigned long long identity() { return 0ull; }
    __device__ static unsigned long long combine(unsigned long long a, unsigned long long b) { return a + b; }
    __device__ void apply(int key, unsigned long long v) const { atomicAdd(size + key, (int)v); }
};

struct colony_min_op {
    int64_t *colony_key;
    __device__ static unsigned long long identity() { return ~0ull; }
    __device__ static unsigned long long combine(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
    __device__ void apply(int key, unsigned long long v) const {
        atomicMin((unsigned long long *)colony_key + key, v);
    }
};

template <class Op>
__device__ __forceinline__ void colony_atomic_by_key(const Op op, bool active, int key, unsigned long long val) {
    __shared__ int lead_key[4];
    __shared__ unsigned long long lead_val[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long act = __ballot(active);
    bool mine = false;
    if (act) {        // the whole wave
        const int k0 = __shfl(key, __ffsll(act) - 1);
        mine = active && key == k0;
        unsigned long long v = mine ? val : Op::identity();
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = Op::combine(v, __shfl_xor(v, o));
        if (lane == 0) {
            lead_key[w] = k0;
            lead_val[w] = v;
        }
    } else if (lane == 0) {
        lead_key[w] = -1;
    }
    if (active && !mine) op.apply(key, val);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 0; i < 4; ++i) {
            if (lead_key[i] < 0) continue;
            unsigned long long v = lead_val[i];
            for (int j = i + 1; j < 4; ++j) {
                if (lead_key[j] == lead_key[i]) {
                    v = Op::combine(v, lead_val[j]);
                    lead_key[j] = -1;
                }
            }
            op.apply(lead_key[i], v);
        }
    }
}

__global__ __launch_bounds__(256) void k_colony_census(int n, const int32_t *__restrict__ root,
                                                       int32_t *__restrict__ size) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    colony_atomic_by_key(colony_count_op{size}, k < n, k < n ? root[k] : -1, 1ull);
}

// slot k is the root of a colony: its own root, enough members, a finite location
__device__ __forceinline__ int colony_is_root(int k, const int32_t *root, const int32_t *size,
                                              const contact_slot *packed, int min_cells) {
    if (root[k] != k || size[k] < min_cells) return 0;
    return isfinite(packed[k].x) && isfinite(packed[k].y) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_colony_count(int n, const int32_t *__restrict__ root,
                                                      const int32_t *__restrict__ size,
                                                      const contact_slot *__restrict__ packed, int min_cells,
                                                      int32_t *__restrict__ block_count) {
    const int base = blockIdx.x * COL_BLOCK;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = base + i * 256 + threadIdx.x;
        if (k < n) cnt += colony_is_root(k, root, size, packed, min_cells);
    }
    __shared__ int part[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// one block: exclusive scan of the nb block counts in place; the total goes to element nb
// and to *n_colonies
__global__ __launch_bounds__(256) void k_colony_scan_blocks(int32_t *__restrict__ block_count, int nb,
                                                            int32_t *__restrict__ n_colonies) {
    __shared__ int carry;
    __shared__ int wsum[4];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int v = b < nb ? block_count[b] : 0;
        int x = v;     // inclusive wave scan
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        int ws = 0;
        for (int i = 0; i < w; ++i) ws += wsum[i];
        const int e = carry + ws + x - v;
        __syncthreads();
        if (b < nb) block_count[b] = e;
        if (threadIdx.x == 255) carry = e + v;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        block_count[nb] = carry;
        *n_colonies = carry;
    }
}

__global__ __launch_bounds__(256) void k_colony_rank(int n, const int32_t *__restrict__ root,
                                                     const int32_t *__restrict__ size,
                                                     const contact_slot *__restrict__ packed, int min_cells,
                                                     const int32_t *__restrict__ block_off,
                                                     const uint32_t *__restrict__ skey, int32_t *__restrict__ rank,
                                                     int32_t *__restrict__ cells, int64_t *__restrict__ colony_key,
                                                     int32_t *__restrict__ big_list, int32_t *n_big) {
    // 4 consecutive slots per thread -> thread counts -> block exclusive scan
    const int k0 = blockIdx.x * COL_BLOCK + threadIdx.x * 4;
    int f[4], cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[i] = k0 + i < n ? colony_is_root(k0 + i, root, size, packed, min_cells) : 0;
        cnt += f[i];
    }
    __shared__ int wcount[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) wcount[w] = x;
    __syncthreads();
    int ws = 0;
    for (int i = 0; i < w; ++i) ws += wcount[i];
    int c = block_off[blockIdx.x] + ws + x - cnt;     // colonies before slot k0
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + i;
        if (k >= n) break;
        if (f[i]) {
            rank[k] = c;               // c < n_colonies <= n <= ld
            cells[c] = size[k];
            colony_key[c] = (int64_t)skey[k];     // a member's key; k_colony_label takes the minimum
            // a large colony's reductions are split over workgroups: list it (at most
            // n / COL_SPLIT of them; the list's order decides only which workgroups serve it)
            if (size[k] > COL_SPLIT) big_list[atomicAdd(n_big, 1)] = c;
            ++c;
        } else {
            rank[k] = -1;
        }
    }
}

__global__ __launch_bounds__(256) void k_colony_label(int n, const int32_t *__restrict__ root,
                                                      const int32_t *__restrict__ rank,
                                                      const int32_t *__restrict__ order,
                                                      const uint32_t *__restrict__ skey,
                                                      int32_t *__restrict__ colony, int64_t *colony_key,
                                                      int32_t *__restrict__ bin2) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    int c = -1;
    if (k < n) {
        c = rank[root[k]];
        colony[order[k]] = c;
        bin2[k] = c >= 0 ? c : n;          // agents of no colony: the last bin
    }
    colony_atomic_by_key(colony_min_op{colony_key}, c >= 0, c, c >= 0 ? (unsigned long long)skey[k] : ~0ull);
}

// col_start[c] = where colony c's run begins in the second sort's order
__global__ __launch_bounds__(256) void k_colony_runs(int n, const int32_t *__restrict__ sorted_col,
                                                     int32_t *__restrict__ col_start) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int c = sorted_col[j];
    if (c < n && (j == 0 || sorted_col[j - 1] != c)) col_start[c] = j;
}

// ---------------------------------------------------------------------------
// the three segmented passes: one kernel, three functors
// ---------------------------------------------------------------------------
// A functor has NV values per member, combined per value by op(i, a, b) from identity(i);
// begin(c) reads what earlier passes left for colony c, term() gives a member's values,
// finish() writes the colony's.

struct colony_sums {      // mass, cell_area, sum x, sum y -> mass, cell_area, cx, cy
    static constexpr int NV = 4;
    const double *mass;
    double mass_const, width;
    double *metrics;
    int64_t ld;
    __device__ void begin(int) {}
    __device__ static double identity(int) { return 0.0; }
    __device__ static double op(int, double a, double b) { return a + b; }
    __device__ void term(int a, const contact_slot &s, const double2, double *v) const {
        v[0] = mass ? mass[a] : mass_const;
        v[1] = width * fmax(s.L - width, 0.0) + 3.141592653589793 * width * width / 4.0;
        v[2] = s.x;
        v[3] = s.y;
    }
    __device__ void finish(int c, int size, const double *t) const {
        metrics[VK_COLONY_MASS * ld + c] = t[0];
        metrics[VK_COLONY_CELL_AREA * ld + c] = t[1];
        metrics[VK_COLONY_CX * ld + c] = t[2] / (double)size;
        metrics[VK_COLONY_CY * ld + c] = t[3] / (double)size;
    }
};

struct colony_moments {   // centred second moments -> sxx, syy, sxy, angle
    static constexpr int NV = 3;
    double *metrics;
    int64_t ld;
    double cx, cy;
    __device__ void begin(int c) {
        cx = metrics[VK_COLONY_CX * ld + c];
        cy = metrics[VK_COLONY_CY * ld + c];
    }
    __device__ static double identity(int) { return 0.0; }
    __device__ static double op(int, double a, double b) { return a + b; }
    __device__ void term(int, const contact_slot &s, const double2, double *v) const {
        const double dx = s.x - cx, dy = s.y - cy;
        v[0] = dx * dx;
        v[1] = dy * dy;
        v[2] = dx * dy;
    }
    __device__ void finish(int c, int, const double *t) const {
        metrics[VK_COLONY_SXX * ld + c] = t[0];
        metrics[VK_COLONY_SYY * ld + c] = t[1];
        metrics[VK_COLONY_SXY * ld + c] = t[2];
        metrics[VK_COLONY_ANGLE * ld + c] = 0.5 * atan2(2.0 * t[2], t[0] - t[1]);
    }
};

struct colony_extents {   // lo and hi along e1 and e2 -> major, minor
    static constexpr int NV = 4;
    double *metrics;
    int64_t ld;
    double width;
    double cx, cy, ex, ey;
    __device__ void begin(int c) {
        cx = metrics[VK_COLONY_CX * ld + c];
        cy = metrics[VK_COLONY_CY * ld + c];
        const double phi = metrics[VK_COLONY_ANGLE * ld + c];
        ex = cos(phi);
        ey = sin(phi);
    }
    __device__ static double identity(int i) { return (i & 1) ? -INFINITY : INFINITY; }
    __device__ static double op(int i, double a, double b) { return (i & 1) ? fmax(a, b) : fmin(a, b); }
    __device__ void term(int, const contact_slot &s, const double2 u, double *v) const {
        const double r = width / 2.0, h = fmax(s.L - width, 0.0) / 2.0;
        const double dx = s.x - cx, dy = s.y - cy;
        const double p1 = dx * ex + dy * ey, q1 = h * fabs(u.x * ex + u.y * ey);
        const double p2 = dy * ex - dx * ey, q2 = h * fabs(u.y * ex - u.x * ey);
        v[0] = (p1 - q1) - r;
        v[1] = (p1 + q1) + r;
        v[2] = (p2 - q2) - r;
        v[3] = (p2 + q2) + r;
    }
    __device__ void finish(int c, int, const double *t) const {
        const double along = t[1] - t[0], across = t[3] - t[2];
        metrics[VK_COLONY_MAJOR * ld + c] = fmax(along, across);
        metrics[VK_COLONY_MINOR * ld + c] = fmin(along, across);
    }
};

// Members [m0, m1) of the run that begins at `start`, combined by one workgroup in the fixed
// order of the header; thread 0 gets the result in t.  Every thread of the workgroup calls it.
template <class F>
__device__ __forceinline__ void colony_reduce_members(const F &f, int start, int m0, int m1,
                                                      const int32_t *__restrict__ order2,
                                                      const int32_t *__restrict__ order,
                                                      const contact_slot *__restrict__ packed,
                                                      const double2 *__restrict__ dir, double *t) {
    double acc[F::NV];
#pragma unroll
    for (int i = 0; i < F::NV; ++i) acc[i] = F::identity(i);
    // at most ceil((m1 - m0) / 256) terms; unrolled so that the loads of four members are in
    // flight together (the combines keep their order)
#pragma unroll 4
    for (int m = m0 + threadIdx.x; m < m1; m += 256) {
        const int k = order2[start + m];
        double v[F::NV];
        f.term(order[k], packed[k], dir[k], v);
#pragma unroll
        for (int i = 0; i < F::NV; ++i) acc[i] = F::op(i, acc[i], v[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < F::NV; ++i) acc[i] = F::op(i, acc[i], __shfl_xor(acc[i], o));
    }
    __shared__ double part[4][F::NV];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < F::NV; ++i) part[threadIdx.x >> 6][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < F::NV; ++i)
            t[i] = F::op(i, F::op(i, F::op(i, part[0][i], part[1][i]), part[2][i]), part[3][i]);
    }
}

// colonies of at most COL_SPLIT members: one workgroup each
template <class F>
__global__ __launch_bounds__(256) void k_colony_reduce(F f, const int32_t *__restrict__ n_colonies,
                                                       const int32_t *__restrict__ col_start,
                                                       const int32_t *__restrict__ cells,
                                                       const int32_t *__restrict__ order2,
                                                       const int32_t *__restrict__ order,
                                                       const contact_slot *__restrict__ packed,
                                                       const double2 *__restrict__ dir) {
    const int c = blockIdx.x;
    if (c >= *n_colonies) return;        // the whole workgroup
    const int size = cells[c];
    if (size > COL_SPLIT) return;        // k_colony_reduce_parts
    f.begin(c);
    double t[F::NV];
    colony_reduce_members(f, col_start[c], 0, size, order2, order, packed, dir, t);
    if (threadIdx.x == 0) f.finish(c, size, t);
}

// part p of large colony big_list[i]: members [p S, (p + 1) S), S = 256 ceil(size / (256 COL_PARTS))
template <class F>
__global__ __launch_bounds__(256) void k_colony_reduce_parts(F f, const int32_t *__restrict__ n_big,
                                                             const int32_t *__restrict__ big_list,
                                                             const int32_t *__restrict__ col_start,
                                                             const int32_t *__restrict__ cells,
                                                             const int32_t *__restrict__ order2,
                                                             const int32_t *__restrict__ order,
                                                             const contact_slot *__restrict__ packed,
                                                             const double2 *__restrict__ dir,
                                                             double *__restrict__ partial) {
    const int i = blockIdx.x / COL_PARTS, p = blockIdx.x - i * COL_PARTS;
    if (i >= *n_big) return;             // the whole workgroup
    const int c = big_list[i], size = cells[c];
    const int S = 256 * ((size + 256 * COL_PARTS - 1) / (256 * COL_PARTS));      // p S <= size + 2^14
    const int m0 = p * S < size ? p * S : size, m1 = m0 + S < size ? m0 + S : size;
    f.begin(c);
    double t[F::NV];
    colony_reduce_members(f, col_start[c], m0, m1, order2, order, packed, dir, t);      // empty: the identity
    if (threadIdx.x == 0) {
#pragma unroll
        for (int v = 0; v < F::NV; ++v) partial[((int64_t)blockIdx.x) * F::NV + v] = t[v];
    }
}

// one thread per large colony: its parts in order, ((P_0 op P_1) op P_2) ... op P_63
template <class F>
__global__ __launch_bounds__(64) void k_colony_reduce_finish(F f, const int32_t *__restrict__ n_big,
                                                             const int32_t *__restrict__ big_list,
                                                             const int32_t *__restrict__ cells,
                                                             const double *__restrict__ partial) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *n_big) return;
    const int c = big_list[i];
    double t[F::NV];
#pragma unroll
    for (int v = 0; v < F::NV; ++v) t[v] = partial[((int64_t)i * COL_PARTS) * F::NV + v];
    for (int p = 1; p < COL_PARTS; ++p) {
#pragma unroll
        for (int v = 0; v < F::NV; ++v) t[v] = F::op(v, t[v], partial[((int64_t)i * COL_PARTS + p) * F::NV + v]);
    }
    f.finish(c, cells[c], t);
}

// one pass: the small colonies, then the parts of the large ones and their combination
template <class F>
static int colony_pass(F f, int64_t n, int min_cells, hipStream_t s, const int32_t *n_colonies, const int32_t *n_big,
                       const int32_t *big_list, const int32_t *col_start, const int32_t *cells,
                       const int32_t *order2, const int32_t *order, const contact_slot *packed, const double2 *dir,
                       double *partial) {
    const dim3 col_grid((unsigned)(n / min_cells > 0 ? n / min_cells : 1));      // >= the colonies there can be
    hipLaunchKernelGGL(k_colony_reduce<F>, col_grid, dim3(256), 0, s, f, n_colonies, col_start, cells, order2, order,
                       packed, dir);
    const int64_t max_big = n / COL_SPLIT;      // >= the large colonies there can be
    if (max_big > 0) {
        hipLaunchKernelGGL(k_colony_reduce_parts<F>, dim3((unsigned)(max_big * COL_PARTS)), dim3(256), 0, s, f, n_big,
                           big_list, col_start, cells, order2, order, packed, dir, partial);
        hipLaunchKernelGGL(k_colony_reduce_finish<F>, dim3((unsigned)((max_big + 63) / 64)), dim3(64), 0, s, f, n_big,
                           big_list, cells, partial);
    }
    return vk::launch_check("k_colony_reduce");
}

extern "C" int vk_colony_metrics(const vk_colonies_params *p, int64_t n, int64_t ld, const double *location,
                                 const double *angle, const double *length, const double *mass,
                                 const int64_t *key, double bound_x, double bound_y, int32_t *colony,
                                 int32_t *n_colonies, int32_t *cells, int64_t *colony_key, double *metrics,
                                 int32_t *flags, void *scratch, int64_t scratch_bytes, vk_stream_t stream) {
    if (!p || n < 0 || n >= INT32_MAX - 1 || ld < n || !n_colonies || !flags || !(bound_x > 0.0) ||
        !(bound_y > 0.0)) {
        vk::set_error("vk_colony_metrics: bad arguments");
        return VK_ERR_ARG;
    }
    if (p->min_cells < 1 || !(p->width > 0.0) || !(p->max_length >= p->width) || !(p->link_gap >= 0.0) ||
        !(p->link_gap < INFINITY) || !(p->max_length < INFINITY) || (!length && !(p->length > 0.0))) {
        vk::set_error("vk_colony_metrics: min_cells >= 1, 0 < width <= max_length, 0 <= link_gap < inf, "
                      "length > 0");
        return VK_ERR_ARG;
    }
    // the grid: a cell edge of at least max_length + link_gap on an axis with more than one cell
    const double reach = p->max_length + p->link_gap;
    if (p->gx < 1 || p->gy < 1 || (int64_t)p->gx * p->gy >= INT32_MAX || (p->gx > 1 && bound_x / p->gx < reach) ||
        (p->gy > 1 && bound_y / p->gy < reach)) {
        vk::set_error("vk_colony_metrics: the grid must be gx = max(1, floor(bound_x / (max_length + link_gap))) "
                      "by gy likewise (cell edges >= max_length + link_gap)");
        return VK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return vk::hip_check(hipMemsetAsync(n_colonies, 0, sizeof(int32_t), s), "hipMemsetAsync(n_colonies)");
    const int64_t g = (int64_t)p->gx * p->gy;
    if (!location || !angle || !colony || !cells || !colony_key || !scratch || ((uintptr_t)scratch & 255) ||
        scratch_bytes < vk_colonies_scratch_bytes(n, g)) {
        vk::set_error("vk_colony_metrics: null array, or scratch not 256-B aligned / smaller than "
                      "vk_colonies_scratch_bytes(n, gx * gy)");
        return VK_ERR_ARG;
    }
    const int64_t nb = (n + COL_BLOCK - 1) / COL_BLOCK;
    char *base = (char *)scratch;
    auto take = [&](int64_t bytes) {
        char *q = base;
        base += align256(bytes);
        return q;
    };
    int32_t *cell = (int32_t *)take(n * 4);
    int32_t *order = (int32_t *)take(n * 4);
    int32_t *sorted_cell = (int32_t *)take(n * 4);
    uint32_t *skey = (uint32_t *)take(n * 4);
    contact_slot *packed = (contact_slot *)take(n * 32);
    double2 *dir = (double2 *)take(n * 16);
    int32_t *cell_start = (int32_t *)take(g * 4);     // cell_end follows: one memset clears both
    int32_t *cell_end = (int32_t *)take(g * 4);
    int32_t *parent = (int32_t *)take(n * 4);
    int32_t *root = (int32_t *)take(n * 4);
    int32_t *size = (int32_t *)take(n * 4);
    int32_t *rank = (int32_t *)take(n * 4);
    int32_t *bin2 = (int32_t *)take(n * 4);
    int32_t *order2 = (int32_t *)take(n * 4);
    int32_t *sorted_col = (int32_t *)take(n * 4);
    int32_t *col_start = (int32_t *)take(n * 4);
    int32_t *block_count = (int32_t *)take((nb + 2) * 4);
    int32_t *n_big = (int32_t *)take(4);
    int32_t *big_list = (int32_t *)take((n / COL_SPLIT + 1) * 4);
    double *partial = (double *)take((n / COL_SPLIT + 1) * COL_PARTS * 4 * 8);
    const int64_t sort_bytes = scratch_bytes - colonies_fixed_bytes(n, g);
    const double edge_x = bound_x / p->gx, edge_y = bound_y / p->gy;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256), scan_grid((unsigned)nb);
    int rc;

    // the grid
    hipLaunchKernelGGL(k_contact_cells, grid, block, 0, s, (int)n, ld, location, length, p->length, edge_x, edge_y,
                       p->gx, p->gy, cell, flags);
    if ((rc = vk::launch_check("k_contact_cells"))) return rc;
    if ((rc = vk_occupancy_sort(cell, key, n, g, order, sorted_cell, base, sort_bytes, stream))) return rc;
    if ((rc = vk::hip_check(hipMemsetAsync(cell_start, 0, (size_t)(2 * align256(g * 4)), s),
                            "hipMemsetAsync(cells)")))
        return rc;
    hipLaunchKernelGGL(k_contact_pack, grid, block, 0, s, (int)n, ld, location, angle, length, p->length, key, order,
                       sorted_cell, packed, dir, skey, cell_start, cell_end);
    if ((rc = vk::launch_check("k_contact_pack"))) return rc;

    // link and union
    hipLaunchKernelGGL(k_colony_init, grid, block, 0, s, (int)n, parent);
    hipLaunchKernelGGL(k_colony_link, grid, block, 0, s, *p, (int)n, packed, dir, sorted_cell, cell_start, cell_end,
                       parent, flags);
    hipLaunchKernelGGL(k_colony_flatten, grid, block, 0, s, (int)n, parent, root);
    if ((rc = vk::launch_check("k_colony_link"))) return rc;

    // census and numbering
    if ((rc = vk::hip_check(hipMemsetAsync(size, 0, (size_t)(n * 4), s), "hipMemsetAsync(size)"))) return rc;
    if ((rc = vk::hip_check(hipMemsetAsync(n_big, 0, 256, s), "hipMemsetAsync(n_big)"))) return rc;
    hipLaunchKernelGGL(k_colony_census, grid, block, 0, s, (int)n, root, size);
    hipLaunchKernelGGL(k_colony_count, scan_grid, block, 0, s, (int)n, root, size, packed, p->min_cells, block_count);
    hipLaunchKernelGGL(k_colony_scan_blocks, dim3(1), block, 0, s, block_count, (int)nb, n_colonies);
    hipLaunchKernelGGL(k_colony_rank, scan_grid, block, 0, s, (int)n, root, size, packed, p->min_cells, block_count,
                       skey, rank, cells, colony_key, big_list, n_big);
    hipLaunchKernelGGL(k_colony_label, grid, block, 0, s, (int)n, root, rank, order, skey, colony, colony_key, bin2);
    if ((rc = vk::launch_check("k_colony_label"))) return rc;
    if (!metrics) return VK_OK;

    // every colony one run in (cell, key) order, then the three passes
    if ((rc = vk_occupancy_sort(bin2, nullptr, n, n + 1, order2, sorted_col, base, sort_bytes, stream))) return rc;
    hipLaunchKernelGGL(k_colony_runs, grid, block, 0, s, (int)n, sorted_col, col_start);
    if ((rc = colony_pass(colony_sums{mass, p->mass, p->width, metrics, ld}, n, p->min_cells, s, n_colonies, n_big,
                          big_list, col_start, cells, order2, order, packed, dir, partial)))
        return rc;
    if ((rc = colony_pass(colony_moments{metrics, ld, 0.0, 0.0}, n, p->min_cells, s, n_colonies, n_big, big_list,
                          col_start, cells, order2, order, packed, dir, partial)))
        return rc;
    return colony_pass(colony_extents{metrics, ld, p->width, 0.0, 0.0, 0.0, 0.0}, n, p->min_cells, s, n_colonies,
                       n_big, big_list, col_start, cells, order2, order, packed, dir, partial);
}
