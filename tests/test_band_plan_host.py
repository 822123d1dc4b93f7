"""The banded form of the 10-deep block plan (vk_plan::plan_lanes in
lens_amd/csrc/vk_pass_plan.h) through vk_diffuse_plan_lanes: host only, no GPU.

A whole-plane step of P 10-deep pair-sum passes, with vk_set_stencil_bands(2, m_0),
lists every pass twice: a top band T_p = rows [0, m_0 - 10 p) on lane 0 and a bottom
band B_p = the rest of the plane on lane 1, B_p `after` T_p-1.  Everything here is
checked from the lists alone: the order the launch loop guarantees is "earlier in the
same lane" plus the `after` edges, closed transitively, and under that order alone
every pass must read what the pass before it wrote, and write nothing that a pass not
ordered against it reads or writes.

Grid: planes of 300, 1024 and 4096 rows, n_sub in {20, 30, 100}, variants 20 and 70,
m_0 from the smallest valid value (10 P: the last top band is one pass depth) to the
largest (N - 1: the first bottom band is one row).
"""

import ctypes

import numpy as np
import pytest

FIELD = 0
ALL, INTERIOR = 0, 1
PS10, PS10_ALIGNED = 5, 6
VK_OK = 0
CAPACITY = 256
PLANES = (300, 1024, 4096)
N_SUBS = (20, 30, 100)
VARIANTS = (20, 70)


def top_rows_of(n, n_sub):
    p = n_sub // 10
    picks = {10 * p, 10 * p + 1, 10 * p + 7, int(0.40 * n), int(0.45 * n), n // 2, int(0.55 * n), n - 11, n - 1}
    return sorted(m for m in picks if 10 * p <= m < n)


@pytest.fixture(scope='module')
def lib():
    from lens_amd import native
    from lens_amd.build import build
    build(verbose=False)
    lib = ctypes.CDLL(native.LIB_PATH)
    names = ('vk_diffuse_plan', 'vk_diffuse_plan_lanes', 'vk_set_stencil_mode', 'vk_set_stencil_depth',
             'vk_set_stencil_kernel', 'vk_set_stencil_bands')
    for name in names:
        getattr(lib, name).argtypes, getattr(lib, name).restype = native._SIGS[name]
    saved = (lib.vk_set_stencil_mode(-1), lib.vk_set_stencil_depth(0), lib.vk_set_stencil_kernel(-1, -1),
             lib.vk_set_stencil_bands(-1, 0))
    assert saved[3] == 0                        # the default is the automatic rule
    lib.vk_set_stencil_mode(1)
    lib.vk_set_stencil_depth(10)
    yield lib
    lib.vk_set_stencil_mode(saved[0])
    lib.vk_set_stencil_depth(saved[1])
    lib.vk_set_stencil_kernel(saved[2], 0)
    lib.vk_set_stencil_bands(0, 0)


def whole(n, n_sub, coupled=0):
    return (0, n, 0, n, 1, 1, 0, n_sub, n_sub, ALL, 0, coupled)


def plan(lib, shape):
    """vk_diffuse_plan's list as tuples of 13."""
    from lens_amd import native
    buf = (native.VkPass * CAPACITY)()
    n = ctypes.c_int32(0)
    rc = lib.vk_diffuse_plan(*shape, buf, CAPACITY, ctypes.byref(n))
    assert n.value <= CAPACITY
    ints = (ctypes.c_int32 * (13 * CAPACITY)).from_buffer(buf)
    return rc, [tuple(ints[13 * i:13 * i + 13]) for i in range(n.value)]


def plan_lanes(lib, shape):
    from lens_amd import native
    buf = (native.VkPass * CAPACITY)()
    lane = (ctypes.c_int32 * CAPACITY)(*([-7] * CAPACITY))
    after = (ctypes.c_int32 * CAPACITY)(*([-7] * CAPACITY))
    n = ctypes.c_int32(0)
    rc = lib.vk_diffuse_plan_lanes(*shape, buf, lane, after, CAPACITY, ctypes.byref(n))
    assert n.value <= CAPACITY
    ints = (ctypes.c_int32 * (13 * CAPACITY)).from_buffer(buf)
    return rc, [tuple(ints[13 * i:13 * i + 13]) for i in range(n.value)], list(lane[:n.value]), list(after[:n.value])


def ordered_before(lane, after):
    """before[i, j]: pass i has finished when pass j starts -- same lane and earlier, or
    an `after` edge, closed transitively."""
    n = len(lane)
    before = np.zeros((n, n), dtype=bool)
    for j in range(n):
        for i in range(j):
            before[i, j] = lane[i] == lane[j]
        if after[j] >= 0:
            assert after[j] < j and lane[after[j]] != lane[j]     # recorded before it is waited for
            before[after[j], j] = True
    for k in range(n):                                             # Warshall
        before |= np.outer(before[:, k], before[k, :])
    return before


def overlap(a, b):
    return max(a[0], b[0]) < min(a[1], b[1])


def check_banded(n, n_sub, m0, unbanded, passes, lane, after):
    P = n_sub // 10
    assert len(unbanded) == P and len(passes) == 2 * P
    tops = [i for i in range(2 * P) if lane[i] == 0]
    bots = [i for i in range(2 * P) if lane[i] == 1]
    assert len(tops) == len(bots) == P and set(lane) == {0, 1}
    number = np.empty(2 * P, dtype=np.int64)            # which of the step's P passes a launch belongs to
    for p, (t, b, u) in enumerate(zip(tops, bots, unbanded)):
        number[t] = number[b] = p
        T, B = passes[t], passes[b]
        # the two bands partition the plane, at a boundary 10 rows higher per pass
        assert (T[4], T[5], B[4], B[5]) == (0, m0 - 10 * p, m0 - 10 * p, n), (p, T, B)
        for q in (T, B):
            # the same pass but for its rows; inputs = the rows grown by the depth, clipped to the plane
            assert q[:4] == u[:4] and q[8:] == u[8:] and q[10] in (PS10, PS10_ALIGNED)
            assert (q[6], q[7]) == (max(0, q[4] - 10), min(n, q[5] + 10))
        assert after[t] == -1                            # the top chain never waits for the bottom lane
        assert after[b] == (tops[p - 1] if p else -1)
    before = ordered_before(lane, after)
    assert not (before & before.T).any()
    for j, q in enumerate(passes):
        src, in_lo, in_hi = q[1], q[6], q[7]
        # the latest write, among the passes ordered before j, to each row of the buffer j reads
        # (list order extends the partial order, and two writers of one row are ordered: below)
        latest = np.full(n, -1, dtype=np.int64)
        for i in range(j):
            if before[i, j] and passes[i][2] == src:
                latest[passes[i][4]:passes[i][5]] = number[i]
        assert (latest[in_lo:in_hi] == number[j] - 1).all(), (j, q)     # (-1: the step-start field)
        for i in range(2 * P):
            if i == j or before[i, j] or before[j, i]:
                continue
            w = passes[i]
            # not ordered against j: what i writes, j neither reads nor writes in that buffer
            assert not (w[2] == src and overlap((w[4], w[5]), (in_lo, in_hi))), (i, j)
            assert not (w[2] == q[2] and overlap((w[4], w[5]), (q[4], q[5]))), (i, j)
    # the step ends in the field, whole
    assert passes[tops[-1]][2] == passes[bots[-1]][2] == FIELD and passes[tops[0]][1] == FIELD


@pytest.mark.parametrize('variant', VARIANTS)
def test_forced_bands_keep_every_dependency(lib, variant):
    lib.vk_set_stencil_kernel(variant, 0)
    checked = 0
    for n in PLANES:
        for n_sub in N_SUBS:
            lib.vk_set_stencil_bands(1, 0)
            rc, unbanded = plan(lib, whole(n, n_sub))
            assert rc == VK_OK and [p[0] for p in unbanded] == [10] * (n_sub // 10)
            assert 10 * (n_sub // 10) in top_rows_of(n, n_sub)       # the smallest valid m_0
            for m0 in top_rows_of(n, n_sub):
                assert lib.vk_set_stencil_bands(2, m0) in (1, 2)
                assert lib.vk_set_stencil_bands(-1, 0) == 2
                rc, passes, lane, after = plan_lanes(lib, whole(n, n_sub))
                assert rc == VK_OK
                check_banded(n, n_sub, m0, unbanded, passes, lane, after)
                assert plan(lib, whole(n, n_sub)) == (VK_OK, passes)  # vk_diffuse_plan: what would launch
                checked += 1
    assert checked >= 60


def test_bad_top_rows_fall_back_to_the_unbanded_plan(lib):
    lib.vk_set_stencil_kernel(70, 0)
    for n in PLANES:
        for n_sub in N_SUBS:
            lib.vk_set_stencil_bands(1, 0)
            rc, unbanded = plan(lib, whole(n, n_sub))
            P = n_sub // 10
            for m0 in (1, 9, 10 * P - 10, 10 * P - 1, n, n + 1, 2 * n):   # T_P-1 under 10 rows / B_0 empty
                lib.vk_set_stencil_bands(2, m0)
                assert plan_lanes(lib, whole(n, n_sub)) == (VK_OK, unbanded, [0] * P, [-1] * P), (n, n_sub, m0)
    lib.vk_set_stencil_bands(1, 0)
    assert lib.vk_set_stencil_bands(2, 0) == 1 and lib.vk_set_stencil_bands(-1, 0) == 1   # no rows: ignored


AUTO = {(70, 4096, 100): 1638}     # (variant, rows, n_sub): the one shape the automatic rule bands, and its m_0


def test_off_and_default_give_the_unbanded_plan(lib):
    """Bands off, and the default (the automatic rule) for every shape but the rule's own:
    vk_diffuse_plan's list as it was, all on lane 0.  The rule's shape -- the C4 step --
    comes out as the forced plan with its m_0."""
    shapes = [whole(n, n_sub) for n in PLANES + (40, 4095, 4097) for n_sub in N_SUBS + (7, 93, 90, 110, 1001)]
    auto_seen = set()
    for variant in (20, 40, 70):
        lib.vk_set_stencil_kernel(variant, 0)
        for shape in shapes:
            lib.vk_set_stencil_bands(1, 0)
            rc, off = plan(lib, shape)
            assert rc == VK_OK
            assert plan_lanes(lib, shape) == (VK_OK, off, [0] * len(off), [-1] * len(off))
            lib.vk_set_stencil_bands(0, 0)
            m0 = AUTO.get((variant, shape[1], shape[8]))
            if m0 is None:
                assert plan(lib, shape) == (VK_OK, off), (variant, shape)
                assert plan_lanes(lib, shape) == (VK_OK, off, [0] * len(off), [-1] * len(off))
                continue
            auto_seen.add((variant, shape[1], shape[8]))
            got = plan_lanes(lib, shape)
            lib.vk_set_stencil_bands(2, m0)
            assert got == plan_lanes(lib, shape) and set(got[2]) == {0, 1}
            check_banded(shape[1], shape[8], m0, off, *got[1:])
    assert auto_seen == set(AUTO)
    # the rule bands the uncoupled whole-plane step only
    lib.vk_set_stencil_kernel(70, 0)
    for shape in (whole(4096, 100, 1), whole(4096, 100, 2), (0, 4096, 0, 4096, 1, 1, 0, 50, 100, ALL, 0, 0),
                  (10, 4106, 0, 4116, 0, 0, 0, 100, 100, ALL, 0, 0), (0, 4096, 0, 4106, 1, 0, 0, 10, 100, ALL, 0, 0)):
        lib.vk_set_stencil_bands(1, 0)
        rc, off = plan(lib, shape)
        assert rc == VK_OK and off
        lib.vk_set_stencil_bands(0, 0)
        assert plan_lanes(lib, shape) == (VK_OK, off, [0] * len(off), [-1] * len(off)), shape


def test_only_the_uncoupled_whole_plane_pair_sum_step_is_banded(lib):
    """Forced bands leave every other call as it is: coupled steps, a block of a step,
    row bands and their parts, the stage-split pass, other depths, the exact mode."""
    n, m0 = 300, 140
    others = [
        (70, 1, 10, whole(n, 100, 1)), (70, 1, 10, whole(n, 100, 2)),            # coupled
        (70, 1, 10, (0, n, 0, n, 1, 1, 0, 50, 100, ALL, 0, 0)),                   # not the whole step
        (70, 1, 10, (20, n - 20, 0, n, 0, 0, 0, 20, 100, ALL, 0, 0)),             # a middle row band's block
        (70, 1, 10, (0, n - 20, 0, n, 1, 0, 0, 20, 100, ALL, 0, 0)),              # a top row band's
        (70, 1, 10, (20, n - 20, 0, n, 0, 0, 0, 20, 100, INTERIOR, 0, 0)),        # a part
        (40, 1, 10, whole(n, 100)),                                               # the stage-split pass
        (70, 1, 9, whole(n, 100)), (70, 1, 10, whole(n, 93)),                     # odd depths
        (70, 0, 10, whole(n, 100)),                                               # the exact mode
    ]
    for variant, mode, depth, shape in others:
        lib.vk_set_stencil_kernel(variant, 0)
        lib.vk_set_stencil_mode(mode)
        lib.vk_set_stencil_depth(depth)
        lib.vk_set_stencil_bands(1, 0)
        rc, off = plan(lib, shape)
        assert rc == VK_OK and off
        lib.vk_set_stencil_bands(2, m0)
        assert plan_lanes(lib, shape) == (VK_OK, off, [0] * len(off), [-1] * len(off)), (variant, mode, depth, shape)
    lib.vk_set_stencil_mode(1)
    lib.vk_set_stencil_depth(10)
    lib.vk_set_stencil_kernel(70, 0)
    rc, passes, lane, after = plan_lanes(lib, whole(n, 100))      # (and the plain step under the same setting is)
    assert rc == VK_OK and len(passes) == 20 and set(lane) == {0, 1}
