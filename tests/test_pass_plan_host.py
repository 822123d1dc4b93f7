"""The diffusion pass planner (lens_amd/csrc/vk_pass_plan.h) through vk_diffuse_plan:
host only, no GPU.

tests/golden/stencil_pass_plans.json holds the plans of commit 1088b26, the last one
whose vk_lattice.hip planned and launched in one function.  It was recorded from a
scratch copy of that commit's planning code (its globals and setters, launch_pass,
odd_plan, vk_diffuse, vk_diffuse_part, diffuse_impl, vk_diffuse_coupled) compiled
into a stand-alone program in which only the launch sites were replaced: the
vk_launch_* functions, the k_diffuse_substep launch and the k_copy_rows launch
appended a descriptor instead of launching (the stage-split launcher declining
exactly as vk_stencil_sp.hip did).  The program ran the grid below -- every
combination of the settings with the call shapes -- and a script folded its output
into tables: `passes` (descriptors without the kernel), `pass_lists` and
`kernel_lists` (run-length coded as [repeat, pattern] pieces), `plans` (a pass list
and a kernel list), and per setting a row of one entry per shape, a plan or minus
the status.  The recorder is not in the repository; the file never came from the
planner under test.

Grid: mode {exact, fma} x depth {1, 3, 5, 7, 9, 10, 11, 13, 15} x variant {2, 3, 6,
20, 40, 70} x rows {0, 8, 64} (settings that cannot change a plan share a row of
the file); whole planes of 40 and 300 rows with n_sub in {1, 2, 3, 7, 10, 11, 18, 20,
30, 50, 93, 100, 501, 1001}, plain, coupled without agents and coupled with agents;
bands of 300 owned rows (top edge, middle, bottom edge) stepping n_sub = 100 in halo
blocks of {5, 7, 8, 20, 50, 100} substeps, every block, as VK_PART_ALL and as
INTERIOR / EDGES with interior_passes in {0, 1, 3, 10}; middle bands of 40 rows with
blocks of 20 and of 100 rows with blocks of 50 (no more than 2 sub_count rows: the
parts must get VK_ERR_LIMIT).
"""

import ctypes
import json
import os
from types import SimpleNamespace

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'stencil_pass_plans.json')
FIELD, WORK0, WORK1 = 0, 1, 2
ALL, INTERIOR, EDGES = 0, 1, 2
PS10_STRIPS = 7
VK_OK, VK_ERR_LIMIT = 0, 3
CAPACITY = 1024

# Coupled steps of an odd number (>= 3) of 10-deep passes: vk_diffuse_coupled used to
# rotate work0, work1, work0, ..., field on its own; it now takes vk_diffuse's backward
# assignment, which for an odd count starts in work1.  Only the scratch buffer ids of
# these plans may differ from the golden: (mode, depth, n_sub) of the coupled shapes.
ROTATED = {(1, 10, 30), (1, 10, 50)}


def unrle(pieces):
    out = []
    for n, pattern in pieces:
        out.extend(pattern * n)
    return out


@pytest.fixture(scope='module')
def lib():
    from lens_amd import native
    from lens_amd.build import build
    build(verbose=False)
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in ('vk_diffuse_plan', 'vk_set_stencil_mode', 'vk_set_stencil_depth', 'vk_set_stencil_kernel'):
        getattr(lib, name).argtypes, getattr(lib, name).restype = native._SIGS[name]
    saved = (lib.vk_set_stencil_mode(-1), lib.vk_set_stencil_depth(0), lib.vk_set_stencil_kernel(-1, -1))
    yield lib
    lib.vk_set_stencil_mode(saved[0])
    lib.vk_set_stencil_depth(saved[1])
    lib.vk_set_stencil_kernel(saved[2], 0)     # (the rows have no query: back to auto, the default)


@pytest.fixture(scope='module')
def golden():
    g = json.load(open(GOLDEN))
    names = g['pass_fields']
    assert names == ['k', 'src', 'dst', 'f0', 'lo', 'hi', 'in_lo', 'in_hi', 'gap_lo', 'gap_hi', 'couple', 'copy_back']
    pass_lists = [unrle(p) for p in g['pass_lists']]
    kernel_lists = [unrle(p) for p in g['kernel_lists']]
    plans = []
    for pl, kl in g['plans']:
        assert len(pass_lists[pl]) == len(kernel_lists[kl])
        # in the library's field order: the kernel sits between gap_hi and couple
        plans.append(tuple(tuple(g['passes'][i][:10]) + (k,) + tuple(g['passes'][i][10:])
                           for i, k in zip(pass_lists[pl], kernel_lists[kl])))
    shapes = [tuple(g['calls'][c]) + (part, ip, coupled) for c, part, ip, coupled in g['shapes']]
    rows = [unrle(r) for r in g['rows']]
    assert all(len(r) == len(shapes) for r in rows)
    return SimpleNamespace(settings=[tuple(s) for s in g['settings']], setting_row=g['setting_row'], shapes=shapes,
                           plans=plans, rows=rows)


@pytest.fixture(scope='module')
def planned(lib, golden):
    """(status, passes) of every grid case from the library: [setting][shape]."""
    from lens_amd import native
    buf = (native.VkPass * CAPACITY)()
    n = ctypes.c_int32(0)
    ints = (ctypes.c_int32 * (13 * CAPACITY)).from_buffer(buf)
    cache, out = {}, []
    for mode, depth, variant, rows in golden.settings:
        assert lib.vk_set_stencil_mode(mode) in (0, 1)
        lib.vk_set_stencil_depth(depth)
        lib.vk_set_stencil_kernel(variant, rows)
        assert (lib.vk_set_stencil_mode(-1), lib.vk_set_stencil_depth(0)) == (mode, depth)
        assert lib.vk_set_stencil_kernel(-1, rows) == variant
        res = []
        for shape in golden.shapes:
            rc = lib.vk_diffuse_plan(*shape, buf, CAPACITY, ctypes.byref(n))
            assert n.value <= CAPACITY
            flat = tuple(ints[:13 * n.value])
            if flat not in cache:
                cache[flat] = tuple(flat[i:i + 13] for i in range(0, len(flat), 13))
            res.append((rc, cache[flat]))
        out.append(res)
    return out


def test_plans_equal_the_parent_commits(golden, planned):
    rotated_seen = set()
    for si, setting in enumerate(golden.settings):
        row = golden.rows[golden.setting_row[si]]
        for ci, shape in enumerate(golden.shapes):
            rc, got = planned[si][ci]
            entry = row[ci]
            if entry < 0:
                assert (rc, got) == (-entry, ()), (setting, shape)
                continue
            want = golden.plans[entry]
            assert rc == VK_OK, (setting, shape)
            if got != want and shape[11] and (setting[0], setting[1], shape[8]) in ROTATED:
                rotated_seen.add((setting[0], setting[1], shape[8]))
                mask = lambda plan: tuple(p[:1] + p[3:] for p in plan)   # all but src, dst
                assert mask(got) == mask(want), (setting, shape)
                assert [p[2] for p in got][-1] == FIELD and got[0][1] == FIELD
                continue
            assert got == want, (setting, shape)
    assert rotated_seen == ROTATED


def state_buffer(j):
    from lens_amd.lattice import Lattice
    return Lattice.state_buffer(SimpleNamespace(fields=FIELD, work0=WORK0, work1=WORK1), j)


def written_rows(p):
    lo, hi, gap_lo, gap_hi = p[4], p[5], p[8], p[9]
    return [(lo, gap_lo), (gap_hi, hi)] if gap_lo >= 0 else [(lo, hi)]


def check_whole_plan(mode, shape, plan):
    """The invariants of a VK_PART_ALL (or coupled) plan."""
    row_lo, row_hi, lo_min, hi_max, _, _, sub_begin, sub_count, n_sub = shape[:9]
    last = sub_begin + sub_count - 1
    ends_step = sub_begin + sub_count == n_sub
    assert sum(p[0] for p in plan) == sub_count
    if not plan:
        return
    assert plan[0][1] == state_buffer(sub_begin)
    j = sub_begin
    for i, p in enumerate(plan):
        k, src, dst, f0, lo, hi, in_lo, in_hi, gap_lo, gap_hi, kernel, couple, copy_back = p
        assert src != dst
        if i:
            assert src == plan[i - 1][2]
        e = j + k - 1
        g = last - e
        assert (lo, hi) == (max(lo_min, row_lo - g), min(hi_max, row_hi + g)) and gap_lo < 0
        assert (in_lo, in_hi) == (max(lo_min, lo - k), min(hi_max, hi + k))
        final = ends_step and i == len(plan) - 1
        if copy_back:
            assert len(plan) == 1 and sub_begin == 0 and ends_step and (src, dst) == (FIELD, WORK0)
        assert bool(copy_back) == (len(plan) == 1 and sub_begin == 0 and ends_step)
        if mode == 0:
            assert bool(f0) == final
            assert (dst == FIELD) == (final and not copy_back)
        j += k
    end = plan[-1][2]
    if plan[-1][12]:
        assert end == WORK0     # and its owned rows are copied to the field
    else:
        assert end == (FIELD if ends_step else state_buffer(sub_begin + sub_count))


def test_every_plan_keeps_the_invariants(golden, planned):
    checked = set()
    for si, (mode, depth, variant, rows) in enumerate(golden.settings):
        by_shape = dict(zip(golden.shapes, planned[si]))
        for shape, (rc, plan) in by_shape.items():
            part, ip, coupled = shape[9:]
            if rc != VK_OK or (mode, shape, plan) in checked:
                continue
            checked.add((mode, shape, plan))
            if part == ALL:
                check_whole_plan(mode, shape, plan)
                continue
            # a part: its passes are the whole block's, on some of their rows
            rc_all, whole = by_shape[shape[:9] + (ALL, 0, 0)]
            assert rc_all == VK_OK and all(p[0] == 10 for p in whole)
            P = len(whole)
            m = P if ip <= 0 or ip > P else ip
            _, interior = by_shape[shape[:9] + (INTERIOR, ip, 0)]
            _, edges = by_shape[shape[:9] + (EDGES, ip, 0)]
            assert len(interior) == m
            rest = list(edges)
            for p in range(P):
                w = whole[p]
                if p >= m:
                    assert rest.pop(0) == w
                    continue
                pieces, e = [], interior[p]
                while True:
                    # the same pass (depth, buffers, base), its inputs the rows grown by k
                    assert e[:4] == w[:4]
                    assert (e[6], e[7]) == (max(shape[2], e[4] - 10), min(shape[3], e[5] + 10))
                    assert (e[10] == PS10_STRIPS) == (e[8] >= 0)
                    pieces += written_rows(e)
                    if sum(hi - lo for lo, hi in pieces) >= w[5] - w[4]:
                        break
                    e = rest.pop(0)
                pieces.sort()
                assert all(lo < hi for lo, hi in pieces)
                assert pieces[0][0] == w[4] and pieces[-1][1] == w[5]
                assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))   # disjoint, and no row missing
            assert not rest
    assert len(checked) > 1000
