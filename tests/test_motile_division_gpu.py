"""Motile agents that grow and divide: vk_flagella_counts and vk_divide_flagella at the
ABI level, and Colony(cells=..., motility=MotilityModel(division=...)) against the NumPy
restatement tests/motile_division_ref.py (draws from oracle.colony.philox_uniform).

The ints (counts, masks, keys, agent ids, bins) must be exactly equal, the expression rows
and the counts derived from them bitwise (+ - x only, -ffp-contract=off on both sides).
The other FP64 rows come out of vk_flagella_step and get the bound tests/test_flagella_gpu.py
derives for that kernel, 1e-12 (absolute for CheY, CheY_P, cw_bias, angle and torque,
relative for P_on, n_methyl, the cell rows and mmol_to_counts, relative to the bound for
locations) -- taken here for the whole 300-update trajectory, not per update: the test
prints the largest deviation of every row.  Exact agreement on the discrete results is
required where the restatement's own decisions are not ties: every margin (switch and
structural draws, bin edges, the coin of an odd count) is >= 1e-9, asserted on the
restatement alone; the seed of the case was chosen on the CPU so that this holds with no
agent left out (tests/test_motile_division_host.py runs the same case).

The whole-colony case (motile_division_ref.colony_case): 24 agents on 16 x 16 bins with the
planes glc__D_e, lcts_e and MeAsp (nothing exchanges with MeAsp: it only diffuses), steps of
1 s in 10 inner updates, GrowthProtein at rate 0.05, capacity 128."""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import flagella_ref as fref
import motile_division_ref as ref

pytestmark = pytest.mark.gpu

BOUND = 1e-12
FI = ref.FI
STEPS = 30


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lens_amd import native
    native.load()
    return torch.device('cuda', 0)


def _stream():
    from lens_amd import native
    return native.stream_handle()


# -- vk_flagella_counts ----------------------------------------------------------------------

def _count_cases(n, rng):
    """(conc, m2c) with products in [0, 33): zeros, k / m2c for k = 0..33 and its two
    neighbours (products just below, at and just above whole numbers), random values, and
    in the last element the largest concentration whose product stays below 33."""
    m2c = rng.uniform(5e5, 2e6, n)
    conc = (np.arange(n) % 34).astype(np.float64) / m2c
    kind = np.arange(n) // 34 % 4
    conc = np.where(kind == 1, np.nextafter(conc, -np.inf), conc)
    conc = np.where(kind == 2, np.nextafter(conc, np.inf), conc)
    conc = np.where(kind == 3, rng.uniform(0.0, 33.0, n) / m2c, conc)
    conc = np.where((conc * m2c >= 0.0) & (conc * m2c < 33.0), conc, 0.0)      # k = 33, and roundings across an end
    if n > 1:
        c = 33.0 / m2c[-1]
        while c * m2c[-1] >= 33.0:
            c = np.nextafter(c, 0.0)
        conc[-1] = c                                 # 32.999...
    return conc, m2c


def _counts(dev, conc, m2c, flags=0):
    from lens_amd import native
    n = len(conc)
    c = torch.from_numpy(np.ascontiguousarray(conc)).to(dev)
    m = torch.from_numpy(np.ascontiguousarray(m2c)).to(dev)
    target = torch.full((n + 3,), -7, dtype=torch.int32, device=dev)
    flag = torch.tensor([flags], dtype=torch.int32, device=dev)
    native.check(native._lib.vk_flagella_counts(n, native.ptr(c), native.ptr(m), native.ptr(target), native.ptr(flag),
                                                _stream()), 'vk_flagella_counts')
    torch.cuda.synchronize()
    assert (target[n:] == -7).all()
    return target[:n].cpu().numpy(), int(flag[0])


@pytest.mark.parametrize('n', [0, 1, 1000])
def test_flagella_counts_equal_trunc(dev, n):
    rng = np.random.default_rng(20261020 + n)
    conc, m2c = _count_cases(n, rng)
    want, flagged = ref.flagella_counts(conc, m2c)
    assert not flagged
    got, flag = _counts(dev, conc, m2c)
    assert np.array_equal(got, want) and flag == 0
    if n:
        with np.errstate(invalid='ignore'):
            assert np.array_equal(got, np.trunc(conc * m2c).astype(np.int32))        # no clamp was needed
    if n == 1000:
        assert set(range(33)) <= set(got.tolist())
        assert ((conc * m2c == np.round(conc * m2c)) & (conc > 0)).any()             # products at whole numbers
        assert conc[-1] * m2c[-1] == np.nextafter(33.0, 0.0) and got[-1] == 32
    # outside [0, 33): each kind alone sets the flag word, and the value is clamped
    for value, clamped in ((33.0, 32), (1e9, 32), (-0.5, 0), (-3.0, 0), (np.nan, 0), (np.inf, 32), (-np.inf, 0)):
        c2, m2 = np.append(conc, value), np.append(m2c, 1.0)
        want, flagged = ref.flagella_counts(c2, m2)
        got, flag = _counts(dev, c2, m2)
        assert flagged and flag == 1 and np.array_equal(got, want) and got[-1] == clamped, value
    # the word is only ever set: a clean launch leaves a raised flag alone
    assert _counts(dev, conc, m2c, flags=1)[1] == 1
    # -0.0 and 32.999... are inside
    got, flag = _counts(dev, np.array([-0.0, 32.999 / 7e5]), np.array([7e5, 7e5]))
    assert got.tolist() == [0, 32] and flag == 0


def test_flagella_counts_bad_arguments(dev):
    from lens_amd import native
    a = torch.zeros(4, dtype=torch.float64, device=dev)
    t = torch.full((4,), -7, dtype=torch.int32, device=dev)
    f = torch.zeros(1, dtype=torch.int32, device=dev)
    call = native._lib.vk_flagella_counts
    for args in ((-1, native.ptr(a), native.ptr(a), native.ptr(t), native.ptr(f)),
                 (4, 0, native.ptr(a), native.ptr(t), native.ptr(f)),
                 (4, native.ptr(a), 0, native.ptr(t), native.ptr(f)),
                 (4, native.ptr(a), native.ptr(a), 0, native.ptr(f)),
                 (4, native.ptr(a), native.ptr(a), native.ptr(t), 0)):
        assert call(*args, _stream()) == native.VK_ERR_ARG
    torch.cuda.synchronize()
    assert (t == -7).all() and int(f[0]) == 0


# -- vk_divide_flagella ----------------------------------------------------------------------

def _plan(dev, divide):
    from lens_amd import native
    n = len(divide)
    d = torch.from_numpy(divide.astype(np.int32)).to(dev)
    src = torch.full((2 * n,), -7, dtype=torch.int32, device=dev)
    kind = torch.full((2 * n,), -7, dtype=torch.int32, device=dev)
    n_out = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(int(native._lib.vk_divide_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    native.check(native._lib.vk_divide_plan(native.ptr(d), n, native.ptr(src), native.ptr(kind), native.ptr(n_out),
                                            native.ptr(scratch), _stream()), 'vk_divide_plan')
    return src, kind, int(n_out.item())


def _divide(dev, mode, flag_int, keys, lineage, divide, ld_dst, seed, step, key_base):
    from lens_amd import native
    from lens_amd.motility import DIVISION_MODES
    n = flag_int.shape[1]
    src, kind, n_out = _plan(dev, divide)
    n_keep = 2 * n - n_out
    fi = torch.from_numpy(flag_int).to(dev).contiguous()
    k = torch.from_numpy(keys).to(dev)
    root, depth, path = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in lineage)
    fi_dst = torch.full((3, ld_dst), -7, dtype=torch.int32, device=dev)
    k_dst = torch.full((ld_dst,), -7, dtype=torch.int64, device=dev)
    native.check(native._lib.vk_divide_flagella(
        n_out, n_keep, n, native.ptr(src), native.ptr(kind), native.ptr(fi), n, native.ptr(k), native.ptr(root),
        native.ptr(depth), native.ptr(path), native.ptr(fi_dst), ld_dst, native.ptr(k_dst), DIVISION_MODES[mode], seed,
        step, key_base, _stream()), 'vk_divide_flagella')
    torch.cuda.synchronize()
    assert (fi_dst[:, n_out:] == -7).all() and (k_dst[n_out:] == -7).all()          # the padding is untouched
    return fi_dst[:, :n_out].cpu().numpy(), k_dst[:n_out].cpu().numpy(), src[:n_out].cpu().numpy().astype(np.int64), n_keep


def _divide_state(n, rng):
    have, target = rng.integers(0, 33, n), rng.integers(0, 33, n)
    for k, (a, b) in enumerate([(a, b) for a in (0, 1, 31, 32) for b in (0, 1, 31, 32)][:n]):
        have[k], target[k] = a, b
    mask = rng.integers(0, 2 ** 32, n, dtype=np.uint64) & ((np.uint64(1) << have.astype(np.uint64)) - np.uint64(1))
    flag_int = np.stack([target.astype(np.int32), have.astype(np.int32), mask.astype(np.uint32).view(np.int32)])
    keys = rng.permutation(5 * n + 7)[:n].astype(np.int64)
    depth = rng.integers(0, 4, n).astype(np.int32)
    path = (rng.integers(0, 8, n) & ((1 << depth) - 1)).astype(np.int64)
    root = rng.permutation(n).astype(np.int32)
    return flag_int, keys, (root, depth, path)


def _popcount(x):
    return np.array([bin(int(v)).count('1') for v in x])


@pytest.mark.parametrize('mode', ['merged', 'split_dict'])
def test_divide_flagella_equals_the_restatement(dev, mode):
    n, ld_dst, seed, step, key_base = 1000, 1700, 20261020, 41, 5 * 1000 + 7
    rng = np.random.default_rng(7)
    flag_int, keys, lineage = _divide_state(n, rng)
    divide = rng.random(n) < 0.5
    divide[:16] = np.arange(16) % 2 == 0                 # mothers and survivors among the special counts
    got_fi, got_keys, order, n_keep = _divide(dev, mode, flag_int, keys, lineage, divide, ld_dst, seed, step, key_base)
    keep, moth = np.flatnonzero(~divide), np.flatnonzero(divide)
    assert np.array_equal(order, np.concatenate([keep, np.repeat(moth, 2)])) and n_keep == len(keep)
    assert 400 < len(moth) < 600 and (lineage[1][moth] > 0).any() and len(order) > n
    margins = {}
    want_fi, want_keys = ref.divide_flagella(flag_int, keys, order, n_keep, mode, seed, step, lineage, key_base, margins)
    assert margins['split'] >= 1e-9
    assert np.array_equal(got_fi, want_fi) and np.array_equal(got_keys, want_keys)
    # invariants, on the device result
    assert np.array_equal(got_fi[:, :n_keep], flag_int[:, keep]) and np.array_equal(got_keys[:n_keep], keys[keep])
    d0, d1, mother = got_fi[:, n_keep::2], got_fi[:, n_keep + 1::2], flag_int[:, moth]
    assert np.array_equal(d0[FI['target']] + d1[FI['target']], mother[FI['target']])
    assert (np.abs(d0[FI['target']] - d1[FI['target']]) <= 1).all()
    odd = mother[FI['target']] % 2 == 1
    assert (d0[FI['target']][odd] > d1[FI['target']][odd]).any() and (d0[FI['target']][odd] < d1[FI['target']][odd]).any()
    m0, m1, mm = (x[FI['mask']].view(np.uint32) for x in (d0, d1, mother))
    if mode == 'split_dict':
        assert np.array_equal(d0[FI['have']] + d1[FI['have']], mother[FI['have']])
        assert np.array_equal(_popcount(m0) + _popcount(m1), _popcount(mm))
        assert np.array_equal(d1[FI['have']], mother[FI['have']] // 2)
    else:
        for d in (d0, d1):
            assert np.array_equal(d[FI['have']], mother[FI['have']]) and np.array_equal(d[FI['mask']], mother[FI['mask']])
    masks, haves = got_fi[FI['mask']].view(np.uint32).astype(np.uint64), got_fi[FI['have']].astype(np.uint64)
    assert ((masks >> haves) == 0).all()                 # no bit at or above have (>> 32 of a uint64: 0)
    for c in (0, 1, 31, 32):
        assert (mother[FI['have']] == c).any() and (mother[FI['target']] == c).any()
    assert len(set(got_keys.tolist())) == len(got_keys)
    assert got_keys[n_keep:].tolist() == list(range(key_base, key_base + 2 * len(moth)))


@pytest.mark.parametrize('divides', [True, False])
def test_divide_flagella_of_one_agent(dev, divides):
    flag_int = np.array([[7], [6], [0b101101]], dtype=np.int32)
    keys, lineage = np.array([12], dtype=np.int64), (np.array([0], dtype=np.int32), np.array([2], dtype=np.int32),
                                                    np.array([0b10], dtype=np.int64))
    for mode in ('merged', 'split_dict'):
        got_fi, got_keys, order, n_keep = _divide(dev, mode, flag_int, keys, lineage, np.array([divides]), 4, 5, 9, 100)
        want_fi, want_keys = ref.divide_flagella(flag_int, keys, order, n_keep, mode, 5, 9, lineage, 100)
        assert np.array_equal(got_fi, want_fi) and np.array_equal(got_keys, want_keys)
        if divides:
            assert got_keys.tolist() == [100, 101] and sorted(got_fi[FI['target']].tolist()) == [3, 4]
            if mode == 'split_dict':
                assert got_fi[FI['have']].tolist() == [3, 3] and got_fi[FI['mask']].tolist() == [0b101, 0b101]
        else:
            assert got_keys.tolist() == [12] and np.array_equal(got_fi, flag_int)


def test_divide_flagella_bad_arguments(dev):
    from lens_amd import native
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=dev)
    i64 = lambda *shape: torch.full(shape, -7, dtype=torch.int64, device=dev)
    src, kind, fi, key, root, depth, path = i32(8), i32(8), i32(3, 4), i64(4), i32(4), i32(4), i64(4)
    fi_dst, key_dst = i32(3, 8), i64(8)
    p = native.ptr
    good = [6, 2, 4, p(src), p(kind), p(fi), 4, p(key), p(root), p(depth), p(path), p(fi_dst), 8, p(key_dst), 0, 1, 1, 10]
    for index, value in ((0, -1), (1, 7), (1, -1), (2, 5), (6, 3), (12, 5), (14, 2), (14, -1), (17, -1),
                         (17, 2 ** 31 - 3), (3, 0), (4, 0), (7, 0), (13, 0), (5, 0), (11, 0), (8, 0), (9, 0), (10, 0)):
        args = list(good)
        args[index] = value
        assert native._lib.vk_divide_flagella(*args, _stream()) == native.VK_ERR_ARG, (index, value)
    torch.cuda.synchronize()
    assert (fi_dst == -7).all() and (key_dst == -7).all()


# -- the colony ------------------------------------------------------------------------------

def _plane():
    x = np.linspace(0.0, 1.0, ref.CASE_BINS[0])
    return 0.2 * x[:, None] + 0.05 * x[None, :] ** 2


def _colony(dev, mode, capacity=128, cells=True, expression=True, growth_rate=None, flagella=True):
    from lens_amd import configs
    from lens_amd.colony import Colony
    from lens_amd.lattice import Lattice
    model, cm, n, loc, bounds = ref.colony_case(mode, expression=expression, flagella=flagella)
    if growth_rate is not None:
        cm.growth_rate = growth_rate
    start = {'glc__D_e': configs.gaussian_bump_field(ref.CASE_BINS), 'lcts_e': np.full(ref.CASE_BINS, 10.0),
             'MeAsp': _plane()}
    lat = Lattice(['glc__D_e', 'lcts_e', 'MeAsp'], ref.CASE_BINS, bounds, 10.0, 5.0, device=dev, initial=start)
    col = Colony(configs.glc_lct_config(), n, capacity=capacity, device=dev, integrator='dopri5', environment=lat,
                 cells=cm if cells else None, motility=model)
    col.set_agents(location=loc)
    col.gather_external()
    return col


def _field(col):
    return col.lattice.owned('MeAsp').cpu().numpy().copy()


def _host(col):
    n = col.n
    out = {name: getattr(col, name)[..., :n].cpu().numpy() for name in ('motil', 'flag', 'flag_int', 'location',
                                                                        'bin_lin', 'm2c')}
    for name in ('flag_expr', 'cell', 'motile_key'):
        if getattr(col, name, None) is not None:
            out[name] = getattr(col, name)[..., :n].cpu().numpy()
    return out


def _compare(col, c, where, worst):
    """The device colony against the restatement ``c`` after the same step."""
    got = _host(col)
    R, F = fref.R, fref.F
    assert col.n == c.n and col.agent_ids() == c.ids, where
    assert np.array_equal(got['motile_key'], c.keys), where
    assert np.array_equal(got['flag_int'], c.flag_int), where                      # target, have, mask
    assert np.array_equal(got['bin_lin'], c.bins), where
    assert got['flag_expr'].tobytes() == c.expr.tobytes(), where                   # bitwise
    for name in ('motile_state', 'PMF'):
        assert np.array_equal(got['flag'][F[name]], c.flag[F[name]]), (where, name)
    for name in ('motor_state', 'thrust', 'CheY_P', 'ccw_motor_bias', 'ccw_to_cw'):
        assert np.array_equal(got['motil'][R[name]], c.motil[R[name]]), (where, name)
    assert np.array_equal(got['cell'][5], got['motil'][R['angle']]), where         # one heading, bitwise
    rel = lambda g, w: float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300)))
    dev_abs = lambda g, w: float(np.max(np.abs(g - w)))
    figures = {'n_methyl': rel(got['motil'][R['n_methyl']], c.motil[R['n_methyl']]),
               'chemoreceptor_activity': rel(got['motil'][R['chemoreceptor_activity']],
                                             c.motil[R['chemoreceptor_activity']]),
               'm2c': rel(got['m2c'], c.m2c)}
    for name in ('angle', 'torque'):
        figures[name] = dev_abs(got['motil'][R[name]], c.motil[R[name]])
    for name in ('CheY', 'CheY_P', 'cw_bias'):
        figures[name] = dev_abs(got['flag'][F[name]], c.flag[F[name]])
    figures['location'] = max(dev_abs(got['location'][k], c.loc[k]) / c.bounds[k] for k in (0, 1))
    for row, name in enumerate(('mass', 'volume', 'length', 'surface_area', 'protein')):
        figures[name] = rel(got['cell'][row], c.cell[name])
    for name, v in figures.items():
        worst[name] = max(worst.get(name, 0.0), v)
        assert v <= BOUND, (where, name, v)


@pytest.fixture(scope='module')
def trajectories(dev):
    """Both modes' device colonies after STEPS steps, each compared with its restatement
    at every step; what the later tests need of the way there."""
    out = {}
    for mode in ('merged', 'split_dict'):
        col = _colony(dev, mode)
        c = ref.MotileColony(*ref.colony_case(mode))
        assert np.array_equal(col.flag_int[:, :col.n].cpu().numpy(), c.flag_int)   # the derivers ran once at t = 0
        margins, worst, targets, events = {}, {}, set(), []
        for step in range(STEPS):
            field = _field(col)
            mothers = c.step(field, 1.0, margins)
            assert all(v >= 1e-9 for v in margins.values()), (step, margins)       # nobody is left out
            col.step(1.0)
            torch.cuda.synchronize()
            _compare(col, c, (mode, step), worst)
            if not events:
                targets |= set(c.flag_int[FI['target']].tolist())
            if mothers:
                events.append((step, mothers))
        col.check_status()
        print(mode, 'margins', margins, 'largest deviations', worst, 'divisions', events)
        out[mode] = (col, c, margins, targets, events)
    return out


@pytest.mark.parametrize('mode', ['merged', 'split_dict'])
def test_colony_equals_the_restatement(trajectories, mode):
    col, c, margins, targets, events = trajectories[mode]
    assert set(margins) == {'switch', 'structural', 'edge', 'split'}
    assert set(range(9)) <= targets                      # the count passed 0..8 before the first division
    assert col.n >= 3 * ref.CASE_N and len(events) >= 2
    assert not c.flagged and int(col._flag_flags[0]) == 0
    assert int(col._motil_counter[0]) == STEPS * ref.CASE_SUBSTEPS and col.step_index == STEPS
    snap = col.snapshot()
    assert sorted(snap['flagella_expression']) == ['flag_RNA', 'flagella']
    assert np.array_equal(snap['motile_key'], c.keys) and len(set(snap['motile_key'].tolist())) == col.n
    assert np.array_equal(snap['flagella_expression']['flagella'], c.expr[1])
    names = col.agent_array_names()
    assert 'motile_key' in names and 'flag_expr' in names
    with pytest.raises(ValueError, match='derived'):
        col.set_flagella(3)
    with pytest.raises(ValueError, match='division'):
        col.capture(1.0, 1)


def _same(a, b, names, where):
    n = a.n
    assert a.n == b.n, where
    for m in a.lattice.molecules:
        assert torch.equal(a.lattice.owned(m), b.lattice.owned(m)), (where, m)
    for name in names:
        assert torch.equal(getattr(a, name)[..., :n], getattr(b, name)[..., :n]), (where, name)


def test_opting_in_changes_nothing_without_cells(dev):
    a, b = _colony(dev, 'merged', cells=False, expression=False), _colony(dev, None, cells=False, expression=False)
    for step in range(5):
        a.step(1.0)
        b.step(1.0)
    torch.cuda.synchronize()
    _same(a, b, ('motil', 'flag', 'flag_int', 'location', 'bin_lin', 'conc', 'counts'), 'division= without cells')
    assert a.agent_array_names() == b.agent_array_names() and not hasattr(a, 'motile_key')


def test_cells_that_do_not_divide_change_no_motile_row(dev):
    """Growth at the reference's rate: nobody divides in 5 steps.  The motor senses only the
    MeAsp plane, which no kinetics touches, and the agents' keys are their columns."""
    a = _colony(dev, 'merged', expression=False, growth_rate=0.000275)
    b = _colony(dev, None, cells=False, expression=False)
    for step in range(5):
        a.step(1.0)
        b.step(1.0)
    torch.cuda.synchronize()
    n = ref.CASE_N
    assert a.n == b.n == n
    for name in ('motil', 'flag', 'flag_int', 'location', 'bin_lin'):
        assert torch.equal(getattr(a, name)[..., :n], getattr(b, name)[..., :n]), name
    assert torch.equal(a.lattice.owned('MeAsp'), b.lattice.owned('MeAsp'))
    assert torch.equal(a.cell[5, :n], a.motil[fref.R['angle'], :n])
    assert torch.equal(a.motile_key[:n], torch.arange(n, device=dev))


def test_division_geometry_and_the_first_update_after_it(dev, trajectories):
    from lens_amd.motility import flagella_step
    first = trajectories['merged'][4][0][0]              # the step of the first division
    a, b = _colony(dev, 'merged'), _colony(dev, 'merged')
    for step in range(first):
        a.step(1.0)
        b.step(1.0)
    n = a.n
    assert n == ref.CASE_N
    expr_before = a.flag_expr[:, :n].clone()
    b._motility_step(1.0)                                # the mothers as the division finds them
    a.step(1.0)
    torch.cuda.synchronize()
    assert a.n == 2 * n                                  # the growth is all but synchronous: every agent divided
    R = fref.R
    d0, d1 = slice(0, 2 * n, 2), slice(1, 2 * n, 2)
    for name in ('motil', 'flag'):
        for d in (d0, d1):
            assert torch.equal(getattr(a, name)[:, d], getattr(b, name)[:, :n]), name
    assert torch.equal(a.flag_expr[:, d0], a.flag_expr[:, d1])
    assert not torch.equal(a.flag_expr[:, d0], expr_before)                        # the step's update, then copied
    mother, angle = b.location[:, :n], b.motil[R['angle'], :n]
    length = 2.0 * a.cell[2, d0]                         # the mother's length: split exactly
    assert torch.equal(a.cell[2, d0], a.cell[2, d1])
    for d, q in ((d0, -0.25), (d1, 0.25)):
        want = mother + torch.stack([length * q * torch.cos(angle), length * q * torch.sin(angle)])
        assert float((a.location[:, d] - want).abs().max()) <= 1e-12 * ref.CASE_BOUNDS[0]
    # 'merged': every flagellum of the mother, and the split count
    fi, mfi = a.flag_int[:, :2 * n].cpu().numpy(), b.flag_int[:, :n].cpu().numpy()
    target = a.flag_int[FI['target'], :2 * n].clone()
    assert np.array_equal(fi[FI['have'], d0], mfi[FI['have']]) and np.array_equal(fi[FI['mask'], d1], mfi[FI['mask']])
    assert (fi[FI['have']] > fi[FI['target']]).all()
    # one inner update: the surplus is shed
    flagella_step(a.motility, a.lattice, a.location, a.motil, a.flag, a.flag_int, a.n, 0.1, a._motil_counter,
                  key=a.motile_key, bin_lin=a.bin_lin, bin_ix=a.bin_ix, substeps=1)
    torch.cuda.synchronize()
    assert torch.equal(a.flag_int[FI['have'], :2 * n], target)
    masks = a.flag_int[FI['mask'], :2 * n].cpu().numpy().view(np.uint32).astype(np.uint64)
    assert ((masks >> target.cpu().numpy().astype(np.uint64)) == 0).all()


def test_capacity_growth(dev, trajectories):
    """capacity == n: division grows ld twice; every array, the occupancy buffers and the
    counter follow, and the result is the roomy colony's bit for bit."""
    roomy = trajectories['merged'][0]
    tight = _colony(dev, 'merged', capacity=ref.CASE_N)
    assert tight.ld == ref.CASE_N
    for step in range(STEPS):
        tight.step(1.0)
    torch.cuda.synchronize()
    assert tight.ld > ref.CASE_N and tight.ld != roomy.ld
    names = tight.agent_array_names()
    assert names == roomy.agent_array_names()
    _same(tight, roomy, names + ['bin_lin', 'bin_ix'], 'capacity growth')
    for name in names:
        assert getattr(tight, name).shape[-1] == tight.ld, name
    assert tight._occ_dev.order.numel() == tight.ld and tight._flag_expr_update.shape[1] == tight.ld
    assert int(tight._motil_counter[0]) == int(roomy._motil_counter[0]) == STEPS * ref.CASE_SUBSTEPS
    assert tight._key_base == roomy._key_base


def test_remove_keeps_keys_and_expression_rows(dev, trajectories):
    first = trajectories['split_dict'][4][0][0]
    a = _colony(dev, 'split_dict')
    for step in range(first + 1):
        a.step(1.0)
    n = a.n
    assert n == 2 * ref.CASE_N
    a.flag_expr[0, :n] += torch.arange(n, dtype=torch.float64, device=dev) * 1e-9        # a tag per agent
    mask = torch.zeros(n, dtype=torch.int32, device=dev)
    mask[::3] = 1
    keep = torch.nonzero(mask == 0).flatten()
    before = {name: getattr(a, name)[..., keep].clone() for name in ('motile_key', 'flag_expr', 'flag_int', 'motil')}
    ids = [a.agent_ids()[k] for k in keep.tolist()]
    removed = a.remove(mask)
    assert removed == (n + 2) // 3 and a.n == n - removed and a.agent_ids() == ids
    for name, want in before.items():
        assert torch.equal(getattr(a, name)[..., :a.n], want), name
        assert getattr(a, name).shape[-1] == a.ld
    assert a.motile_key.dtype == torch.int64
    key_base = a._key_base
    a.step(1.0)                                          # and the colony steps on
    torch.cuda.synchronize()
    a.check_status()
    assert torch.equal(a.motile_key[:a.n], before['motile_key']) and a._key_base == key_base
    # a key that would pass 2**31 - 1 is refused when the next division comes
    a._key_base = 2 ** 31 - 1
    with pytest.raises(OverflowError):
        for step in range(20):
            a.step(1.0)


def test_coarse_motor_divides_and_both_modes_agree(dev):
    """The coarse motor has no flagella: vk_divide_flagella hands out keys only, and the two
    modes are one.  Against the restatement (tests/motility_ref.py under the same loop)
    through the first division: ids, keys, motor state and bins exactly, the FP64 rows
    within the bound of tests/test_motility_gpu.py (1e-12 relative)."""
    a, b = _colony(dev, 'merged', flagella=False), _colony(dev, 'split_dict', flagella=False)
    c = ref.MotileColony(*ref.colony_case('merged', flagella=False))
    assert not hasattr(a, 'flag_int') and 'motile_key' in a.agent_array_names()
    margins, R, worst = {}, fref.R, 0.0
    for step in range(16):
        c.step(_field(a), 1.0, margins)
        assert all(v >= 1e-9 for v in margins.values()), (step, margins)
        a.step(1.0)
        b.step(1.0)
        torch.cuda.synchronize()
        _same(a, b, a.agent_array_names() + ['bin_lin'], ('modes', step))
        n = a.n
        motil, loc = a.motil[:, :n].cpu().numpy(), a.location[:, :n].cpu().numpy()
        assert n == c.n and a.agent_ids() == c.ids and np.array_equal(a.motile_key[:n].cpu().numpy(), c.keys), step
        assert np.array_equal(a.bin_lin[:n].cpu().numpy(), c.bins), step
        for name in ('motor_state', 'thrust'):
            assert np.array_equal(motil[R[name]], c.motil[R[name]]), (step, name)
        assert torch.equal(a.cell[5, :n], a.motil[R['angle'], :n])
        dev_rel = float(np.max(np.abs(motil - c.motil) / np.maximum(np.abs(c.motil), 1.0)))
        dev_loc = float(np.max(np.abs(loc - c.loc)) / c.bounds[0])
        worst = max(worst, dev_rel, dev_loc)
        assert dev_rel <= BOUND and dev_loc <= BOUND, (step, dev_rel, dev_loc)
    print('coarse motor: margins', margins, 'largest deviation', worst)
    assert a.n == 2 * ref.CASE_N and a._key_base == 3 * ref.CASE_N
    assert sorted(a.motile_key[:a.n].tolist()) == list(range(ref.CASE_N, 3 * ref.CASE_N))


def test_graph_replay_without_cells(dev):
    a = _colony(dev, 'merged', cells=False)
    b = _colony(dev, 'merged', cells=False)
    replay = b.capture(1.0, 1)
    targets = []
    for step in range(5):
        a.step(1.0)
        replay()
        torch.cuda.synchronize()
        _same(a, b, ('motil', 'flag', 'flag_int', 'flag_expr', 'location', 'bin_lin', 'conc', 'counts'), step)
        targets.append(int(b.flag_int[FI['target'], 0]))
    assert targets == sorted(targets) and targets[-1] > targets[0], targets
    b.check_status()
    assert int(b._flag_flags[0]) == 0 and int(b._motil_counter[0]) == 5 * ref.CASE_SUBSTEPS
    with pytest.raises(ValueError, match='derived'):
        b.set_flagella(3)


def test_a_count_past_the_motor_raises(dev):
    """33 flagella and more: the kernel clamps, the colony raises where it reads anyway."""
    a = _colony(dev, 'merged', cells=False)
    a.flag_expr[1, :a.n] = 40.0 / float(a.m2c[0])
    a.step(1.0)
    assert int(a.flag_int[FI['target'], :a.n].max()) == 32
    with pytest.raises(FloatingPointError, match='flagella'):
        a.check_status()
