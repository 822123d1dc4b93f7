"""vk_cell_step_tree and the ``set`` divider of count rows on the device, bit for bit against
the restatement (tests/tree_mass_ref.py): cell rows, mmol_to_counts, divide, the protein row the
tree model must not touch, and the sentinel columns beyond n.

Sizes: n in {1, 63, 64, 65, 257} with ld = n + 7 and ld_counts = n + 3, n_weighted around the
load chunk of 16 and at both limits; the weighted rows lie sparse in a larger table (first row,
last row, gaps); counts of 0 and INT32_MAX and a weight of 0.0 are among them."""

import ctypes
import types

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import tree_mass_ref as tref
from lens_amd import native, population
from lens_amd.cells import CellModel, TreeWeights, cell_step_tree
from lens_amd.stochastic import MAX_SPECIES, StochasticModel, divide_agent_counts

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)
WEIGHTED = (0, 1, 15, 16, 17, 33, 256)
SEED = 20261021
INT32_MAX = 2 ** 31 - 1
VARIANTS = (('growth_protein', 'stream'), ('growth_protein', 'philox'), ('tree_mass', 'stream'))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    native.load()
    return torch.device('cuda', 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def _case(cm, n, W, salt=0):
    """Host arrays of one launch: sentinels (7 / -5) in every column >= n."""
    rng = np.random.default_rng([SEED, n, W, salt])
    ld, ldc = n + 7, n + 3
    n_rows = 300 if W == 256 else W + 9
    rows = np.sort(rng.choice(n_rows, size=W, replace=False)) if W else np.zeros(0, dtype=np.int64)
    if W >= 2:
        rows[0], rows[-1] = 0, n_rows - 1                       # the first row, the last row, gaps between
        assert np.all(np.diff(rows) > 0)
    weights = rng.uniform(1e3, 1e7, W)
    if W:
        weights[W // 2] = 0.0
    counts = rng.integers(0, 10 ** 6, (n_rows, ldc)).astype(np.int32)
    counts[rng.random((n_rows, ldc)) < 0.05] = 0
    counts[rng.random((n_rows, ldc)) < 0.05] = INT32_MAX
    counts[:, n:] = 7
    cell = np.full((native.VK_CELL_ROWS, ld), 7.0)
    p0 = cm.initial_protein()
    cell[native.VK_CELL_PROTEIN, :n] = np.floor(p0 * rng.uniform(0.8, 2.2, n))     # around divide_protein = 2 p0
    cell[native.VK_CELL_MASS, :n] = rng.uniform(1000.0, 3000.0, n)
    cell[native.VK_CELL_VOLUME, :n] = cm.division_volume * rng.uniform(0.5, 1.5, n)
    cell[native.VK_CELL_LENGTH, :n] = rng.uniform(1.0, 4.0, n)
    cell[native.VK_CELL_SURFACE_AREA, :n] = rng.uniform(3.0, 12.0, n)
    cell[native.VK_CELL_ANGLE, :n] = rng.uniform(0.0, 6.0, n)
    m2c = np.full(ld, 7.0)
    divide = np.full(ld, -5, dtype=np.int32)
    u = rng.random(ld)
    depth = rng.integers(0, 6, ld).astype(np.int32)
    path = (rng.integers(0, 64, ld) & ((1 << depth.astype(np.int64)) - 1)).astype(np.int64)
    root = rng.permutation(ld).astype(np.int32)
    initial_mass = rng.uniform(1000.0, 2000.0, ld)
    return dict(ld=ld, ldc=ldc, n_rows=n_rows, rows=rows, weights=weights, counts=counts, cell=cell, m2c=m2c,
                divide=divide, u=u, root=root, depth=depth, path=path, initial_mass=initial_mass)


def _launch(dev, cm, c, n, step=5, tree=None, raw=None):
    """The launch on device copies of ``c``; returns (status, cell, m2c, divide) as host arrays."""
    t = {k: torch.from_numpy(c[k]).to(dev) for k in ('counts', 'cell', 'm2c', 'divide', 'u', 'root', 'depth', 'path',
                                                     'initial_mass')}
    tree = TreeWeights(c['rows'], c['weights'], c['n_rows']).upload(dev) if tree is None else tree
    p = cm.vk_params(1.0, step)
    if raw is not None:
        rc = raw(p, t, tree)
    else:
        rc = cell_step_tree(p, n, c['ld'], t['cell'], t['m2c'], t['u'] if cm.rng == 'stream' else None,
                            t['root'], t['depth'], t['path'], t['divide'], t['counts'], tree,
                            t['initial_mass'] if cm.model == 'tree_mass' else None)
    torch.cuda.synchronize()
    return rc, t['cell'].cpu().numpy(), t['m2c'].cpu().numpy(), t['divide'].cpu().numpy()


def _expected(cm, c, n, step=5):
    cell, m2c = c['cell'].copy(), c['m2c'].copy()
    divide = c['divide'].copy()
    divide[:n] = tref.cell_step(cm, 1.0, step, n, cell, m2c, c['counts'], c['rows'], c['weights'], u=c['u'],
                                lineage=(c['root'], c['depth'], c['path']), initial_mass=c['initial_mass'])
    return cell, m2c, divide


def _model(model, rng):
    return CellModel(model=model, rng=rng, seed=99, growth_rate=0.05, division_volume=1.7,
                     molecular_weights={'x': 1.0})               # the launches bind their own rows


@pytest.mark.parametrize('W', WEIGHTED)
@pytest.mark.parametrize('n', SIZES)
def test_step_equals_the_restatement(dev, n, W):
    for k, (model, rng) in enumerate(VARIANTS):
        cm = _model(model, rng)
        c = _case(cm, n, W, k)
        rc, cell, m2c, divide = _launch(dev, cm, c, n)
        assert rc == native.VK_OK
        want_cell, want_m2c, want_divide = _expected(cm, c, n)
        where = (model, rng, n, W)
        assert np.array_equal(_bits(cell), _bits(want_cell)), where       # the sentinel columns too
        assert np.array_equal(_bits(m2c), _bits(want_m2c)), where
        assert np.array_equal(divide, want_divide), where
        assert set(divide[:n].tolist()) <= {0, 1} and np.all(divide[n:] == -5)
        if model == 'tree_mass':
            assert np.array_equal(_bits(cell[native.VK_CELL_PROTEIN]), _bits(c['cell'][native.VK_CELL_PROTEIN])), where
        elif W:
            assert not np.array_equal(cell[native.VK_CELL_MASS, :n], c['cell'][native.VK_CELL_MASS, :n])
    if n >= 63:
        assert 0 < divide[:n].sum() < n                          # both sides of the threshold occur


@pytest.mark.parametrize('rng', ['stream', 'philox'])
@pytest.mark.parametrize('n', SIZES)
def test_no_weighted_rows_is_vk_cell_step(dev, n, rng):
    cm = _model('growth_protein', rng)
    c = _case(cm, n, 0)
    rc, cell, m2c, divide = _launch(dev, cm, c, n)

    def plain(p, t, tree):
        return native._lib.vk_cell_step(ctypes.byref(p), n, c['ld'], native.ptr(t['cell']), native.ptr(t['m2c']),
                                        native.ptr(t['u']), native.ptr(t['root']), native.ptr(t['depth']),
                                        native.ptr(t['path']), native.ptr(t['divide']), native.stream_handle())
    rc2, cell2, m2c2, divide2 = _launch(dev, cm, c, n, raw=plain)
    assert rc == rc2 == native.VK_OK
    assert np.array_equal(_bits(cell), _bits(cell2)) and np.array_equal(_bits(m2c), _bits(m2c2))
    assert np.array_equal(divide, divide2) and not np.array_equal(cell[:, :n], c['cell'][:, :n])


def test_the_divide_flag_on_either_side_of_the_threshold(dev):
    cm = _model('tree_mass', 'stream')
    c = _case(cm, 3, 17)
    dv = cm.division_volume
    c['cell'][native.VK_CELL_VOLUME, :3] = [np.nextafter(dv, 0.0), dv, np.nextafter(dv, np.inf)]
    rc, cell, m2c, divide = _launch(dev, cm, c, 3)
    assert rc == native.VK_OK and divide[:3].tolist() == [0, 1, 1]
    want_cell, want_m2c, want_divide = _expected(cm, c, 3)
    assert np.array_equal(_bits(cell), _bits(want_cell)) and np.array_equal(divide, want_divide)


def test_vk_cell_step_still_refuses_the_tree_model(dev):
    cm = _model('tree_mass', 'stream')
    c = _case(cm, 5, 0)

    def plain(p, t, tree):
        return native._lib.vk_cell_step(ctypes.byref(p), 5, c['ld'], native.ptr(t['cell']), native.ptr(t['m2c']),
                                        native.ptr(t['u']), native.ptr(t['root']), native.ptr(t['depth']),
                                        native.ptr(t['path']), native.ptr(t['divide']), native.stream_handle())
    rc, cell, m2c, divide = _launch(dev, cm, c, 5, raw=plain)
    assert rc == native.VK_ERR_ARG and np.array_equal(_bits(cell), _bits(c['cell'])) and np.all(divide == -5)


BAD = ['growth model', 'unknown model', 'null cell', 'null m2c', 'null divide', 'null counts', 'null rows',
       'null weights', 'n_weighted < 0', 'n_weighted > 256', 'n_weighted > n_rows', 'ld < n', 'ld_counts < n',
       'tree without initial_mass', 'stream without u', 'philox without lineage', 'unknown rng', 'n < 0', 'null params']


@pytest.mark.parametrize('what', BAD)
def test_bad_arguments_launch_nothing(dev, what):
    n, W = 9, 4
    tree_model = what == 'tree without initial_mass'
    cm = _model('tree_mass' if tree_model else 'growth_protein', 'philox' if 'philox' in what else 'stream')
    c = _case(cm, n, W)

    def raw(p, t, tree):
        a = dict(p=ctypes.byref(p), n=n, ld=c['ld'], cell=native.ptr(t['cell']), m2c=native.ptr(t['m2c']),
                 u=native.ptr(t['u']), root=native.ptr(t['root']), depth=native.ptr(t['depth']),
                 path=native.ptr(t['path']), divide=native.ptr(t['divide']), counts=native.ptr(t['counts']),
                 ldc=c['ldc'], n_rows=c['n_rows'], rows=native.ptr(tree.dev_rows), weights=native.ptr(tree.dev_weights),
                 W=W, initial_mass=native.ptr(t['initial_mass']))
        if what == 'growth model':
            p.model = native.VK_GROWTH_MASS
        elif what == 'unknown model':
            p.model = 3
        elif what == 'unknown rng':
            p.rng = 7
        elif what.startswith('null '):
            a[{'params': 'p'}.get(what[5:], what[5:])] = None
        elif what == 'n_weighted < 0':
            a['W'] = -1
        elif what == 'n_weighted > 256':
            a['W'], a['n_rows'] = 257, 1000
        elif what == 'n_weighted > n_rows':
            a['n_rows'] = W - 1
        elif what == 'ld < n':
            a['ld'] = n - 1
        elif what == 'ld_counts < n':
            a['ldc'] = n - 1
        elif what == 'tree without initial_mass':
            a['initial_mass'] = None
        elif what == 'stream without u':
            a['u'] = None
        elif what == 'philox without lineage':
            a['depth'] = None
        elif what == 'n < 0':
            a['n'] = -1
        return native._lib.vk_cell_step_tree(a['p'], a['n'], a['ld'], a['cell'], a['m2c'], a['u'], a['root'], a['depth'],
                                             a['path'], a['divide'], a['counts'], a['ldc'], a['n_rows'], a['rows'],
                                             a['weights'], a['W'], a['initial_mass'], native.stream_handle())
    rc, cell, m2c, divide = _launch(dev, cm, c, n, raw=raw)
    assert rc == native.VK_ERR_ARG, what
    assert b'vk_cell_step_tree' in native._lib.vk_last_error()
    assert np.array_equal(_bits(cell), _bits(c['cell'])) and np.array_equal(_bits(m2c), _bits(c['m2c']))
    assert np.array_equal(divide, c['divide'])


@pytest.mark.parametrize('rows', [[0, 13], [-1, 2], [3, 3], [4, 2]])
def test_bad_rows_are_refused_on_the_host_side(dev, rows):
    """rows[] is validated where it is uploaded (the header says so): nothing reaches a launch."""
    with pytest.raises(ValueError, match='TreeWeights'):
        TreeWeights(rows, [1.0, 1.0], 13).upload(dev)
    cm = _model('tree_mass', 'stream')
    c = _case(cm, 4, 2)
    other = TreeWeights([0, 1], [1.0, 1.0], c['n_rows'] + 1).upload(dev)      # bound to another table
    with pytest.raises(ValueError, match='table the weights were bound to'):
        _launch(dev, cm, c, 4, tree=other)


# -- the set divider through divide_agent_counts ------------------------------------------------
N_DIV = 40
MOTHERS, REMOVED = (1, 7, 8, 20, 39), (0, 8, 15, 33)             # 8: a removed mother leaves no daughters


def _divide(dev, sm, x, keys, step=3, key_base=1000):
    col = types.SimpleNamespace(_ssa_key_base=key_base, stochastic=sm, step_index=step, _ssa_complex=lambda: None)
    divide, remove = np.zeros(N_DIV, dtype=np.int32), np.zeros(N_DIV, dtype=np.int32)
    divide[list(MOTHERS)], remove[list(REMOVED)] = 1, 1
    plan = population.plan_population(N_DIV, torch.from_numpy(divide).to(dev), torch.from_numpy(remove).to(dev), dev)
    ld_new = plan.n_out + 5
    old = {'ssa': torch.from_numpy(x).to(dev), 'ssa_key': torch.from_numpy(keys).to(dev)}
    new = {'ssa': torch.full((sm.n_rows, ld_new), -3, dtype=torch.int32, device=dev),
           'ssa_key': torch.full((ld_new,), -3, dtype=torch.int64, device=dev)}
    divide_agent_counts(col, plan, old, new, ld_new)
    torch.cuda.synchronize()
    return plan, new['ssa'].cpu().numpy(), new['ssa_key'].cpu().numpy()


@pytest.mark.parametrize('n_passive', [10, 2 * MAX_SPECIES + 5])          # one chunk, three chunks
def test_set_rows_keep_the_mothers_count(dev, n_passive):
    S = 3
    passive = ['p%d' % i for i in range(n_passive)]
    # in the active block, across the passive edge, a lone row, at a chunk edge, the last row
    named = ['A', 'AB', 'p0', 'p4', passive[-1]]
    if n_passive > MAX_SPECIES:
        named += ['p%d' % (MAX_SPECIES - 1), 'p%d' % MAX_SPECIES, 'p%d' % (MAX_SPECIES + 1)]
    args = (['A', 'B', 'AB'], {'bind': {'A': -1, 'B': -1, 'AB': 1}}, {'bind': 0.01})
    plain = StochasticModel(*args, passive=passive, seed=SEED)
    sm = StochasticModel(*args, passive=passive, seed=SEED, dividers={name: 'set' for name in named})
    set_rows = sorted(sm.index(name) for name in named)
    assert sum(hi - lo for lo, hi in sm.set_runs()) == len(set_rows) and len(sm.set_runs()) < len(set_rows)
    rng = np.random.default_rng([SEED, n_passive])
    x = rng.integers(0, 1000, (S + n_passive, N_DIV + 2)).astype(np.int32)
    x[:, MOTHERS[1]] = 1                                         # a mother of odd counts: the coin decides
    keys = rng.choice(2 ** 31, size=N_DIV + 2, replace=False).astype(np.int64)
    plan, got, got_keys = _divide(dev, sm, x, keys)
    plan2, want, want_keys = _divide(dev, plain, x, keys)
    n_out = plan.n_out
    assert (n_out, plan.n_daughters, plan.n_removed) == (N_DIV - 4 - 4 + 8, 8, 4) and plan2.n_out == n_out
    src, kind = plan.src[:n_out].cpu().numpy(), plan.kind[:n_out].cpu().numpy()
    assert np.array_equal(got_keys, want_keys) and np.all(got_keys[n_out:] == -3)
    others = [r for r in range(S + n_passive) if r not in set_rows]
    assert np.array_equal(got[others], want[others])              # no coin of any other row moved
    assert np.array_equal(got[set_rows, :n_out], x[np.ix_(set_rows, src)])      # survivors and both daughters
    assert np.all(got[:, n_out:] == -3)
    daughters = kind >= 0
    assert not np.array_equal(want[set_rows][:, :n_out][:, daughters],
                              x[np.ix_(set_rows, src[daughters])])             # the split differs
    # the split restated: every other row is divide_split's
    import ssa_ref as sref
    from lens_amd.stochastic import passive_seed
    active, rk = sref.divide_counts(x[:S, :N_DIV], keys[:N_DIV], src, kind, plan.n_keep, SEED, 3, 1000)
    parts = [active] + [sref.divide_counts(x[lo:lo + MAX_SPECIES, :N_DIV], keys[:N_DIV], src, kind, plan.n_keep,
                                           passive_seed(SEED, chunk), 3, 1000)[0]
                        for chunk, lo in enumerate(range(S, S + n_passive, MAX_SPECIES))]
    split = np.concatenate([p[:min(MAX_SPECIES, len(p))] for p in parts])
    assert np.array_equal(want[:, :n_out], split) and np.array_equal(got_keys[:n_out], rk)
    assert np.array_equal(got[:, :n_out], tref.set_rows(split, x, src, set_rows))
