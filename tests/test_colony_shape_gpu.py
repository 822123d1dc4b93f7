"""vk_colony_metrics on the device against the restatement (tests/colony_shape_ref.py).

Labels.  ``colony`` per agent, the colony count, ``cells`` and ``colony_key`` must equal the
restatement's exactly: the same partition in the same numbering.  A link decision can be
required to agree only when it is not a tie within rounding (device cos and sin stay within
an ulp of libm), so every case asserts on the restatement's values that no ordered pair has
|2 r + gap - d| < 1e-9 (TIE); no pair is left out.  The seeds were picked and recorded on
the CPU (smallest margins: 2.8e-4 at n = 1000 up to 0.7 at n = 2); the hand-built cases sit on their branch with
margins of 0.25 or more.

Metrics.  The restatement's sums are math.fsum.  A sum of n terms in any order is within
(n - 1) 2^-53 of the exact one relative to the sum of |terms|: below 1.2e-13 at n <= 1000,
asserted as SUM_TOL = 1e-12 (colony_shape_ref.bounds, from the restatement's values alone).
  mass, cell_area, cx, cy: sums of positive terms, so 1e-12 relative.
  sxx, syy, sxy: 1e-12 of the sum of |terms|.
  angle: phi = atan2(2 sxy, sxx - syy) / 2 moves by at most
      (d sxy + (d sxx + d syy) / 2) / hypot(2 sxy, sxx - syy) <= |dS| / (lambda_1 - lambda_2),
      |dS| the sum of the three bounds above.
  major, minor: d extent <= radius * dphi, radius the farthest capsule end from the centroid.
Angle and axes are compared only on conditioned inputs, asserted on the restatement: every
colony has anisotropy (lambda_1 - lambda_2) / lambda_1 >= 0.05, radius <= 64 um and
|phi| < pi / 2 - 1e-3 (phi jumps by pi across the cut at +-pi / 2).  The straight chain of 513
cells is 257 um from end to centre, so only its sums and moments are compared.  No tolerance
comes from the device's results.
"""

import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import colony_shape_ref as ref

pytestmark = pytest.mark.gpu

BOUNDS = (41.5, 37.0)         # gx = 9, gy = 8 at gap 0.5, (9, 8) at 0.25: a swapped axis shows
GAP = 0.25
TIE = 1e-9
# n -> (seed, patch_x, patch_y): uniform capsules (w = 1, L in [1, 4]) on the patch; picked on the CPU
RANDOM = {1: (1, 30.0, 30.0), 2: (2, 3.0, 3.0), 3: (3, 4.0, 4.0), 63: (63, 14.0, 12.0), 64: (64, 14.0, 12.0),
          65: (65, 14.0, 12.0), 257: (257, 30.0, 27.0), 1000: (1000, 41.5, 37.0)}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lens_amd import native
    native.load()
    return torch.device('cuda', torch.cuda.current_device())


def random_case(n):
    seed, px, py = RANDOM[n]
    rng = np.random.default_rng(seed)
    return dict(x=rng.uniform(0.0, px, n), y=rng.uniform(0.0, py, n), th=rng.uniform(0.0, 2 * math.pi, n),
                L=rng.uniform(1.0, 4.0, n), keys=rng.permutation(5 * n + 11)[:n].astype(np.int64),
                mass=rng.uniform(500.0, 2000.0, n))


def circles(points, keys=None, seed=0):
    """Unit circles (w = L = 1) at ``points``, stored in a shuffled order under shuffled keys."""
    pts = np.array(points, dtype=np.float64).reshape(-1, 2)
    n = pts.shape[0]
    rng = np.random.default_rng(seed)
    pts = pts[rng.permutation(n)]
    keys = rng.permutation(3 * n + 5)[:n].astype(np.int64) if keys is None else keys
    return dict(x=pts[:, 0].copy(), y=pts[:, 1].copy(), th=np.zeros(n), L=np.ones(n), keys=keys, mass=None)


_REF = {}


def restate(tag, case, bounds, gap, min_cells):
    """The restatement of a case, computed once per (tag, min_cells) and never changed."""
    k = (tag, bounds, gap, min_cells)
    if k not in _REF:
        _REF[k] = ref.analyse(case['x'], case['y'], case['th'], case['L'], case['keys'], bounds, width=1.0, gap=gap,
                              min_cells=min_cells, max_length=4.0, mass=case['mass'], mass_const=1.0)
    return _REF[k]


def device_run(dev, case, bounds, gap, min_cells, metrics=True, perm=None):
    """One call: dict of numpy outputs.  ld = n + 7; ``perm`` permutes the columns."""
    from lens_amd import native
    from lens_amd.colonies import ColonyShape, ColonyShapeModel
    n = case['x'].shape[0]
    ld = n + 7
    perm = np.arange(n) if perm is None else perm

    def row(a, dtype=np.float64, fill=0):
        out = np.full(ld, fill, dtype=dtype)
        out[:n] = a[perm]
        return torch.from_numpy(out).to(dev)

    loc = torch.from_numpy(np.stack([np.concatenate([case['x'][perm], np.full(7, 1e300)]),
                                     np.concatenate([case['y'][perm], np.full(7, 1e300)])])).to(dev).contiguous()
    shape = ColonyShape(ColonyShapeModel(link_gap=gap, min_cells=min_cells, max_length=4.0, width=1.0), bounds, ld,
                        dev, length=2.0, mass=1.0, labels_only=not metrics)
    shape.colony.fill_(-7)
    shape.cells.fill_(-7)
    shape.colony_key.fill_(-7)
    shape.launch(n, loc, row(case['th']), length=row(case['L']), mass=None if case['mass'] is None else row(case['mass']),
                 key=row(case['keys'], np.int64))
    torch.cuda.synchronize()
    c = int(shape.n_colonies.item())
    colony = np.empty(n, dtype=np.int64)
    colony[perm] = shape.colony[:n].cpu().numpy()
    out = dict(colony=colony, n_colonies=c, cells=shape.cells.cpu().numpy(), key=shape.colony_key.cpu().numpy(),
               flags=int(shape.flags.item()), tail=shape.colony[n:].cpu().numpy(), shape=shape)
    if metrics:
        out['rows'] = shape.metrics.cpu().numpy()
    return out


def check_labels(got, want, n):
    assert want['tie'] >= TIE, want['tie']               # no link decision is a tie
    assert got['flags'] == 0
    c = want['n_colonies']
    assert got['n_colonies'] == c
    assert np.array_equal(got['colony'], want['colony'])
    assert np.array_equal(got['cells'][:c], want['cells']) and np.array_equal(got['key'][:c], want['key'])
    # nothing at or beyond the count, and no agent beyond n, is written
    assert (got['cells'][c:] == -7).all() and (got['key'][c:] == -7).all() and (got['tail'] == -7).all()


def check_metrics(got, want, axes=True):
    """Sums and moments always; angle and axes too (``axes``), on conditioned inputs only."""
    from lens_amd import native
    c = want['n_colonies']
    assert c >= 1
    tol = ref.bounds(want)
    if axes:
        assert tol['conditioned'].all()                  # anisotropy >= 0.05, radius <= 64, off the cut
    rows = got['rows'][:, :c]
    for name, r in (('mass', native.VK_COLONY_MASS), ('cell_area', native.VK_COLONY_CELL_AREA),
                    ('cx', native.VK_COLONY_CX), ('cy', native.VK_COLONY_CY)):
        err = np.abs(rows[r] - want[name])
        print(name, 'max relative error', float((err / np.abs(want[name])).max()))
        assert (err <= tol['sum'] * np.abs(want[name])).all(), name
    for i, (name, r) in enumerate((('sxx', native.VK_COLONY_SXX), ('syy', native.VK_COLONY_SYY),
                                   ('sxy', native.VK_COLONY_SXY))):
        err = np.abs(rows[r] - want[name])
        print(name, 'max error', float(err.max()), 'smallest bound', float(tol['moments'][:, i].min()))
        assert (err <= tol['moments'][:, i]).all(), name
    if not axes:
        return
    err = np.abs(rows[native.VK_COLONY_ANGLE] - want['angle'])
    print('angle max error / bound', float((err / tol['angle']).max()))
    assert (err <= tol['angle']).all()
    for name, r in (('major', native.VK_COLONY_MAJOR), ('minor', native.VK_COLONY_MINOR)):
        err = np.abs(rows[r] - want[name])
        print(name, 'max error / bound', float((err / tol['extent']).max()))
        assert (err <= tol['extent']).all(), name


# -- labels -------------------------------------------------------------------------------

@pytest.mark.parametrize('min_cells', [1, 3])
@pytest.mark.parametrize('n', sorted(RANDOM))
def test_labels_equal_the_restatement(dev, n, min_cells):
    case = random_case(n)
    want = restate(('random', n), case, BOUNDS, GAP, min_cells)
    check_labels(device_run(dev, case, BOUNDS, GAP, min_cells), want, n)
    if n == 1000:
        assert want['cells'].max() >= 900                # one giant component
    if n == 257:
        assert want['n_colonies'] >= 4                   # and many small ones


def component_sizes_case():
    """Rows of 1, 2, 3 and 4 unit circles spaced 1.0, the rows 6 um apart."""
    return circles([(3.0 + i, 3.0 + 6.0 * row) for row in range(4) for i in range(row + 1)], seed=11)


@pytest.mark.parametrize('min_cells, sizes', [(1, [1, 2, 3, 4]), (2, [2, 3, 4]), (3, [3, 4]), (4, [4])])
def test_components_of_exactly_min_cells_and_one_fewer(dev, min_cells, sizes):
    case = component_sizes_case()
    want = restate('sizes', case, BOUNDS, GAP, min_cells)
    assert want['tie'] >= 0.25 and sorted(want['cells']) == sizes
    check_labels(device_run(dev, case, BOUNDS, GAP, min_cells), want, 10)


CHAIN_BOUNDS = (520.0, 9.0)


def chain_case():
    """513 unit circles spaced 1.0 along x: long for the union, and its one colony crosses the
    256 and 512 member strides of the reductions."""
    c = circles([(0.5 + i, 4.0) for i in range(513)], seed=12)
    c['mass'] = np.random.default_rng(13).uniform(500.0, 2000.0, 513)
    return c


def diagonal_case():
    return circles([(1.0 + 0.7 * i, 1.0 + 0.7 * i) for i in range(46)], seed=14)


SHAPES = {
    'chain of 513': (chain_case, CHAIN_BOUNDS, 3, 1),
    'diagonal chain': (diagonal_case, BOUNDS, 3, 1),
    # three capsules on one centre under different angles, and two more circles on another
    'coincident centres': (lambda: dict(x=np.array([5.0, 5.0, 5.0, 20.0, 20.0]), y=np.array([6.0, 6.0, 6.0, 9.0, 9.0]),
                                        th=np.array([0.0, 1.0, 2.0, 0.0, 0.0]), L=np.array([2.0, 3.0, 2.5, 1.0, 1.0]),
                                        keys=np.array([9, 4, 7, 1, 30], dtype=np.int64), mass=None), BOUNDS, 2, 2),
    # exactly parallel spines (den = 0): three stacked 1.0 apart are linked, the pair 1.5 apart is not
    'parallel spines': (lambda: dict(x=np.array([10.0, 10.5, 10.0, 25.0, 25.0]), y=np.array([10.0, 11.0, 12.0, 20.0, 21.5]),
                                     th=np.zeros(5), L=np.full(5, 3.0), keys=np.array([5, 3, 8, 2, 6], dtype=np.int64),
                                     mass=None), BOUNDS, 2, 1),
    'all singletons': (lambda: circles([(3.0 + 6.0 * i, 3.0 + 6.0 * j) for i in range(6) for j in range(6)], seed=15),
                       BOUNDS, 3, 0),
    # not finite: in no colony although min_cells = 1 makes every other agent one
    'NaN and infinity': (lambda: dict(x=np.array([5.0, math.nan, 6.0, 7.0, math.inf, 30.0]),
                                      y=np.array([5.0, 5.0, 5.0, -math.inf, 5.0, 30.0]), th=np.zeros(6),
                                      L=np.ones(6), keys=np.arange(6, dtype=np.int64)[::-1].copy(), mass=None),
                         BOUNDS, 1, 2),
}


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_specific_shapes(dev, name):
    make, bounds, min_cells, n_colonies = SHAPES[name]
    case = make()
    want = restate(name, case, bounds, GAP, min_cells)
    assert want['tie'] >= 0.25 and want['n_colonies'] == n_colonies
    n = case['x'].shape[0]
    check_labels(device_run(dev, case, bounds, GAP, min_cells), want, n)
    if name == 'NaN and infinity':
        assert list(want['colony']) == [0, -1, 0, -1, -1, 1]
    if name == 'chain of 513':
        assert list(want['cells']) == [513]


def test_labels_only(dev):
    case = random_case(257)
    want = restate(('random', 257), case, BOUNDS, GAP, 3)
    got = device_run(dev, case, BOUNDS, GAP, 3, metrics=False)
    check_labels(got, want, 257)
    res = got['shape'].result()
    assert np.array_equal(res.cells, want['cells']) and np.isnan(res.mass).all()


def test_too_long_agent_sets_the_flag_and_the_call_returns(dev):
    from lens_amd import native
    case = circles([(5.0, 5.0), (6.0, 5.0), (7.0, 5.0), (20.0, 20.0)], seed=16)
    case['L'][int(np.argmax(case['x']))] = 4.25          # the lone one: longer than max_length = 4
    got = device_run(dev, case, BOUNDS, GAP, 3)
    assert got['flags'] == native.VK_COLONIES_TOO_LONG and got['n_colonies'] == 1
    with pytest.raises(ValueError):
        got['shape'].result()


# -- arguments ----------------------------------------------------------------------------

def test_argument_errors_launch_nothing(dev):
    from lens_amd import native
    from lens_amd.colonies import ColonyShape, ColonyShapeModel
    lib = native._lib
    n, ld = 5, 12
    shape = ColonyShape(ColonyShapeModel(link_gap=GAP), BOUNDS, ld, dev)
    loc = torch.full((2, ld), 3.0, dtype=torch.float64, device=dev)
    ang = torch.zeros(ld, dtype=torch.float64, device=dev)
    shape.n_colonies.fill_(7)

    def call(p=None, n=n, ld=ld, loc=loc.data_ptr(), bx=BOUNDS[0], by=BOUNDS[1], off=0, nbytes=None, flags=None,
             n_col=None, colony=None):
        p = shape.params if p is None else p
        return lib.vk_colony_metrics(
            ctypes.byref(p) if p else None, n, ld, loc, ang.data_ptr(), 0, 0, 0, bx, by,
            shape.colony.data_ptr() if colony is None else colony, shape.n_colonies.data_ptr() if n_col is None else n_col,
            shape.cells.data_ptr(), shape.colony_key.data_ptr(), shape.metrics.data_ptr(),
            shape.flags.data_ptr() if flags is None else flags, shape.scratch.data_ptr() + shape._off + off,
            shape._bytes if nbytes is None else nbytes, native.stream_handle())

    def params(**kw):
        p = ColonyShapeModel(link_gap=GAP).vk_params(BOUNDS)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    E = native.VK_ERR_ARG
    assert call(p=0) == E and call(n=-1) == E and call(ld=n - 1) == E and call(loc=0) == E
    assert call(bx=0.0) == E and call(by=math.nan) == E and call(flags=0) == E and call(n_col=0) == E
    assert call(colony=0) == E and call(off=8) == E and call(nbytes=shape._bytes // 2) == E
    assert call(p=params(min_cells=0)) == E and call(p=params(link_gap=-0.5)) == E
    assert call(p=params(link_gap=math.inf)) == E and call(p=params(width=5.0)) == E
    assert call(p=params(length=0.0)) == E               # no length array and no constant
    assert call(p=params(gx=10)) == E                    # 41.5 / 10 < 4.25: edges too short
    assert call(p=params(gx=0)) == E
    assert b'vk_colony_metrics' in lib.vk_last_error()
    torch.cuda.synchronize()
    assert int(shape.n_colonies.item()) == 7             # nothing ran
    assert call(n=0) == native.VK_OK
    torch.cuda.synchronize()
    assert int(shape.n_colonies.item()) == 0
    assert call() == native.VK_OK                        # the arguments the refusals varied
    torch.cuda.synchronize()
    assert int(shape.n_colonies.item()) == 1 and int(shape.cells[0].item()) == 5


# -- metrics ------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [257, 1000])
def test_metrics_of_random_capsules(dev, n):
    case = random_case(n)
    want = restate(('random', n), case, BOUNDS, GAP, 3)
    got = device_run(dev, case, BOUNDS, GAP, 3)
    check_labels(got, want, n)
    check_metrics(got, want)


@pytest.mark.parametrize('name', ['chain of 513', 'diagonal chain'])
def test_metrics_of_chains(dev, name):
    make, bounds, min_cells, _ = SHAPES[name]
    case = make()
    want = restate(name, case, bounds, GAP, min_cells)
    got = device_run(dev, case, bounds, GAP, min_cells)
    check_labels(got, want, case['x'].shape[0])
    # the chain of 513 is 257 um from end to centre, beyond the 64 um the axes' bound is stated
    # for: its sums and moments (they cross the 256 stride and the 512 split) only
    check_metrics(got, want, axes=name == 'diagonal chain')
    if name == 'diagonal chain':
        assert want['angle'][0] == pytest.approx(math.pi / 4, abs=1e-12)
        assert want['major'][0] == pytest.approx(45 * 0.7 * math.sqrt(2) + 1.0, abs=1e-9)
        assert want['minor'][0] == pytest.approx(1.0, abs=1e-9)


def test_constant_mass_and_length(dev):
    """mass == NULL and length == NULL: the constants of the parameters."""
    from lens_amd import native
    from lens_amd.colonies import ColonyShape, ColonyShapeModel
    pts = np.array([(5.0 + 1.5 * i, 7.0) for i in range(4)])
    n, ld = 4, 11
    loc = torch.zeros((2, ld), dtype=torch.float64, device=dev)
    loc[:, :n] = torch.from_numpy(pts.T.copy())
    shape = ColonyShape(ColonyShapeModel(link_gap=GAP), BOUNDS, ld, dev, length=2.0, mass=1339.0)
    shape.launch(n, loc, torch.zeros(ld, dtype=torch.float64, device=dev))
    res = shape.result()
    assert res.n_colonies == 1 and list(res.cells) == [4] and list(res.key) == [0] and list(res.colony) == [0] * 4
    assert res.mass[0] == 4 * 1339.0
    assert res.cell_area[0] == pytest.approx(4 * (1.0 + math.pi / 4), rel=1e-15)
    assert res.major_axis[0] == pytest.approx(4.5 + 2.0, abs=1e-12) and res.minor_axis[0] == pytest.approx(1.0, abs=1e-12)
    assert res.centroid.shape == (1, 2) and res.centroid[0, 0] == pytest.approx(7.25, rel=1e-15)
    g = res.as_colony_global()
    assert sorted(g) == ['major_axis', 'mass', 'minor_axis', 'surface_area'] and g['mass'] == [4 * 1339.0]
    assert g['surface_area'] == res.cell_area.tolist()


def test_launch_refuses_arrays_of_another_ld(dev):
    """The metrics rows have the buffers' stride: a location of another ld, or one that is
    not [2, ld], is refused before anything is launched."""
    from lens_amd.colonies import ColonyShape, ColonyShapeModel
    shape = ColonyShape(ColonyShapeModel(link_gap=GAP), BOUNDS, 12, dev)
    angle = torch.zeros(16, dtype=torch.float64, device=dev)
    shape.n_colonies.fill_(7)
    for ld in (11, 16):
        with pytest.raises(ValueError):
            shape.launch(5, torch.full((2, ld), 3.0, dtype=torch.float64, device=dev), angle)
    with pytest.raises(ValueError):
        shape.launch(5, torch.full((12,), 3.0, dtype=torch.float64, device=dev), angle)
    with pytest.raises(ValueError):
        shape.launch(5, torch.full((2, 12), 3.0, dtype=torch.float32, device=dev), angle)
    with pytest.raises(ValueError):
        shape.launch(13, torch.full((2, 12), 3.0, dtype=torch.float64, device=dev), angle)
    with pytest.raises(ValueError):
        shape.launch(5, torch.full((2, 12), 3.0, dtype=torch.float64, device=dev), angle[:4])
    torch.cuda.synchronize()
    assert int(shape.n_colonies.item()) == 7             # nothing ran
    shape.launch(5, torch.full((2, 12), 3.0, dtype=torch.float64, device=dev), angle)
    assert shape.result().n_colonies == 1


def test_the_flag_word_is_cleared_by_every_launch(dev):
    """A too-long agent fails the call it is in, not the calls after it."""
    from lens_amd.colonies import ColonyShape, ColonyShapeModel
    shape = ColonyShape(ColonyShapeModel(link_gap=GAP), BOUNDS, 12, dev)
    loc = torch.zeros((2, 12), dtype=torch.float64, device=dev)
    loc[0, :4] = torch.tensor([5.0, 6.0, 7.0, 20.0], dtype=torch.float64)
    loc[1, :4] = 5.0
    angle = torch.zeros(12, dtype=torch.float64, device=dev)
    length = torch.ones(12, dtype=torch.float64, device=dev)
    length[3] = 4.25
    shape.launch(4, loc, angle, length=length)
    with pytest.raises(ValueError):
        shape.result()
    length[3] = 1.0
    shape.launch(4, loc, angle, length=length)
    res = shape.result()
    assert res.n_colonies == 1 and list(res.cells) == [3]


# -- storage independence and capture -----------------------------------------------------------

@pytest.mark.parametrize('n', [257, 1000])
def test_storage_independence_is_bit_identical(dev, n):
    case = random_case(n)
    a = device_run(dev, case, BOUNDS, GAP, 3)
    b = device_run(dev, case, BOUNDS, GAP, 3, perm=np.random.default_rng(n + 1).permutation(n))
    c = a['n_colonies']
    assert c == b['n_colonies'] and np.array_equal(a['colony'], b['colony'])
    assert np.array_equal(a['cells'][:c], b['cells'][:c]) and np.array_equal(a['key'][:c], b['key'][:c])
    assert a['rows'][:, :c].tobytes() == b['rows'][:, :c].tobytes()


def test_captured_call_replays_on_moved_agents(dev):
    from lens_amd.colonies import ColonyShape, ColonyShapeModel
    first = random_case(257)
    n, ld = 257, 264
    model = ColonyShapeModel(link_gap=GAP)

    def rows(case, m):
        f = lambda a, dt=np.float64: np.concatenate([a, np.zeros(ld - m, dtype=dt)])
        return (torch.from_numpy(np.stack([f(case['x']), f(case['y'])])).to(dev), torch.from_numpy(f(case['th'])).to(dev),
                torch.from_numpy(f(case['L'])).to(dev), torch.from_numpy(f(case['mass'])).to(dev),
                torch.from_numpy(f(case['keys'], np.int64)).to(dev))

    moved = dict(first)
    rng = np.random.default_rng(99)
    moved['x'] = first['x'] + rng.uniform(-0.5, 0.5, n)
    moved['y'] = first['y'] + rng.uniform(-0.5, 0.5, n)
    want = ref.analyse(moved['x'], moved['y'], moved['th'], moved['L'], moved['keys'], BOUNDS, gap=GAP,
                       mass=moved['mass'])
    assert want['tie'] >= TIE
    loc, th, L, mass, keys = rows(first, n)
    shape = ColonyShape(model, BOUNDS, ld, dev)
    shape.launch(n, loc, th, length=L, mass=mass, key=keys)          # loads the kernels before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        shape.launch(n, loc, th, length=L, mass=mass, key=keys)
    loc2 = rows(moved, n)[0]
    loc.copy_(loc2)
    graph.replay()
    torch.cuda.synchronize()
    replayed = shape.result()
    fresh = ColonyShape(model, BOUNDS, ld, dev)
    fresh.launch(n, loc2, th, length=L, mass=mass, key=keys)
    expect = fresh.result()
    assert np.array_equal(replayed.colony, want['colony']) and replayed.n_colonies == want['n_colonies']
    assert np.array_equal(replayed.colony, expect.colony) and np.array_equal(replayed.cells, expect.cells)
    assert np.array_equal(replayed.key, expect.key) and replayed.rows.tobytes() == expect.rows.tobytes()
    first_labels = restate(('random', 257), first, BOUNDS, GAP, 3)['colony']
    assert not np.array_equal(first_labels, want['colony'])          # the move changed the partition
