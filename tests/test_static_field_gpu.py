"""vk_gradient_fill and vk_static_gather against the NumPy restatement
(tests/static_field_ref.py), and the lattice-side consumers against the fixture made from the
reference's own make_gradient (tests/golden/gradients.npz).

Tolerances.  Uniform and linear use only + - x / and sqrt, all correctly rounded and in the
same order on both sides under -ffp-contract=off: bitwise.  Gaussian and exponential add one
exp or pow whose argument is bitwise equal on both sides, so the difference is the two
libraries' function error alone.  The device library is built to OpenCL's full-profile bounds,
3 ulp for exp and 16 ulp for pow; the host's are within 1: at most 17 * 2.2e-16 = 3.8e-15
relative.  The bound is 1e-13.
"""

import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import static_field_ref as sref

pytestmark = pytest.mark.gpu

EXACT = ('uniform', 'linear')
TOL = 1e-13
CANARY = -7.0
WORST = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gradients.npz'))


def _agree(kind, got, want, where):
    if kind in EXACT:
        assert np.array_equal(got, want), (where, kind)
        return
    worst = float(np.max(np.abs(got - want) / np.abs(want)))
    WORST[kind] = max(WORST.get(kind, 0.0), worst)
    print('%s %s: worst relative difference %.3g (so far %.3g)' % (where, kind, worst, WORST[kind]))
    assert worst <= TOL, (where, kind, worst)


def _specs(gradient, bounds):
    from lens_amd.static_field import _spec_array, gradient_specs
    molecules, specs = gradient_specs(gradient, bounds)
    return molecules, specs, _spec_array(specs)


@pytest.mark.parametrize('kind', sref.TYPES)
@pytest.mark.parametrize('nx,ny', [(1, 1), (5, 7), (67, 129)])
def test_fill_through_padded_strides(dev, kind, nx, ny):
    """Two planes inside a canary buffer: a padded row stride, a padded plane stride, and
    slack in front of the first plane."""
    from lens_amd import native
    bounds = sref.GRID_BOUNDS
    molecules, specs, array = _specs(sref.GRID[kind], bounds)
    row_stride, front = ny + 5, 11
    plane_stride = nx * row_stride + 13
    buf = torch.full((front + 2 * plane_stride + 17,), CANARY, dtype=torch.float64, device=dev)
    native.check(native.load().vk_gradient_fill(array, 2, buf.data_ptr() + 8 * front, plane_stride, row_stride, nx, ny,
                                              float(bounds[0]), float(bounds[1]), native.stream_handle()), 'fill')
    got = buf.cpu().numpy()
    want = sref.make_gradient(sref.GRID[kind], (nx, ny), bounds)
    written = np.zeros(got.shape, dtype=bool)
    for f, m in enumerate(molecules):
        idx = front + f * plane_stride + np.arange(nx)[:, None] * row_stride + np.arange(ny)[None, :]
        written[idx] = True
        _agree(kind, got[idx], want[m], 'fill %dx%d' % (nx, ny))
    assert np.all(got[~written] == CANARY)


def test_fill_checks_its_arguments(dev):
    from lens_amd import native
    _, specs, array = _specs(sref.GRID['gaussian'], sref.GRID_BOUNDS)
    buf = torch.full((64,), CANARY, dtype=torch.float64, device=dev)
    fill = lambda arr, n, row_stride=7, ps=35: native.load().vk_gradient_fill(
        arr, n, native.ptr(buf), ps, row_stride, 5, 7, 10.0, 21.0, native.stream_handle())
    assert fill(array, native.VK_GRADIENT_MAX + 1) == native.VK_ERR_ARG
    assert fill(array, 1, row_stride=6) == native.VK_ERR_ARG
    assert fill(array, 2, ps=34) == native.VK_ERR_ARG              # planes would overlap
    bad = (native.VkGradientSpec * 1)(native.VkGradientSpec(native.VK_GRADIENT_GAUSSIAN, 0.0, 0.0, 0.0, 0.0))
    assert fill(bad, 1) == native.VK_ERR_ARG
    bad[0].type = 9
    assert fill(bad, 1) == native.VK_ERR_ARG
    bad[0].type, bad[0].p0 = native.VK_GRADIENT_EXPONENTIAL, -1.0
    assert fill(bad, 1) == native.VK_ERR_ARG
    assert fill(array, 0) == native.VK_OK
    assert bool((buf == CANARY).all())


def _many(n_mol, kind):
    """n_mol molecules of one type with distinct centres and parameters."""
    mols = {}
    for i in range(n_mol):
        c = [0.1 + 0.09 * i, 0.95 - 0.1 * i]
        mols['m%d' % i] = {'gaussian': {'center': c, 'deviation': 0.7 + 0.3 * i},
                           'linear': {'center': c, 'base': 0.1 * i, 'slope': 1.0 - 0.3 * i},
                           'exponential': {'center': c, 'base': 0.5 + 20.0 * i, 'scale': 1.0 + i}}[kind]
    return {'type': kind, 'molecules': mols}


@pytest.mark.parametrize('kind', sref.FIELD_TYPES)
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('n_mol', [1, 3, 8, 9])
def test_gather(dev, kind, n, n_mol):
    """conc rows in another order than the molecules, ld > n on both arrays; nine molecules
    make the wrapper launch twice."""
    from lens_amd.static_field import gradient_specs, static_gather
    bounds = sref.POINT_BOUNDS
    gradient = _many(n_mol, kind)
    molecules, specs = gradient_specs(gradient, bounds)
    rng = np.random.default_rng(20261020 + n)
    loc = np.stack([rng.uniform(0, bounds[0], n), rng.uniform(0, bounds[1], n)])
    ld, ld_conc, rows = n + 3, n + 6, n_mol + 4
    loc_d = torch.full((2, ld), CANARY, dtype=torch.float64, device=dev)
    loc_d[:, :n] = torch.from_numpy(loc).to(dev)
    conc = torch.full((rows, ld_conc), CANARY, dtype=torch.float64, device=dev)
    row_of = [(3 * f + 2) % rows for f in range(n_mol)]
    if len(set(row_of)) < n_mol:
        row_of = list(range(rows - 1, rows - 1 - n_mol, -1))
    static_gather(specs, list(zip(range(n_mol), row_of)), loc_d, n, conc)
    got = conc.cpu().numpy()
    want = sref.concentration(gradient, bounds, loc)
    for f, m in enumerate(molecules):
        _agree(kind, got[row_of[f], :n], want[m], 'gather n=%d' % n)
    assert np.all(got[:, n:] == CANARY)
    assert np.all(got[[r for r in range(rows) if r not in row_of]] == CANARY)


def test_gather_one_launch_takes_at_most_eight(dev):
    from lens_amd import native
    _, specs, array = _specs(_many(8, 'linear'), sref.POINT_BOUNDS)
    idx = (ctypes.c_int32 * 9)(*range(9))
    loc = torch.zeros((2, 4), dtype=torch.float64, device=dev)
    conc = torch.full((9, 4), CANARY, dtype=torch.float64, device=dev)
    call = lambda n_map, n=4: native.load().vk_static_gather(array, idx, idx, n_map, native.ptr(loc), 4, n,
                                                           native.ptr(conc), 4, native.stream_handle())
    assert call(9) == native.VK_ERR_ARG and call(8, n=5) == native.VK_ERR_ARG
    assert bool((conc == CANARY).all())
    assert call(8) == native.VK_OK and bool((conc[8] == CANARY).all()) and bool((conc[:8] != CANARY).all())


@pytest.mark.parametrize('kind', sref.TYPES)
def test_lattice_and_drop_in_start_from_the_gradient(dev, fixture, kind):
    """Lattice(gradient=) and BatchedDiffusionField({'gradient': ...}) against the reference's
    own 5 x 7 planes; the gradient overrides the initial state, as initial_state.update does."""
    from lens_amd.lattice import Lattice
    from lens_amd.process import BatchedDiffusionField
    want = fixture['grid_' + kind]
    initial = {'a': np.full(sref.GRID_BINS, 3.0), 'c': np.full(sref.GRID_BINS, 4.0)}
    lat = Lattice(['c', 'b', 'a'], sref.GRID_BINS, sref.GRID_BOUNDS, 10.0, 5.0, device=dev, initial=initial,
                  gradient=sref.GRID[kind])
    _agree(kind, lat.owned('a').cpu().numpy(), want[0], 'Lattice')
    _agree(kind, lat.owned('b').cpu().numpy(), want[1], 'Lattice')
    assert bool((lat.owned('c') == 4.0).all())
    with pytest.raises(ValueError, match='not one of the molecules'):
        Lattice(['a'], sref.GRID_BINS, sref.GRID_BOUNDS, 10.0, 5.0, device=dev, gradient=sref.GRID[kind])
    p = BatchedDiffusionField({'molecules': ['c', 'b', 'a'], 'n_bins': list(sref.GRID_BINS),
                               'bounds': list(sref.GRID_BOUNDS), 'initial_state': initial,
                               'gradient': sref.GRID[kind], 'device': dev})
    fields = p.ports_schema()['fields']
    plane = lambda m: fields[m]['_value'].tensor.cpu().numpy() if hasattr(fields[m]['_value'], 'tensor') \
        else np.asarray(torch.as_tensor(fields[m]['_value']).cpu())
    _agree(kind, plane('a'), want[0], 'BatchedDiffusionField')
    _agree(kind, plane('b'), want[1], 'BatchedDiffusionField')
    assert np.all(plane('c') == 4.0)
    assert initial['a'][0, 0] == 3.0                               # the caller's dict is not written


def test_drop_in_without_a_gradient_still_returns_ones(dev):
    from lens_amd.process import BatchedDiffusionField
    p = BatchedDiffusionField({'molecules': ['a'], 'n_bins': [5, 7], 'bounds': [10, 21], 'device': dev})
    v = p.ports_schema()['fields']['a']['_value']
    t = v.tensor if hasattr(v, 'tensor') else torch.as_tensor(v)
    assert tuple(t.shape) == (5, 7) and bool((t == 1.0).all())
    from lens_amd.lattice import Lattice
    assert bool((Lattice(['a'], (5, 7), (10, 21), 10.0, 5.0, device=dev, gradient={}).fields == 1.0).all())
