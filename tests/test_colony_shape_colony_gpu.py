"""Colony.colony_metrics(): the colonies of a growing, dividing colony with mechanics.

A 24-cell colony (glc_lct kinetics, CellModel 'growth', ContactModel) runs 30 steps through
divisions and through a growth of its capacity.  After every step colony_metrics() is checked
against the restatement (tests/colony_shape_ref.py) evaluated on the device's own state of that
step, with the tie condition (no |2 r + gap - d| < 1e-9) asserted on that state: it cannot be
pre-checked on the CPU, so a failure of that assertion means another seed, never a skip.  A
twin colony that never calls colony_metrics() must keep every array bit-identical.
"""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import colony_shape_ref as ref
from lens_amd import configs, native
from lens_amd.rate_law_compiler import compile_rate_laws

pytestmark = pytest.mark.gpu

NX, BOUND = 64, 128.0
N_CELLS, CAPACITY, STEPS = 24, 40, 30
TIE = 1e-9


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _lattice(dev):
    from lens_amd.lattice import Lattice
    start = {'glc__D_e': configs.gaussian_bump_field((NX, NX)), 'lcts_e': np.full((NX, NX), 10.0)}
    return Lattice(['glc__D_e', 'lcts_e'], (NX, NX), (BOUND, BOUND), 10.0, 5.0, device=dev, initial=start)


def _colony(dev, n, *, mechanics, cells=None, capacity=None, loc=None, seed=23):
    from lens_amd.colony import Colony
    cfg = configs.glc_lct_config()
    t = compile_rate_laws(cfg['reactions'], cfg['kinetic_parameters'])
    rng = np.random.default_rng(seed)
    params, conc = configs.heterogeneous_colony(t, cfg, n)
    if loc is None:
        loc = 64.0 - 6.0 + rng.uniform(0.0, 12.0, (2, n))
    col = Colony(cfg, n, capacity=capacity, device=dev, integrator='dopri5', environment=_lattice(dev), table=t,
                 cells=cells, mechanics=mechanics)
    col.set_agents(params=params, conc=conc, location=loc)
    if cells is not None:
        # division at 2640 fg; 2 % a step: everybody divides within the 30 steps
        col.set_cell_mass(rng.uniform(1500.0, 2600.0, n))
        col.cell[native.VK_CELL_ANGLE, :n] = torch.from_numpy(rng.uniform(0.0, 2.0 * np.pi, n)).to(dev)
    col.gather_external()
    return col


def _growing(dev):
    from lens_amd.cells import CellModel
    from lens_amd.mechanics import ContactModel
    return _colony(dev, N_CELLS, mechanics=ContactModel(seed=11, jitter=0.01, jitter_angle=0.02),
                   cells=CellModel(model='growth', growth_rate=0.02), capacity=CAPACITY)


def _restate(col, link_gap, min_cells):
    n = col.n
    loc = col.location[:, :n].cpu().numpy()
    if col.cells is not None:
        th = col.cell[native.VK_CELL_ANGLE, :n].cpu().numpy()
        L = col.cell[native.VK_CELL_LENGTH, :n].cpu().numpy()
        mass = col.cell[native.VK_CELL_MASS, :n].cpu().numpy()
    else:
        th = col.mech_angle[:n].cpu().numpy()
        L, mass = np.full(n, col.mechanics.length), np.full(n, col.mass_fg)
    keys = np.arange(n, dtype=np.int64) if col.agent_order is None else col.agent_order[:n].cpu().numpy()
    return ref.analyse(loc[0], loc[1], th, L, keys, col.lattice.bounds, width=col.mechanics.width, gap=link_gap,
                       min_cells=min_cells, max_length=col.mechanics.max_length, mass=mass)


def _check(got, want):
    """Labels, cells and keys exactly; every per-colony value within colony_shape_ref.bounds:
    sums 1e-12 relative, moments 1e-12 of the sum of |terms|, and -- for the colonies the
    restatement finds conditioned (anisotropy >= 0.05, radius <= 64 um, off the cut) -- the
    angle within |dS| / (lambda_1 - lambda_2) and the axes within radius * dphi.  Returns how
    many colonies had their angle and axes compared."""
    assert want['tie'] >= TIE, want['tie']
    assert got.n_colonies == want['n_colonies']
    assert np.array_equal(got.colony, want['colony'])
    assert np.array_equal(got.cells, want['cells']) and np.array_equal(got.key, want['key'])
    tol = ref.bounds(want)
    for name, have in (('mass', got.mass), ('cell_area', got.cell_area), ('cx', got.centroid[:, 0]),
                       ('cy', got.centroid[:, 1])):
        assert (np.abs(have - want[name]) <= tol['sum'] * np.abs(want[name])).all(), name
    for i, (name, r) in enumerate((('sxx', native.VK_COLONY_SXX), ('syy', native.VK_COLONY_SYY),
                                   ('sxy', native.VK_COLONY_SXY))):
        assert (np.abs(got.rows[r] - want[name]) <= tol['moments'][:, i]).all(), name
    ok = tol['conditioned']
    assert (np.abs(got.angle - want['angle'])[ok] <= tol['angle'][ok]).all()
    assert (np.abs(got.major_axis - want['major'])[ok] <= tol['extent'][ok]).all()
    assert (np.abs(got.minor_axis - want['minor'])[ok] <= tol['extent'][ok]).all()
    return int(ok.sum())


def test_metrics_follow_a_growing_colony_and_change_nothing(dev):
    a, b = _growing(dev), _growing(dev)
    ns, lds, counts, compared = [a.n], [a.ld], [], 0
    for step in range(STEPS):
        a.step(1.0)
        b.step(1.0)
        got = a.colony_metrics(link_gap=0.25, min_cells=3)
        assert a._colony_shape.ld == a.ld                     # made again after the capacity grew
        compared += _check(got, _restate(a, 0.25, 3))
        ns.append(a.n)
        lds.append(a.ld)
        counts.append(got.n_colonies)
    a.check_status()
    print('n per step', ns, 'ld', sorted(set(lds)), 'colonies', counts, 'angle and axes compared', compared)
    assert compared >= 1
    assert ns[-1] >= 2 * N_CELLS - 4 and lds[0] == CAPACITY and lds[-1] > CAPACITY
    assert max(counts) >= 1
    # every array the colony had before is what a colony that never asked has
    assert a.n == b.n and a.agent_array_names() == b.agent_array_names()
    for name in a.agent_array_names() + ['bin_lin', 'bin_ix']:
        assert torch.equal(getattr(a, name)[..., :a.n], getattr(b, name)[..., :b.n]), name
    for m in a.lattice.molecules:
        assert torch.equal(a.lattice.owned(m), b.lattice.owned(m)), m
    assert int(a._mech.counter[0]) == int(b._mech.counter[0])
    assert b._colony_shape is None


def _two_rows(gap_between):
    """Two rows of five capsules (L = 2, along x, 1.5 um apart), ``gap_between`` um between the rows' axes."""
    xs = 60.0 + 1.5 * np.arange(5)
    return np.stack([np.concatenate([xs, xs]), np.concatenate([np.full(5, 60.0), np.full(5, 60.0 + gap_between)])])


def test_two_colonies_then_one(dev):
    from lens_amd.mechanics import ContactModel
    model = ContactModel(angles=np.zeros(10), length=2.0)
    col = _colony(dev, 10, mechanics=model, loc=_two_rows(8.0))
    got = col.colony_metrics()                                # link_gap 0.5, min_cells 3
    want = _restate(col, 0.5, 3)
    assert want['tie'] >= 0.25 and want['n_colonies'] == 2
    _check(got, want)
    assert list(got.cells) == [5, 5] and list(got.key) == [0, 5]
    assert list(got.mass) == [5 * col.mass_fg] * 2
    assert got.major_axis == pytest.approx([8.0, 8.0], abs=1e-12) and got.minor_axis == pytest.approx([1.0, 1.0], abs=1e-12)
    g = got.as_colony_global()
    assert sorted(g) == ['major_axis', 'mass', 'minor_axis', 'surface_area'] and len(g['mass']) == 2
    # other parameters: new buffers, the same answer from the same state (margins 0.5 at gap 0)
    assert col.colony_metrics(link_gap=0.0, min_cells=6).n_colonies == 0
    assert col.colony_metrics(link_gap=0.0, min_cells=5).n_colonies == 2
    # the same cells moved together: rows 1 um apart are linked (margin 0.5; diagonal neighbours 0.38)
    col.set_agents(location=_two_rows(1.0))
    got = col.colony_metrics()
    want = _restate(col, 0.5, 3)
    assert want['tie'] >= 0.25 and want['n_colonies'] == 1
    _check(got, want)
    assert list(got.cells) == [10] and list(got.mass) == [10 * col.mass_fg]
    assert got.minor_axis == pytest.approx([2.0], abs=1e-12) and got.major_axis == pytest.approx([8.0], abs=1e-12)


def test_capacity_hook_drops_the_buffers_between_two_calls(dev):
    from lens_amd.mechanics import ContactModel
    model = ContactModel(angles=np.zeros(10), length=2.0)
    col = _colony(dev, 10, mechanics=model, loc=_two_rows(8.0), capacity=10)
    first = col.colony_metrics()
    shape = col._colony_shape
    assert shape is not None and shape.ld == 10
    col._capacity_scratch()                                   # what every capacity change goes through
    assert col._colony_shape is None
    again = col.colony_metrics()
    assert col._colony_shape is not shape
    assert np.array_equal(first.colony, again.colony) and first.rows.tobytes() == again.rows.tobytes()


def test_needs_mechanics(dev):
    from lens_amd.colony import Colony
    cfg = configs.glc_lct_config()
    t = compile_rate_laws(cfg['reactions'], cfg['kinetic_parameters'])
    col = Colony(cfg, 4, device=dev, environment=_lattice(dev), table=t)
    with pytest.raises(ValueError):
        col.colony_metrics()
