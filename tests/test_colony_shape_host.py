"""Colony metrics without a GPU: the model's refusals and grid sizes, the reference's seven
test scenarios on the restatement (tests/colony_shape_ref.py), and the restatement's own
invariance under a permutation of the agents.

The scenarios are the point sets of the reference's TestDeriveColonyShape
(vivarium/processes/derive_colony_shape.py:256-400), retyped as coordinate data, with every
cell a unit circle (w = L = 1) of mass 1 and link_gap = 0.25: neighbours at distance 1 are
linked (margin 0.25), those at sqrt(2) or 2 are not (margin -0.16 or less).  Under this
engine's definition they give the reference's colony counts and colony masses.
"""

import math

import numpy as np
import pytest

import colony_shape_ref as ref

PLUS = [(1, 2), (0, 1), (1, 1), (2, 1), (1, 0)]
COMB = ([(i, 4) for i in range(5)] + [(i, 3) for i in range(5)] + [(i, 2) for i in range(2)] +
        [(i, 1) for i in range(5)] + [(i, 0) for i in range(5)])
SCENARIOS = {
    'plus sign': (PLUS, [5.0]),
    'concave comb': (COMB, [22.0]),
    'outlier and NaN': ([(1, 2), (0, 1), (1, 1), (2, 1), (10, 1), (1, 0), (math.nan, math.nan)], [5.0]),
    'too diffuse': ([(1, 2), (0, 1), (2, 1), (1, 0)], []),
    'one cell': ([(1, 1)], []),
    'two cells': ([(0, 1), (2, 1)], []),
    'two plus signs': ([(1, 2), (11, 2), (0, 1), (1, 1), (2, 1), (10, 1), (11, 1), (12, 1), (1, 0), (11, 0)],
                       [5.0, 5.0]),
}
BOUNDS = (16.0, 8.0)


def scenario_arrays(points):
    x = np.array([p[0] for p in points], dtype=np.float64)
    y = np.array([p[1] for p in points], dtype=np.float64)
    n = x.shape[0]
    return x, y, np.zeros(n), np.ones(n), np.arange(n, dtype=np.int64)


def test_model_refusals():
    from lens_amd.colonies import ColonyShapeModel
    for bad in (dict(link_gap=-0.1), dict(link_gap=math.nan), dict(link_gap=math.inf), dict(min_cells=0),
                dict(min_cells=2.5), dict(width=2.0, max_length=1.5), dict(width=0.0)):
        with pytest.raises(ValueError):
            ColonyShapeModel(**bad)
    m = ColonyShapeModel()
    assert (m.link_gap, m.min_cells, m.max_length, m.width) == (0.5, 3, 4.0, 1.0)
    ColonyShapeModel(link_gap=0.0, min_cells=1, width=1.0, max_length=1.0)


def test_grid_sizes():
    from lens_amd.colonies import ColonyShapeModel
    m = ColonyShapeModel(link_gap=0.5, max_length=4.0)
    assert m.grid((41.5, 37.0)) == (9, 8)            # floor(41.5 / 4.5), floor(37 / 4.5)
    assert m.grid((4.4, 9.0)) == (1, 2)              # never fewer than one cell
    assert m.grid((4096.0, 4096.0)) == (910, 910)
    assert ColonyShapeModel(link_gap=0.25).grid((41.5, 37.0)) == ref.grid((41.5, 37.0), 4.0, 0.25)[:2] == (9, 8)
    for bounds in ((41.5, 37.0), (4096.0, 4096.0), (10.0, 100.0)):
        gx, gy = m.grid(bounds)
        for g, b in zip((gx, gy), bounds):
            assert g == 1 or b / g >= m.max_length + m.link_gap      # 3 x 3 cells suffice
    p = m.vk_params((41.5, 37.0), length=2.0, mass=1339.0)
    assert (p.gx, p.gy, p.min_cells, p.link_gap, p.max_length, p.width, p.length, p.mass) == (
        9, 8, 3, 0.5, 4.0, 1.0, 2.0, 1339.0)


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_reference_scenarios_give_the_reference_counts_and_masses(name):
    points, masses = SCENARIOS[name]
    x, y, th, L, keys = scenario_arrays(points)
    out = ref.analyse(x, y, th, L, keys, BOUNDS, width=1.0, gap=0.25, min_cells=3, max_length=4.0)
    assert out['tie'] >= 0.16 or len(points) < 2       # every decision far from a tie
    assert out['n_colonies'] == len(masses)
    assert list(out['mass']) == masses
    assert list(out['cells']) == [int(m) for m in masses]
    assert int((out['colony'] >= 0).sum()) == int(sum(masses))
    if name == 'outlier and NaN':
        assert out['colony'][4] == -1 and out['colony'][6] == -1
    if name == 'two plus signs':
        # numbered by first member in (cell, key) order: the left plus sign lies in lower cells
        assert [out['colony'][i] for i in (0, 1)] == [0, 1] and list(out['key']) == [0, 1]
        assert out['cx'] == pytest.approx([1.0, 11.0]) and out['cy'] == pytest.approx([1.0, 1.0])
    if name == 'plus sign':
        assert out['angle'][0] == 0.0                   # isotropic: atan2(0, 0)
        assert out['major'][0] == pytest.approx(3.0) and out['minor'][0] == pytest.approx(3.0)
        assert out['cell_area'][0] == pytest.approx(5 * math.pi / 4)


def test_nan_agent_is_in_no_colony_whatever_min_cells():
    x, y, th, L, keys = scenario_arrays(SCENARIOS['outlier and NaN'][0])
    out = ref.analyse(x, y, th, L, keys, BOUNDS, width=1.0, gap=0.25, min_cells=1)
    assert out['n_colonies'] == 2 and out['colony'][6] == -1 and out['colony'][4] >= 0


def random_capsules(seed, n, patch):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, patch, n), rng.uniform(0.0, patch, n), rng.uniform(0.0, 2 * math.pi, n),
            rng.uniform(1.0, 4.0, n), rng.permutation(n * 3)[:n].astype(np.int64))


def test_restatement_is_invariant_under_permutation():
    x, y, th, L, keys = random_capsules(5, 257, 30.0)
    bounds = (41.5, 37.0)
    mass = np.random.default_rng(6).uniform(500.0, 2000.0, 257)
    a = ref.analyse(x, y, th, L, keys, bounds, gap=0.25, mass=mass)
    assert a['tie'] >= 1e-9 and a['n_colonies'] >= 2
    perm = np.random.default_rng(7).permutation(257)
    b = ref.analyse(x[perm], y[perm], th[perm], L[perm], keys[perm], bounds, gap=0.25, mass=mass[perm])
    assert np.array_equal(a['colony'][perm], b['colony'])
    assert np.array_equal(a['cells'], b['cells']) and np.array_equal(a['key'], b['key'])
    for name in ref.ROWS:                              # fsum and max / min: exact whatever the order
        assert np.array_equal(a[name], b[name]), name
