"""Host side of colony mechanics (no GPU): ContactModel's argument checks, the
combinations Colony(mechanics=...) refuses -- before anything is built -- and
self-checks of the NumPy restatement the GPU tests compare the kernel with
(tests/mechanics_ref.py)."""

import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import mechanics_ref as ref
from lens_amd import configs
from lens_amd.cells import CellModel
from lens_amd.mechanics import ContactModel
from lens_amd.motility import MotilityModel


def test_model_defaults_and_grid():
    m = ContactModel()
    assert (m.iterations, m.stiffness, m.max_length, m.width, m.length) == (4, 0.5, 4.0, 1.0, 2.0)
    assert m.max_push == 0.5 and m.max_turn == 0.5 and m.jitter == 0.0 and m.jitter_angle == 0.0
    assert ContactModel(width=1.5).max_push == 0.75 and ContactModel(max_push=0.1).max_push == 0.1
    assert m.grid((41.5, 37.0)) == (10, 9) and m.grid((3.0, 128.0)) == (1, 32)
    assert m.grid((41.5, 37.0)) == ref.grid((41.5, 37.0), 4.0)[:2]
    p = m.vk_params((41.5, 37.0))
    assert (p.iterations, p.gx, p.gy, p.max_push, p.seed) == (4, 10, 9, 0.5, 0)
    a = m.initial_angles(3, 5)
    assert a.shape == (5,) and np.all((a[:3] >= 0) & (a[:3] < 2 * np.pi)) and np.all(a[3:] == 0)
    assert np.array_equal(a, m.initial_angles(3, 5))          # seeded
    assert np.array_equal(ContactModel(angles=[0.5, 1.5, 2.5]).initial_angles(3, 4), [0.5, 1.5, 2.5, 0.0])
    with pytest.raises(ValueError, match='angle'):
        ContactModel(angles=[0.5]).initial_angles(3, 5)


@pytest.mark.parametrize('kw,match', [
    ({'iterations': 0}, 'iterations'), ({'iterations': -1}, 'iterations'),
    ({'stiffness': 0.0}, 'stiffness'), ({'stiffness': 1.5}, 'stiffness'), ({'stiffness': -0.1}, 'stiffness'),
    ({'max_length': 0.5}, 'max_length'), ({'width': 2.0, 'max_length': 1.9}, 'max_length'),
    ({'width': 0.0}, 'width'), ({'length': 0.0}, 'length'), ({'max_push': -1.0}, 'max_push'),
    ({'max_turn': -1.0}, 'max_turn'), ({'jitter': -1.0}, 'jitter'),
])
def test_model_rejects_out_of_range_parameters(kw, match):
    with pytest.raises(ValueError, match=match):
        ContactModel(**kw)


def test_model_rejects_unknown_parameters():
    with pytest.raises(ValueError, match='unknown ContactModel parameters'):
        ContactModel(stifness=0.5)
    assert ContactModel(stiffness=1.0).stiffness == 1.0           # the closed end of (0, 1]


def _lattice(**kw):
    from lens_amd.lattice import Lattice
    return Lattice(['glc__D_e', 'lcts_e', 'MeAsp'], (8, 8), (16.0, 16.0), 10.0, 5.0, device='cpu', **kw)


def test_colony_names_each_unsupported_combination():
    from lens_amd.colony import Colony
    cfg = configs.glc_lct_config()
    m = ContactModel()
    mk = lambda **kw: Colony(cfg, 4, device='cpu', integrator='euler', mechanics=m, **kw)
    with pytest.raises(ValueError, match='Lattice environment'):
        mk(environment='held')
    with pytest.raises(ValueError, match='Lattice environment'):
        mk(environment='nonspatial')
    with pytest.raises(ValueError, match='unbanded'):
        mk(environment=_lattice(row_band=(0, 4), halo=1))
    with pytest.raises(ValueError, match='motility'):
        mk(environment=_lattice(), motility=MotilityModel())
    with pytest.raises(ValueError, match='width'):
        mk(environment=_lattice(), cells=CellModel(width=2))


def test_router_refuses_a_colony_with_mechanics():
    """The router attaches after construction, so it makes the check itself (before
    it touches the colony: a stand-in with the attribute is enough here)."""
    import types
    from lens_amd.distributed import AgentRouter
    with pytest.raises(ValueError, match='router'):
        AgentRouter(types.SimpleNamespace(motility=None, mechanics=ContactModel()), 0, 1, agent_offset=0)


# -- the restatement ----------------------------------------------------------------
BOUNDS = (40.0, 40.0)


def _iterate(x, y, th, L, **kw):
    n = len(x)
    return ref.iterate(np.array(x, float), np.array(y, float), np.array(th, float), np.array(L, float),
                       np.arange(n), BOUNDS, 0, **kw)


@pytest.mark.parametrize('stiffness', [0.5, 1.0, 0.25])
def test_two_discs_separate_along_their_centre_line_by_stiffness_times_overlap(stiffness):
    # discs (L = w = 1) 0.6 apart along a 3-4-5 direction: overlap 0.4
    x, y = [10.0, 10.0 + 0.6 * 0.6], [10.0, 10.0 + 0.6 * 0.8]
    nx, ny, nt = _iterate(x, y, [0.3, 1.1], [1.0, 1.0], stiffness=stiffness)
    d0 = math.hypot(x[1] - x[0], y[1] - y[0])
    d1 = math.hypot(nx[1] - nx[0], ny[1] - ny[0])
    assert abs((d1 - d0) - stiffness * (1.0 - d0)) <= 1e-14
    # along the centre line: the new separation is parallel to the old
    cross = (nx[1] - nx[0]) * (y[1] - y[0]) - (ny[1] - ny[0]) * (x[1] - x[0])
    assert abs(cross) <= 1e-15
    assert np.array_equal(nt, [0.3, 1.1])                     # a disc's spine has no lever


def test_degenerate_normals():
    # coincident centres: the smaller key goes +x, the other -x, by stiffness * 2r / 2 each
    nx, ny, _ = _iterate([5.0, 5.0], [7.0, 7.0], [0.2, 1.3], [2.0, 3.0])
    assert nx[0] == 5.25 and nx[1] == 4.75 and ny[0] == 7.0 and ny[1] == 7.0
    # crossing spines (closest points coincide, centres do not): along the centre line
    nx, ny, _ = _iterate([5.0, 5.25], [7.0, 7.0], [0.0, math.pi / 2], [3.0, 3.0])
    assert nx[0] < 5.0 and nx[1] > 5.25 and abs(ny[0] - 7.0) <= 1e-15 and abs(ny[1] - 7.0) <= 1e-15


def test_pair_pushes_are_equal_and_opposite_and_the_centroid_stays():
    rng = np.random.default_rng(5)
    n = 60
    x, y = rng.uniform(10.0, 18.0, n), rng.uniform(10.0, 18.0, n)
    th, L = rng.uniform(0.0, 2 * np.pi, n), rng.uniform(1.0, 4.0, n)
    info = {}
    nx, ny, _ = ref.iterate(x, y, th, L, np.arange(n), BOUNDS, 0, max_push=math.inf, clamp=False, info=info)
    px, py = info['px'], info['py']
    assert info['contact'].sum() >= 40 and np.array_equal(info['contact'], info['contact'].T)
    # |push on i from j + push on j from i| within rounding of the closest-point solve
    assert np.abs(px + px.T).max() <= 1e-13 and np.abs(py + py.T).max() <= 1e-13
    assert abs(nx.mean() - x.mean()) <= 1e-13 and abs(ny.mean() - y.mean()) <= 1e-13
    assert np.abs(nx - x).max() > 0.05                        # something did move


def test_cap_turn_limit_and_walls():
    # eight discs on one spot: the sum of seven full pushes is capped at max_push = r
    n = 8
    x, y = np.full(n, 0.1), np.full(n, 39.95)
    info = {}
    nx, ny, _ = ref.iterate(x, y, np.zeros(n), np.ones(n), np.arange(n), BOUNDS, 0, stiffness=1.0, info=info)
    assert info['capped'].any()
    assert np.all(np.hypot(nx - x, ny - y) <= 0.5 + 1e-15)
    assert np.all((nx >= 0.0) & (nx < BOUNDS[0]) & (ny >= 0.0) & (ny < BOUNDS[1]))
    assert (nx == 0.0).any()                                  # pushed into the wall and clamped


def test_restatement_draws_depend_on_key_and_iteration_only():
    x, y = np.array([5.0, 25.0]), np.array([5.0, 25.0])
    th, L = np.zeros(2), np.full(2, 2.0)
    kw = dict(jitter=0.01, jitter_angle=0.02, seed=3)
    a = ref.iterate(x, y, th, L, np.array([0, 1]), BOUNDS, 4, **kw)
    b = ref.iterate(x[::-1].copy(), y[::-1].copy(), th, L, np.array([1, 0]), BOUNDS, 4, **kw)
    assert all(np.array_equal(p, q[::-1]) for p, q in zip(a, b))
    c = ref.iterate(x, y, th, L, np.array([0, 1]), BOUNDS, 5, **kw)
    assert not np.array_equal(a[0], c[0])
    assert 0 < abs(a[0][0] - 5.0) < 0.1 and 0 < abs(a[2][0]) < 0.2
