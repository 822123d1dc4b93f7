"""Host side of the static fields (no GPU): the NumPy restatement the GPU tests compare the
kernels with (tests/static_field_ref.py) against the fixture made from the reference's own
functions (tests/golden/gradients.npz), the StaticField model's validation, the reference
experiment's numbers, the ctypes struct against the header, and the refusals of
Colony(environment=StaticField(...)), which come before anything is allocated.

One finding is pinned here.  The reference squares with ``dx ** 2`` on Python floats, which
is the C library's pow(dx, 2.0); the device (and the restatement's default) multiplies.  The
two agree to the last bit except in about one square in a thousand, where pow is off the
correctly rounded product by one ulp.  ``squares='reference'`` restates the reference's own
call and equals the fixture bit for bit; the product differs from it at one of the fixture's
64 points, by one or two units in the last place of the distance.
"""

import ctypes
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import static_field_ref as sref
from lens_amd import configs, native
from lens_amd.motility import FlagellaModel, MotilityModel
from lens_amd.static_field import StaticField, gradient_specs

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'vk_kinetics.h')


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(HERE, 'golden', 'gradients.npz'))


def _stack(fields):
    return np.stack([fields['a'], fields['b']])


def test_fixture_is_the_configured_cases(fixture):
    assert list(fixture['molecules']) == ['a', 'b'] and tuple(fixture['types']) == sref.TYPES
    assert tuple(fixture['grid_bins']) == sref.GRID_BINS and tuple(fixture['grid_bounds']) == sref.GRID_BOUNDS
    assert np.array_equal(fixture['points'], sref.points())
    assert os.path.getsize(os.path.join(HERE, 'golden', 'gradients.npz')) < 16384


@pytest.mark.parametrize('kind', sref.TYPES)
def test_restated_make_gradient_equals_the_reference_bit_for_bit(fixture, kind):
    ours = _stack(sref.make_gradient(sref.GRID[kind], sref.GRID_BINS, sref.GRID_BOUNDS, squares='reference'))
    assert ours.shape == (2, 5, 7) and np.array_equal(ours, fixture['grid_' + kind])
    # on this grid no square is one of pow's misses: the device's order gives the same bits
    assert np.array_equal(_stack(sref.make_gradient(sref.GRID[kind], sref.GRID_BINS, sref.GRID_BOUNDS)), ours)


@pytest.mark.parametrize('kind', sref.FIELD_TYPES)
def test_restated_concentration_equals_the_reference_bit_for_bit(fixture, kind):
    ours = _stack(sref.concentration(sref.POINTS[kind], sref.POINT_BOUNDS, fixture['points'], squares='reference'))
    assert np.array_equal(ours, fixture['points_' + kind])


@pytest.mark.parametrize('kind', sref.FIELD_TYPES)
def test_product_squares_stay_within_an_ulp_of_the_distance(fixture, kind):
    """pow(dx, 2.0) is within one ulp of dx * dx, so the distance moves by at most 2^-52 of
    itself (the square root halves a relative error, its own rounding adds half an ulp); a
    value f(d) moves by at most |d f'(d)| 2^-52 plus its own rounding."""
    ref = fixture['points_' + kind]
    ours = _stack(sref.concentration(sref.POINTS[kind], sref.POINT_BOUNDS, fixture['points']))
    differ = int((ours != ref).sum())
    print('%s: %d of %d values differ from the reference, worst %.3g relative' % (
        kind, differ, ref.size, np.abs(ours / ref - 1).max()))
    assert differ <= 2
    # |d f'(d) / f| over the fixture: gaussian d^2 / dev^2 <= 16, linear <= 32 (a value near its
    # zero), exponential d |ln base| <= 16; two ulps of slack for the value's own roundings
    assert np.abs(ours / ref - 1).max() <= (32 + 2) * 2.0 ** -52


def test_reference_experiment_numbers():
    """experiments/chemotaxis.py:70-136."""
    for kind in ('exponential', 'linear'):
        c = configs.chemotaxis_static(kind, n_agents=3, seed=7)
        f, m = c['field'], c['motility']
        assert isinstance(f, StaticField) and isinstance(m, MotilityModel)
        assert f.bounds == [1000.0, 3000.0] and f.molecules == ['glc__D_e'] and m.ligand_id == 'glc__D_e'
        assert np.array_equal(c['location'], [[500.0] * 3, [300.0] * 3]) and m.seed == 7
        g = f.spec('glc__D_e')
        assert (g.cx, g.cy) == (500.0, 0.0)
        if kind == 'exponential':
            assert (g.type, g.p0, g.p1) == (native.VK_GRADIENT_EXPONENTIAL, 1.3e2, 4.0)
            assert m.initial_ligand == 4.0 * 1.3e2 ** (300 / 1000)          # the reference's INITIAL_LIGAND
        else:
            assert (g.type, g.p0, g.p1) == (native.VK_GRADIENT_LINEAR, 1e-1, 1.0)
            assert m.initial_ligand == 1e-1 + 1.0 * (300 / 1000)
        assert m.initial_ligand == f.value('glc__D_e', 500.0, 300.0)
    assert configs.chemotaxis_static(flagella=FlagellaModel(5))['motility'].flagella is not None
    with pytest.raises(ValueError, match='exponential'):
        configs.chemotaxis_static('gaussian')
    assert configs.mother_machine()['gradient']['type'] == 'gaussian'


@pytest.mark.parametrize('kind', sref.FIELD_TYPES)
def test_host_value_is_the_restatement(fixture, kind):
    f = StaticField(['a', 'b', 'unwritten'], sref.POINT_BOUNDS, sref.POINTS[kind])
    assert f.gradient_molecules == ['a', 'b']
    want = sref.concentration(sref.POINTS[kind], sref.POINT_BOUNDS, fixture['points'])
    for mol in 'ab':
        got = [f.value(mol, x, y) for x, y in fixture['points'].T]
        if kind == 'gaussian':
            # math.exp and NumPy's exp are two implementations, each within an ulp of the truth
            assert np.abs(np.array(got) / want[mol] - 1).max() <= 2 * 2.0 ** -52
        else:
            assert np.array_equal(got, want[mol])
    with pytest.raises(ValueError, match='no gradient'):
        f.value('unwritten', 1.0, 1.0)


def test_defaults_are_the_references():
    _, (lin,) = gradient_specs({'type': 'linear', 'molecules': {'a': {'center': [0.5, 0.5], 'slope': 2}}}, (10, 20))
    assert (lin.p0, lin.p1, lin.cx, lin.cy) == (0.0, 2.0, 5.0, 10.0)
    _, (ex,) = gradient_specs({'type': 'exponential', 'molecules': {'a': {'center': [0, 1], 'base': 3}}}, (10, 20))
    assert (ex.p0, ex.p1) == (3.0, 1.0)
    # negative linear values are passed on as they are
    f = StaticField(['a'], (10, 20), {'type': 'linear', 'molecules': {'a': {'center': [0, 0], 'slope': -1e4}}})
    assert f.value('a', 10.0, 20.0) < 0


def test_model_validation():
    mk = lambda kind, spec, molecules=('a',): StaticField(list(molecules), (10, 20), {'type': kind,
                                                                                     'molecules': {'a': spec}})
    with pytest.raises(ValueError, match='unknown gradient type'):
        mk('quadratic', {'center': [0, 0]})
    with pytest.raises(ValueError, match='unknown gradient type'):
        StaticField(['a'], (10, 20), {})
    with pytest.raises(ValueError, match='uniform'):
        mk('uniform', 1.0)
    with pytest.raises(ValueError, match="'a' is not one of the molecules"):
        mk('linear', {'center': [0, 0], 'slope': 1}, molecules=('b',))
    for base in (0.0, -2.0):
        with pytest.raises(ValueError, match='base must be positive'):
            mk('exponential', {'center': [0, 0], 'base': base})
    with pytest.raises(ValueError, match='zero deviation'):
        mk('gaussian', {'center': [0, 0], 'deviation': 0})
    # the lattice's make_gradient takes uniform, but the same rules otherwise
    assert gradient_specs({'type': 'uniform', 'molecules': {'a': 2}}, (1, 1))[1][0].p0 == 2.0
    with pytest.raises(ValueError, match='zero deviation'):
        gradient_specs({'type': 'gaussian', 'molecules': {'a': {'center': [0, 0], 'deviation': 0.0}}}, (1, 1))


def test_struct_matches_the_header():
    text = open(HEADER).read()
    m = re.search(r'typedef struct \{([^}]*)\} vk_gradient_spec;', text)
    fields = [(t, n.strip()) for t, names in re.findall(r'(int32_t|double)\s+([^;]+);', m.group(1))
              for n in names.split(',')]
    ctype = {'int32_t': ctypes.c_int32, 'double': ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == native.VkGradientSpec._fields_
    # C layout: the int32 is padded to the doubles' alignment
    assert ctypes.sizeof(native.VkGradientSpec) == 40
    assert [getattr(native.VkGradientSpec, n).offset for _, n in fields] == [0, 8, 16, 24, 32]
    enum = re.search(r'enum \{ (VK_GRADIENT_UNIFORM[^}]*)\}', text).group(1)
    for name, v in re.findall(r'(VK_GRADIENT_\w+) = (\d+)', enum):
        assert getattr(native, name) == int(v)
    assert int(re.search(r'#define VK_GRADIENT_MAX (\d+)', text).group(1)) == native.VK_GRADIENT_MAX
    array = StaticField(['a', 'b'], sref.POINT_BOUNDS, sref.POINTS['linear']).specs()
    assert ctypes.sizeof(array) == 80 and array[1].p1 == -0.25


def test_every_new_export_is_declared():
    text = open(HEADER).read()
    for name in ('vk_gradient_fill', 'vk_static_gather', 'vk_motility_step_static', 'vk_flagella_step_static'):
        assert re.search(r'^int %s\(' % name, text, re.M), name
        assert name in native.EXPORTS and name in native._SIGS
    # the static steps take the plane steps' argument lists, a spec where the plane is
    for name in ('vk_motility_step', 'vk_flagella_step'):
        plane, static = native._SIGS[name][0], native._SIGS[name + '_static'][0]
        i = next(k for k, (a, b) in enumerate(zip(plane, static)) if a is not b)
        assert static[i] is ctypes.POINTER(native.VkGradientSpec) and plane[:i] + plane[i + 1:] == static[:i] + static[i + 1:]


def test_colony_refuses_what_a_static_field_cannot_carry():
    """Before anything is allocated: on the CPU device nothing could be."""
    from lens_amd.cells import CellModel
    from lens_amd.colony import Colony
    from lens_amd.mechanics import ContactModel
    from lens_amd.response import ANTIBIOTICS_DEFAULTS, CellResponse
    from lens_amd.stochastic import StochasticModel
    cfg = configs.glc_lct_config()
    c = configs.chemotaxis_static()
    mk = lambda **kw: Colony(cfg, 4, device='cpu', integrator='euler', environment=c['field'], **kw)
    with pytest.raises(ValueError, match='takes no mechanics='):
        mk(mechanics=ContactModel())
    with pytest.raises(ValueError, match='takes no response='):
        mk(response=CellResponse(membrane=ANTIBIOTICS_DEFAULTS['diffusion']))
    with pytest.raises(ValueError, match='takes no cells='):
        mk(cells=CellModel())
    with pytest.raises(ValueError, match='takes no cells='):
        mk(cells=CellModel(), motility=MotilityModel(ligand_id='glc__D_e', division='merged'))
    with pytest.raises(ValueError, match='takes no stochastic='):
        mk(stochastic=StochasticModel.__new__(StochasticModel))
    with pytest.raises(ValueError, match="no gradient of 'MeAsp'"):
        mk(motility=MotilityModel())


def test_router_refuses_a_static_colony():
    import types
    from lens_amd.distributed import AgentRouter
    col = types.SimpleNamespace(motility=None, mechanics=None, stochastic=None, static=object())
    with pytest.raises(ValueError, match='StaticField takes no router'):
        AgentRouter(col, 0, 2)
