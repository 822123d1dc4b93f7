"""NumPy restatement of the static-field arithmetic for the tests: the value of a gradient
(vk_gradient.h), make_gradient (vivarium/processes/diffusion_field.py:42-206),
StaticField.get_concentration (vivarium/processes/static_field.py:92-119), and the motile
steps with the ligand sensed at the agent's own position (vk_motility_step_static,
vk_flagella_step_static).

The motile steps are the restated steps of tests/motility_ref.py and tests/flagella_ref.py,
one inner update at a time: each inner update is handed a "plane" that answers every bin
with the field at the position the previous inner update left -- everything else (receptor,
motor, draws, move, bins) is those modules' code, unchanged.

GRID and POINTS are the gradients of the fixture tests/golden/gradients.npz (made from the
reference's own functions by tests/golden/make_gradient_ref.py).
"""

import numpy as np

import flagella_ref as fref
import motility_ref as mref

TYPES = ('uniform', 'gaussian', 'linear', 'exponential')
FIELD_TYPES = TYPES[1:]

# the fixture's cases: all four types on a 5 x 7 grid over bounds (10, 21) ...
GRID_BINS, GRID_BOUNDS = (5, 7), (10, 21)
GRID = {
    'uniform': {'type': 'uniform', 'molecules': {'a': 1.5, 'b': 0.25}},
    'gaussian': {'type': 'gaussian', 'molecules': {'a': {'center': [0.25, 0.5], 'deviation': 0.01},
                                                   'b': {'center': [1.0, 0.0], 'deviation': -0.02}}},
    # b's default base is 0.0; a goes negative far from its centre, and is passed on as it is
    'linear': {'type': 'linear', 'molecules': {'a': {'center': [0.0, 0.0], 'base': 0.1, 'slope': -10},
                                               'b': {'center': [0.75, 0.3], 'slope': 5}}},
    # b's default scale is 1
    'exponential': {'type': 'exponential', 'molecules': {'a': {'center': [0.5, 0.0], 'base': 1e4, 'scale': 2.0},
                                                         'b': {'center': [0.1, 0.9], 'base': 0.5}}},
}
# ... and the three field types at 64 random locations on (1000, 3000)
N_POINTS, POINT_BOUNDS, POINT_SEED = 64, (1000, 3000), 20261020
POINTS = {
    'gaussian': {'type': 'gaussian', 'molecules': {'a': {'center': [0.5, 0.5], 'deviation': 0.8},
                                                   'b': {'center': [0.0, 1.0], 'deviation': 2}}},
    'linear': {'type': 'linear', 'molecules': {'a': {'center': [0.5, 0.0], 'base': 1e-1, 'slope': 1.0},
                                               'b': {'center': [1.0, 1.0], 'slope': -0.25}}},
    'exponential': {'type': 'exponential', 'molecules': {'a': {'center': [0.5, 0.0], 'base': 1.3e2, 'scale': 4.0},
                                                         'b': {'center': [0.2, 0.6], 'base': 0.7}}},
}


def points():
    """The fixture's locations [2, N_POINTS] (also stored in it)."""
    rng = np.random.default_rng(POINT_SEED)
    return np.stack([rng.uniform(0.0, POINT_BOUNDS[0], N_POINTS), rng.uniform(0.0, POINT_BOUNDS[1], N_POINTS)])


def _scalar_pow(x, y):
    """x ** y element by element on Python floats: the C library's pow, which is what the
    reference's scalar ``**`` calls (NumPy's array loop is another implementation)."""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    out = np.array([float(a) ** float(b) for a, b in zip(x.ravel().tolist(), y.ravel().tolist())], dtype=np.float64)
    return out.reshape(x.shape)


def value(kind, spec, bounds, x, y, squares='product'):
    """One molecule's gradient at (x, y) (arrays or scalars), in the device function's order.

    ``squares``: the reference writes ``dx ** 2`` on Python floats, which is the C library's
    pow(dx, 2.0) -- within an ulp of, but in about one case in a thousand not equal to, the
    correctly rounded product.  'product' (the device's dx * dx, the default) or 'reference'
    (the reference's own call, which the fixture holds)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if kind == 'uniform':
        return np.full(np.broadcast(x, y).shape, float(spec))
    dx = x - spec['center'][0] * bounds[0]
    dy = y - spec['center'][1] * bounds[1]
    if squares == 'reference':
        d = np.sqrt(_scalar_pow(dx, 2) + _scalar_pow(dy, 2)) / 1000.0
    else:
        assert squares == 'product', squares
        d = np.sqrt(dx * dx + dy * dy) / 1000.0
    if kind == 'gaussian':
        deviation = float(spec['deviation'])
        return np.exp((-(d * d)) / (2.0 * (deviation * deviation)))
    if kind == 'linear':
        return float(spec.get('base', 0.0)) + float(spec['slope']) * d
    assert kind == 'exponential', kind
    return float(spec.get('scale', 1)) * _scalar_pow(float(spec['base']), d)


def make_gradient(gradient, n_bins, bounds, squares='product'):
    """{molecule: [nx, ny]}: every bin's middle, parenthesised as the reference does."""
    x = ((np.arange(n_bins[0]) + 0.5) * bounds[0]) / n_bins[0]
    y = ((np.arange(n_bins[1]) + 0.5) * bounds[1]) / n_bins[1]
    return {m: value(gradient['type'], spec, bounds, x[:, None], y[None, :], squares)
            for m, spec in gradient['molecules'].items()}


def concentration(gradient, bounds, loc, squares='product'):
    """{molecule: [n]} at loc [2, n]: get_concentration for every agent."""
    return {m: value(gradient['type'], spec, bounds, loc[0], loc[1], squares) for m, spec in gradient['molecules'].items()}


class _Sensed:
    """Stands where the restated steps take a ligand plane: whatever the bin, the field at
    the agents' current positions."""

    def __init__(self, n_bins, values):
        self.shape, self.values = tuple(n_bins), values

    def __getitem__(self, bins):
        return self.values


def _ligand(field, ligand_id, loc):
    return value(field.gradient['type'], field.gradient['molecules'][ligand_id], field.bounds, loc[0], loc[1])


def motility_step(model, field, motil, loc, dt, substeps, counter, keys=None, margins=None):
    """vk_motility_step_static: ``substeps`` inner updates in place on motil [9, n] and
    loc [2, n] in the StaticField ``field``; returns the linear bins."""
    h = dt / substeps
    bins = None
    for s in range(substeps):
        sensed = _Sensed(field.n_bins, _ligand(field, model.ligand_id, loc))
        bins = mref.step(model, motil, loc, sensed, field.bounds, h, 1, counter + s, keys=keys, margins=margins)
    return bins


def flagella_step(model, field, motil, flag, flag_int, loc, dt, substeps, counter, keys=None, margins=None):
    """vk_flagella_step_static, as :func:`motility_step`."""
    h = dt / substeps
    bins = None
    for s in range(substeps):
        sensed = _Sensed(field.n_bins, _ligand(field, model.ligand_id, loc))
        bins = fref.step(model, motil, flag, flag_int, loc, sensed, field.bounds, h, 1, counter + s, keys=keys,
                         margins=margins)
    return bins
