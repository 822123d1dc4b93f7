"""Cell growth, derivers and division for a device-resident colony.

Host half of ``vk_cell_step`` / ``vk_divide_*`` (include/vk_kinetics.h).  A
:class:`CellModel` carries the reference processes' parameters:

``model='growth_protein'`` -- GrowthProtein + TreeMass + DeriveGlobals +
    MetaDivision (the ``growth_division_minimal`` agent of the reference's
    colony_metrics experiment; vivarium/compartments/growth_division_minimal.py).
``model='growth'`` -- Growth + DeriveGlobals + DivisionVolume + MetaDivision
    (SURVEY §8d C5).
``model='tree_mass'`` -- no growth process: TreeMass over the colony's count table from
    ``initial_mass`` + DeriveGlobals + DivisionVolume + MetaDivision (``GeneExpression``'s own
    cell, vivarium/compartments/gene_expression.py:62-77).

``molecular_weights`` ({row name of the colony's count table: g/mol}) makes TreeMass fold those
rows into the mass (``vk_cell_step_tree``): with ``'growth_protein'`` after the aggregate
protein, with ``'tree_mass'`` from ``initial_mass``.  The rows are folded in ascending table
order -- THE ENGINE'S OWN order.

Scalars that the reference computes with numpy / pint (``exp(r*dt)``, the
capsule constants, unit-conversion factors) are evaluated here, in Python,
exactly as the reference writes them, and handed to the kernel, so the
device arithmetic reproduces the reference bit for bit.

Random remainder of GrowthProtein (growth_protein.py:94-96):
``rng='stream'`` draws the uniforms on the host from numpy's MT19937 in
agent order -- the reference's own stream (``np.random.seed(seed)``; the
reference's colony_metrics setup consumes ``setup_draws=2`` draws first);
``rng='philox'`` draws them on the device from Philox4x32-10 keyed by
(seed, step, lineage), independent of agent order and rank count.
"""

from __future__ import annotations

import ctypes
import dataclasses
import math
from typing import Dict, Optional

import numpy as np

from lens_amd import native

N_A_LEGACY = 6.022140857e23
PI = math.pi
# unit-conversion factors as pint evaluates them in the reference
FG_PER_G = 1 / 1e-15                          # g -> fg (TreeMass.calculate_mass)
VOLUME_TO_FL = 1e-18 / 1e-3 * 1e18 * 1e-3     # fg*L/g -> fL (DeriveGlobals volume.to('fL'))

MODELS = {'growth_protein': native.VK_GROWTH_PROTEIN, 'growth': native.VK_GROWTH_MASS,
          'tree_mass': native.VK_GROWTH_TREE}
RNGS = {'stream': native.VK_RNG_STREAM, 'philox': native.VK_RNG_PHILOX}


@dataclasses.dataclass
class CellModel:
    model: str = 'growth_protein'
    growth_rate: float = 0.000275          # growth_protein.py:27 (Growth: 0.0006, growth.py:61)
    division_volume: float = 2.4           # fL, division_volume.py:13
    initial_mass: float = 1339.0           # fg
    protein_mw: float = 2.09e4             # g/mol, growth_protein.py:26
    width: float = 1                       # um, derive_globals.py:60 (an int there: emitted as 1)
    density: float = 1100.0                # g/L, derive_globals.py:93
    avogadro: float = N_A_LEGACY
    rng: str = 'stream'
    seed: int = 1
    setup_draws: int = 0
    molecular_weights: Optional[Dict[str, float]] = None     # {row of the count table: g/mol} (TreeMass)

    def __post_init__(self):
        if self.model not in MODELS:
            raise ValueError('model must be one of %s' % sorted(MODELS))
        if self.rng not in RNGS:
            raise ValueError('rng must be one of %s' % sorted(RNGS))
        self._rs = None
        mw = self.molecular_weights
        if mw is not None:
            if not isinstance(mw, dict):
                raise ValueError('molecular_weights must be {row name: g/mol}')
            if self.model == 'growth':
                raise ValueError("molecular_weights with model='growth': Growth writes the mass itself, there is "
                                 'no TreeMass to fold them into')
            if len(mw) > native.VK_TREE_MAX_WEIGHTED:
                raise ValueError('molecular_weights: at most %d rows (got %d)' % (native.VK_TREE_MAX_WEIGHTED, len(mw)))
            clean = {}
            for name, w in mw.items():
                try:
                    w = float(w)
                except (TypeError, ValueError):
                    raise ValueError('molecular_weights: the weight of %r is not a number' % (name,))
                if not math.isfinite(w) or w < 0:
                    raise ValueError('molecular_weights: the weight of %r must be finite and >= 0 (got %r)' % (name, w))
                clean[str(name)] = w             # 0.0 stays: the reference folds every node with the property
            self.molecular_weights = clean
        if self.model == 'tree_mass' and not self.molecular_weights:
            raise ValueError("model='tree_mass' needs molecular_weights: without them the mass never moves")

    @property
    def weighted(self) -> bool:
        """Whether TreeMass folds rows of the count table (vk_cell_step_tree)."""
        return bool(self.molecular_weights)

    # -- reference formulas (Python floats, the reference's operation order) --
    def initial_protein(self) -> float:
        """growth_protein.py:46-47: initial_mass.to('g') / protein_mw * N_A."""
        return self.initial_mass * 1e-15 / self.protein_mw * self.avogadro

    def tree_mass(self, protein: float = None, weighted=(), initial_mass: float = None) -> float:
        """TreeMass (tree_mass.py:10-18): from 0 fg and the aggregate ``protein``, or in the
        ``'tree_mass'`` model from ``initial_mass`` (default the model's); then ``weighted``,
        (g/mol, count) pairs in the fold's order (:meth:`TreeWeights.pairs`).  Counts and
        ``initial_mass`` may be arrays over agents: numpy does the same IEEE operations
        elementwise."""
        if self.model == 'tree_mass':
            m = np.float64(self.initial_mass) if initial_mass is None else np.asarray(initial_mass, dtype=np.float64)
        else:
            m = 0.0 + (self.protein_mw * (protein / self.avogadro)) * FG_PER_G
        for w, count in weighted:
            m = m + (float(w) * (np.asarray(count, dtype=np.float64) / self.avogadro)) * FG_PER_G
        return m

    def capsule(self):
        radius = self.width / 2
        return {'cap_volume': (4 / 3) * PI * radius ** 3, 'cap_area': PI * radius ** 2,
                'two_r': 2 * radius, 'sa_const': 3 * PI * radius ** 2, 'sa_lin': 2 * PI * radius}

    def derive(self, mass: float):
        """DeriveGlobals on one mass: (volume fL, mmol_to_counts, length, surface_area)."""
        c = self.capsule()
        raw = mass / self.density
        length = (raw - c['cap_volume']) / c['cap_area'] + c['two_r']
        area = c['sa_const'] + c['sa_lin'] * (length - self.width)
        return raw * VOLUME_TO_FL, self.avogadro * (raw * 1e-15) * 1e-3, length, area

    def initial_rows(self, n: int, mass=None, weighted=None):
        """Cell rows [VK_CELL_ROWS, n] + mmol_to_counts [n] after the
        initial deriver pass (experiment.py:1247).  A model with ``molecular_weights`` needs
        ``weighted``: (g/mol, initial counts [n]) pairs in the fold's order
        (:meth:`TreeWeights.pairs`); in the ``'tree_mass'`` model ``mass`` is the agents'
        ``initial_mass`` (default the model's)."""
        rows = np.zeros((native.VK_CELL_ROWS, n))
        m2c = np.zeros(n)
        if self.weighted and weighted is None:
            raise ValueError('initial_rows: a model with molecular_weights needs the initial counts of the '
                             'weighted rows (weighted=)')
        if self.weighted or self.model == 'tree_mass':
            p0 = self.initial_protein()
            if self.model == 'growth_protein':
                rows[native.VK_CELL_PROTEIN] = p0
            folded = self.tree_mass(p0, weighted, self.initial_mass if mass is None else mass)
            mass = np.array(np.broadcast_to(folded, (n,)), dtype=np.float64)
        elif self.model == 'growth_protein':
            p0 = self.initial_protein()
            mass = np.full(n, self.tree_mass(p0))
            rows[native.VK_CELL_PROTEIN] = p0
        else:
            mass = np.full(n, self.initial_mass) if mass is None else np.asarray(mass, dtype=np.float64)
        for a in range(n):
            v, mc, length, area = self.derive(float(mass[a]))
            rows[:4, a] = (mass[a], v, length, area)
            m2c[a] = mc
        return rows, m2c

    # -- kernel parameters ----------------------------------------------------
    def vk_params(self, dt: float, step: int) -> native.VkCellParams:
        p = native.VkCellParams()
        p.model = MODELS[self.model]
        p.rng = RNGS[self.rng]
        p.factor = float(np.exp(self.growth_rate * dt))
        p.divide_protein = self.initial_protein() * 2
        p.division_volume = self.division_volume
        p.protein_mw = self.protein_mw
        p.avogadro = self.avogadro
        p.fg_per_g = FG_PER_G
        p.density = self.density
        p.volume_to_fl = VOLUME_TO_FL
        for k, v in self.capsule().items():
            setattr(p, k, v)
        p.width = self.width
        p.seed = int(self.seed) & (2 ** 64 - 1)
        p.step = int(step) & (2 ** 64 - 1)
        return p

    def host_uniforms(self, n: int) -> np.ndarray:
        """The next n draws of numpy's MT19937 stream (rng='stream')."""
        if self._rs is None:
            self._rs = np.random.RandomState(self.seed)
            if self.setup_draws:
                self._rs.random_sample(self.setup_draws)
        return self._rs.random_sample(n)

    def bind(self, stochastic) -> 'TreeWeights':
        """The weighted rows of ``stochastic``'s count table (active or passive), sorted by row:
        what vk_cell_step_tree folds.  ValueError: a name that is no row of the table."""
        rows = stochastic.rows
        index = {name: r for r, name in enumerate(rows)}
        unknown = [name for name in (self.molecular_weights or {}) if name not in index]
        if unknown:
            raise ValueError('molecular_weights: %s: no rows of the count table (rows: %s)' % (
                ', '.join(map(repr, unknown)), rows))
        pairs = sorted((index[name], w) for name, w in (self.molecular_weights or {}).items())
        return TreeWeights([r for r, _ in pairs], [w for _, w in pairs], len(rows))


class TreeWeights:
    """The weighted rows of a count table of ``n_rows`` rows as vk_cell_step_tree takes them:
    ``rows`` (int32, strictly ascending, in [0, n_rows)) and ``weights`` (float64 g/mol, finite,
    >= 0), at most 256 of them.  This is the host side's validation of ``rows[]``, which the C
    function trusts (include/vk_kinetics.h): anything else is a ValueError here, before any
    launch.  :meth:`upload` puts both on a device, once."""

    def __init__(self, rows, weights, n_rows):
        r64 = np.asarray(rows, dtype=np.int64).reshape(-1)
        self.weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        self.n_rows = int(n_rows)
        if r64.shape != self.weights.shape:
            raise ValueError('TreeWeights: one weight per row')
        if len(r64) > native.VK_TREE_MAX_WEIGHTED:
            raise ValueError('TreeWeights: at most %d weighted rows (got %d)' % (native.VK_TREE_MAX_WEIGHTED, len(r64)))
        if len(r64) and (r64.min() < 0 or r64.max() >= self.n_rows):
            raise ValueError('TreeWeights: every row must lie in [0, %d)' % self.n_rows)
        if np.any(np.diff(r64) <= 0):
            raise ValueError('TreeWeights: rows must be strictly ascending')
        if not np.all(np.isfinite(self.weights)) or np.any(self.weights < 0):
            raise ValueError('TreeWeights: weights must be finite and >= 0')
        self.rows = np.ascontiguousarray(r64.astype(np.int32))
        self.dev_rows = self.dev_weights = None

    def __len__(self):
        return len(self.rows)

    def pairs(self, counts):
        """(g/mol, counts[row]) in the fold's order, for CellModel.tree_mass / initial_rows;
        ``counts``: anything indexed by table row."""
        return [(float(w), counts[int(r)]) for r, w in zip(self.rows, self.weights)]

    def upload(self, device):
        import torch
        pad = lambda a: a if a.size else np.zeros(1, dtype=a.dtype)      # no null pointers
        self.dev_rows = torch.from_numpy(pad(self.rows)).to(device)
        self.dev_weights = torch.from_numpy(pad(self.weights)).to(device)
        return self


def cell_step_tree(p, n, ld, cell, m2c, u, root, depth, path, divide, counts, tree, initial_mass):
    """vk_cell_step_tree on the current stream (include/vk_kinetics.h): ``counts`` the int32
    [n_rows, ld_counts] table, ``tree`` an uploaded :class:`TreeWeights` of that table,
    ``initial_mass`` [ld] (the ``'tree_mass'`` model) or None.  Returns the status."""
    if tree.dev_rows is None:
        raise ValueError('cell_step_tree: TreeWeights.upload(device) first')
    if counts is not None and (counts.dim() != 2 or counts.shape[0] != tree.n_rows):
        raise ValueError('cell_step_tree: counts must be the [%d, ld] table the weights were bound to' % tree.n_rows)
    return native._lib.vk_cell_step_tree(
        ctypes.byref(p), int(n), int(ld), native.ptr(cell), native.ptr(m2c), native.ptr(u), native.ptr(root),
        native.ptr(depth), native.ptr(path), native.ptr(divide), native.ptr(counts),
        0 if counts is None else counts.shape[-1], tree.n_rows, native.ptr(tree.dev_rows),
        native.ptr(tree.dev_weights), len(tree), native.ptr(initial_mass), native.stream_handle())


def lineage_ids(roots, root, depth, path):
    """Phylogeny id strings (meta_division.py:15-18) from the lineage arrays."""
    out = []
    for r, d, p in zip(root.tolist(), depth.tolist(), path.tolist()):
        out.append(roots[r] + (format(p & ((1 << d) - 1), '0%db' % d) if d else ''))
    return out


def params_ref(p: native.VkCellParams):
    return ctypes.byref(p)
