"""Colony(cells=CellModel(molecular_weights=...), stochastic=...): the cell rows, mmol_to_counts,
``initial_mass``, the counts and the keys against a restated loop (tests/ssa_ref.py ->
tests/tree_mass_ref.py -> the dividers over the division the restated flags ask for) at every one
of 30 steps, and the whole flagella chromosome with the reference's cells.

The toy colony: 24 agents, capacity 26 (the first division outgrows it), a birth network
X (50 / s) -> Y with the passive rows E (``set`` divider) and Z.  The synthetic weights make one X
0.2 fg, so a cell gains about 10 fg / s.  In the tree model agent a starts from 1000 + 10 a fg
(set_cell_mass) and DivisionVolume asks for 1400 fg: agent 23 divides after 16 s, agent 0 not
within 30 s, and a daughter (half the initial mass, half the X) never again.  The seed was chosen
on the CPU so that no agent's time margin falls below 1e-9 (asserted on the restatement alone)."""

import json
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import ssa_ref as sref
import tree_mass_ref as tref
from lens_amd import configs, native
from lens_amd.cells import CellModel
from lens_amd.stochastic import StochasticModel, passive_seed

pytestmark = pytest.mark.gpu

N, CAP, STEPS, SEED = 24, 26, 30, 20261021
WEIGHTS = {'Z': 6.0e8, 'X': 1.2044e8, 'E': 0.0, 'Y': 2.4e8}      # given out of table order
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    native.load()
    return torch.device('cuda', 0)


def _network(dividers=True):
    return StochasticModel(['X', 'Y'], {'birth': {'X': 1}, 'ripen': {'X': -1, 'Y': 1}}, {'birth': 50.0, 'ripen': 0.01},
                           initial={'Z': 4}, seed=SEED + 2, passive=['E', 'Z'],
                           dividers={'E': 'set'} if dividers else None)


def _cells(model, weights=WEIGHTS):
    if model == 'tree_mass':
        return CellModel(model='tree_mass', division_volume=1400.0 / 1100.0, molecular_weights=weights)
    return CellModel(rng='philox', growth_rate=0.05, seed=SEED + 1, molecular_weights=weights)


def _enzymes(n):
    return (3 + 2 * np.arange(n)).astype(np.int32)               # odd and her own: a split would show


class Loop:
    """The restated colony: counts, keys, cell rows, m2c, initial_mass and the lineage."""

    def __init__(self, sm, cm, n):
        self.sm, self.cm, self.n, self.step_index, self.key_base = sm, cm, n, 0, n
        self.tree = cm.bind(sm) if cm.weighted else None
        self.rows, self.weights = (self.tree.rows, self.tree.weights) if cm.weighted else ([], [])
        self.x = sm.initial_counts(n, n)
        self.x[sm.index('E')] = _enzymes(n)
        self.keys = np.arange(n, dtype=np.int64)
        self.status = np.zeros(n, dtype=np.int32)
        self.root, self.depth, self.path = np.arange(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        self.initial_mass = np.full(n, float(cm.initial_mass))
        self.cell = np.zeros((native.VK_CELL_ROWS, n))
        self.m2c = np.zeros(n)
        self.divisions, self.min_margin, self.halved = [], np.inf, 0
        self.derive_all(cm.initial_protein() if cm.model == 'growth_protein' else 0.0)

    def derive_all(self, protein=None):
        """The initial deriver pass / set_cell_mass: TreeMass and DeriveGlobals on what there is."""
        cm = self.cm
        for a in range(self.n):
            if protein is not None:
                self.cell[native.VK_CELL_PROTEIN, a] = protein
            first = self.initial_mass[a] if cm.model == 'tree_mass' else cm.tree_mass(self.cell[native.VK_CELL_PROTEIN, a])
            m = tref.fold(cm, first, self.rows, self.weights, self.x[:, a])
            v, mc, length, area = tref.derive(cm, m)
            self.cell[:4, a], self.m2c[a] = (m, v, length, area), mc

    def step(self):
        sm, S, step = self.sm, self.sm.n_species, self.step_index
        events, self.status, margin = sref.step(sm, self.x[:S], self.keys, 1.0, sm.seed, step, status=self.status)
        self.min_margin = min(self.min_margin, float(margin.min()))
        assert not self.status.any()
        div = tref.cell_step(self.cm, 1.0, step, self.n, self.cell, self.m2c, self.x, self.rows, self.weights,
                             lineage=(self.root, self.depth, self.path), initial_mass=self.initial_mass)
        if div.any():
            src, kind, n_keep = tref.plan(div)
            x = self.x
            active, keys = sref.divide_counts(x[:S], self.keys, src, kind, n_keep, sm.seed, step, self.key_base)
            passive, _ = sref.divide_counts(x[S:], self.keys, src, kind, n_keep, passive_seed(sm.seed, 0), step,
                                            self.key_base)
            self.x = tref.set_rows(np.concatenate([active, passive]), x, src,
                                   [r for lo, hi in sm.set_runs() for r in range(lo, hi)])
            self.keys = keys
            self.key_base += len(src) - n_keep
            A = native.VK_CELL_ANGLE
            self.cell = np.concatenate([tref.divide_float(self.cell[:A], src, kind, True),
                                        tref.divide_float(self.cell[A:], src, kind, False)])
            self.m2c = tref.divide_float(self.m2c, src, kind, False)
            self.initial_mass = tref.divide_float(self.initial_mass, src, kind, True)
            d = kind >= 0
            self.root, self.depth, self.path = self.root[src], self.depth[src] + d, np.where(
                d, self.path[src] * 2 + np.maximum(kind, 0), self.path[src])
            self.n = len(src)
            self.status = np.zeros(self.n, dtype=np.int32)
            self.divisions.append((step, int(d.sum()) // 2))
            # a daughter carries half the mother's mass, not the fold of her own counts
            j = int(np.nonzero(d)[0][0])
            own = self.initial_mass[j] if self.cm.model == 'tree_mass' else self.cm.tree_mass(self.cell[A - 1, j])
            self.halved += self.cell[0, j] != tref.fold(self.cm, own, self.rows, self.weights, self.x[:, j])
        self.step_index += 1


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(col, loop, where):
    n = loop.n
    assert col.n == n, where
    got = {'cell': col.cell, 'm2c': col.m2c, 'ssa': col.ssa, 'ssa_key': col.ssa_key}
    want = {'cell': loop.cell, 'm2c': loop.m2c, 'ssa': loop.x, 'ssa_key': loop.keys}
    if loop.cm.model == 'tree_mass':
        got['initial_mass'], want['initial_mass'] = col.initial_mass, loop.initial_mass
    for name in got:
        g = got[name][..., :n].cpu().numpy()
        assert g.dtype == want[name].dtype and np.array_equal(_bits(g), _bits(want[name])), (where, name)


def _colony(dev, sm, cm, n=N, capacity=CAP):
    from lens_amd.colony import Colony
    col = Colony(configs.toy_config(), n, capacity=capacity, device=dev, integrator='euler', cells=cm,
                 agent_ids=['c%d.' % i for i in range(n)], stochastic=sm)
    col.ssa[sm.index('E'), :n] = torch.from_numpy(_enzymes(n)).to(dev)
    return col


def _start(model):
    sm, cm = _network(), _cells(model)
    loop = Loop(sm, cm, N)
    masses = 1000.0 + 10.0 * np.arange(N)
    if model == 'tree_mass':
        loop.initial_mass = masses.copy()
        loop.derive_all()
    return sm, cm, loop, masses


@pytest.mark.parametrize('model', ['tree_mass', 'growth_protein'])
def test_colony_equals_the_restated_loop(dev, model):
    sm, cm, loop, masses = _start(model)
    col = _colony(dev, sm, cm)
    assert (col._tree is not None) and (col.initial_mass is not None) == (model == 'tree_mass')
    assert ('initial_mass' in col.agent_array_names()) == (model == 'tree_mass')
    if model == 'tree_mass':
        # the constructor's deriver pass saw E = 0 and Z = 4; set_cell_mass folds the counts as they are now
        col.set_cell_mass(masses)
    _same(col, loop, 'start')                                    # (E weighs 0.0: GrowthProtein's start is the constructor's)
    for step in range(STEPS):
        col.step(1.0)
        loop.step()
        torch.cuda.synchronize()
        _same(col, loop, step)
    col.check_status()
    assert loop.min_margin >= sref.MARGIN                        # nobody is left out with this seed
    assert col.ld > CAP and len(loop.divisions) >= 1 and loop.halved >= 1   # the capacity grew on the way
    mothers = sum(k for _, k in loop.divisions)
    assert col.n == N + mothers
    if model == 'tree_mass':
        assert 0 < mothers < N and len(loop.divisions) >= 3      # some cells, not all, over several steps
        # remove keeps initial_mass with its agent
        mask = torch.zeros(col.n, dtype=torch.int32, device=dev)
        mask[1::3] = 1
        keep = np.nonzero(mask.cpu().numpy() == 0)[0]
        assert col.remove(mask) == len(mask) - len(keep) and col.n == len(keep)
        assert np.array_equal(_bits(col.initial_mass[:col.n].cpu().numpy()), _bits(loop.initial_mass[keep]))
        assert np.array_equal(col.ssa[:, :col.n].cpu().numpy(), loop.x[:, keep])
        assert col.snapshot()['global']['mass'].tolist() == loop.cell[0, keep].tolist()
    with pytest.raises(ValueError, match='sort_by_bin'):
        col.sort_by_bin()                                        # a colony with cells keeps its order


def test_a_colony_without_weights_launches_what_it_did(dev):
    """No weights: vk_cell_step, and the present formula -- the aggregate protein alone."""
    sm = _network()
    cm = CellModel(rng='philox', growth_rate=0.05, seed=SEED + 1)
    col, loop = _colony(dev, sm, cm), Loop(sm, cm, N)
    assert col._tree is None and col.initial_mass is None and loop.rows == []
    _same(col, loop, 'start')
    for step in range(STEPS):
        col.step(1.0)
        loop.step()
        torch.cuda.synchronize()
        _same(col, loop, step)
    assert len(loop.divisions) >= 1 and col.n >= 2 * N
    m = col.snapshot()['global']['mass']
    p = col.cell[native.VK_CELL_PROTEIN, :col.n].cpu().numpy()
    assert m.tolist() == [0.0 + (cm.protein_mw * (x / cm.avogadro)) * (1 / 1e-15) for x in p.tolist()]


def test_refusals(dev):
    from lens_amd.colony import Colony
    with pytest.raises(ValueError, match='stochastic='):
        Colony(configs.toy_config(), 4, device=dev, integrator='euler', cells=_cells('tree_mass'))
    with pytest.raises(ValueError, match="'nothing'"):
        _colony(dev, _network(), _cells('tree_mass', {'nothing': 1.0}))
    col = _colony(dev, _network(), _cells('tree_mass'))
    with pytest.raises(ValueError):
        col.capture(1.0)                                         # steps with cells stay refused
    with pytest.raises(ValueError, match='one initial mass per agent'):
        col.set_cell_mass(np.ones(3))


# -- the whole flagella chromosome -------------------------------------------------------------
def _golden(name):
    with open(os.path.join(GOLDEN, 'flagella_%s.json' % name)) as f:
        return json.load(f)


def _fixtures():
    return [_golden(k) for k in ('transcription', 'translation', 'complexation', 'degradation')]


SET_ROWS = ('CpxR', 'CRP', 'Fnr', 'endoRNAse')
CHROMOSOME_STEPS = 30              # of 1 s: at 22 residues / s the shorter proteins are finished


def _place(col, sm, deg, n):
    """The pools; regulators and RNases of her own for every agent (odd counts: a split would
    show); and what lets proteins and complexes appear within the run: 3 of every transcript, flhD
    and flhC for ten flhDC.  10 free ribosomes and RNA polymerases cannot fill the 16 slots."""
    pools = deg['initial_state']['molecules']
    col.set_transcription_molecules(**{m: pools[m] for m in col.transcription.molecule_ids if m in pools})
    col.set_translation_molecules(**{m: pools[m] for m in col.translation.molecule_ids if m in pools})
    own = {}
    for k, name in enumerate(SET_ROWS):
        own[name] = (11 + 2 * np.arange(n) + 1000 * k if name != 'endoRNAse' else 1 + 2 * (np.arange(n) % 2)).astype(np.int32)
        col.ssa[sm.index(name), :n] = torch.from_numpy(own[name]).to(col.device)
    for name in col.transcription.products:
        col.ssa[sm.index(name), :n] = 3
    for name, count in (('flhD', 40), ('flhC', 20), ('Ribosome', 10), ('RNA Polymerase', 10)):
        col.ssa[sm.index(name), :n] = count
    return own


def _expressed(col, sm, tl):
    """(translated proteins other than the placed flhD / flhC, flhDC complexes) over the colony."""
    x = col.ssa[:, :col.n].cpu().numpy().astype(np.int64)
    proteins = sorted({p for _, p in tl['transcripts']} - {'flhD', 'flhC'})
    return int(x[[sm.index(p) for p in proteins]].sum()), int(x[sm.index('flhDC')].sum())


def _daughters_keep(col, sm, own, mothers, n):
    """Survivors in order, then the daughters in mother order: both hold the mother's set rows."""
    keep = [a for a in range(n) if a not in mothers]
    src = keep + [a for a in mothers for _ in (0, 1)]
    assert col.n == len(src)
    for name in SET_ROWS:
        assert col.ssa[sm.index(name), :col.n].cpu().numpy().tolist() == own[name][src].tolist(), name
    return src


def test_gene_expression_cell_on_the_whole_chromosome(dev):
    from lens_amd.colony import Colony
    tx, tl, cx, deg = _fixtures()
    cfg = configs.flagella_gene_expression(tx, tl, cx, deg, max_rnaps=16, max_ribosomes=16, set_dividers=True)
    sm = cfg['stochastic']
    cm = configs.gene_expression_cell(tl, cfg['transcription'], _golden('complex_weights')['molecular_weight'])
    n, mothers = 65, [3, 40, 64]
    col = Colony(configs.glc_lct_config(), n, device=dev, environment='held', cells=cm, **cfg)
    assert col.ssa.shape[0] == 77 and len(col._tree) == len(cm.molecular_weights) == 69
    masses = np.full(n, 1339.0)
    masses[mothers] = 3 * 1339.0                                 # 3.65 fL at the start of step one: they divide
    col.set_cell_mass(masses)

    def folded():
        x = col.ssa[:, :col.n].cpu().numpy()
        im = col.initial_mass[:col.n].cpu().numpy()
        return np.asarray(cm.tree_mass(None, col._tree.pairs(x), im)).tolist()      # numpy: elementwise

    # how little the contents weigh: the initial state's 8 flagella, 0.117 fg on 1339 fg
    assert float(col.cell[0, 0]) - 1339.0 == pytest.approx(8 * 8815743.0 / cm.avogadro * 1e15, rel=1e-6)
    own = _place(col, sm, deg, n)
    col.set_cell_mass(masses)
    assert col.snapshot()['global']['mass'].tolist() == folded()
    col.step(1.0)
    torch.cuda.synchronize()
    src = _daughters_keep(col, sm, own, mothers, n)
    mass, want = col.snapshot()['global']['mass'], folded()
    assert mass[:n - 3].tolist() == want[:n - 3]                 # every survivor: the fold over her own counts
    assert col.initial_mass[n - 3:col.n].cpu().numpy().tolist() == [1.5 * 1339.0] * 6
    assert mass[n - 3::2].tolist() == mass[n - 2::2].tolist() and np.all(mass[n - 3:] > 1.5 * 1339.0)
    for step in range(1, CHROMOSOME_STEPS):
        col.step(1.0)
        torch.cuda.synchronize()
        # the daughters' too, and after transcription, translation, degradation and the network
        assert col.n == n + 3 and col.snapshot()['global']['mass'].tolist() == folded(), step
    col.check_status()
    proteins, complexes = _expressed(col, sm, tl)
    print('gene_expression_cell: translated proteins', proteins, 'flhDC', complexes)
    assert proteins > 0 and complexes > 0                        # the fold saw proteins and complexes appear


def test_chemotaxis_expression_flagella_on_the_whole_chromosome(dev):
    from lens_amd.colony import Colony
    from test_ssa_colony_gpu import BOUNDS, _lattice
    tx, tl, cx, deg = _fixtures()
    kw = configs.chemotaxis_expression_flagella(tx, tl, cx, deg, complexes=_golden('complex_weights')['molecular_weight'],
                                                expression=dict(max_rnaps=16, max_ribosomes=16), seed=SEED)
    sm, cm = kw['stochastic'], kw['cells']
    cm.rng, cm.seed = 'philox', SEED + 1
    n, mothers = 65, [0, 31]
    col = Colony(configs.glc_lct_config(), n, device=dev, environment=_lattice(dev, ('glc__D_e', 'lcts_e', 'MeAsp')), **kw)
    col.set_agents(location=np.random.default_rng(SEED).uniform(0.0, BOUNDS[0], (2, n)))
    col.gather_external()
    own = _place(col, sm, deg, n)
    P = native.VK_CELL_PROTEIN
    col.cell[P, mothers] = 2 * cm.initial_protein()              # GrowthProtein's own condition: they divide

    def folded():
        x = col.ssa[:, :col.n].cpu().numpy()
        p = col.cell[P, :col.n].cpu().numpy()
        return np.asarray(cm.tree_mass(p, col._tree.pairs(x))).tolist()                # numpy: elementwise

    col.step(1.0)
    torch.cuda.synchronize()
    _daughters_keep(col, sm, own, mothers, n)
    mass = col.snapshot()['global']['mass']
    assert mass[:n - 2].tolist() == folded()[:n - 2]
    for step in range(1, CHROMOSOME_STEPS):
        col.step(1.0)
        torch.cuda.synchronize()
        assert col.n == n + 2 and col.snapshot()['global']['mass'].tolist() == folded(), step
    proteins, complexes = _expressed(col, sm, tl)
    print('chemotaxis_expression_flagella: translated proteins', proteins, 'flhDC', complexes)
    assert proteins > 0 and complexes > 0
    bare = CellModel(rng='philox')
    assert all(m > bare.tree_mass(p) for m, p in zip(folded(), col.cell[P, :col.n].cpu().numpy().tolist()))
    col.check_status()
