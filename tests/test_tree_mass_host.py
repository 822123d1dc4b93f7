"""TreeMass over the count table and the ``set`` dividers, on the host: every refusal, the
weights helper against the fixtures, the initial deriver pass against the restatement
(tests/tree_mass_ref.py), the sorted binding, the population table's new row, and the ctypes
prototype against the header."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import tree_mass_ref as tref
from lens_amd import configs, native, population
from lens_amd.cells import CellModel, TreeWeights
from lens_amd.stochastic import StochasticModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')
FIX = {name: json.load(open(os.path.join(GOLDEN, 'flagella_%s.json' % name)))
       for name in ('transcription', 'translation', 'complexation', 'degradation', 'complex_weights')}
COMPLEXES = FIX['complex_weights']['molecular_weight']


def _table(**kw):
    return StochasticModel(['A', 'B', 'AB'], {'bind': {'A': -1, 'B': -1, 'AB': 1}}, {'bind': 0.01},
                           initial={'A': 40, 'B': 30, 'P': 7, 'Q': 0}, passive=['P', 'Q', 'R'], **kw)


# -- CellModel ------------------------------------------------------------------------------
@pytest.mark.parametrize('weights', [{'A': float('nan')}, {'A': float('inf')}, {'A': -1.0}, {'A': 'heavy'}, ['A']])
def test_a_bad_weight_is_refused(weights):
    with pytest.raises(ValueError, match='molecular_weights'):
        CellModel(molecular_weights=weights)


def test_weights_and_models():
    with pytest.raises(ValueError, match="model='growth'"):
        CellModel(model='growth', molecular_weights={'A': 1.0})
    for missing in (None, {}):
        with pytest.raises(ValueError, match='tree_mass'):
            CellModel(model='tree_mass', molecular_weights=missing)
    with pytest.raises(ValueError, match='at most 256'):
        CellModel(molecular_weights={'s%d' % i: 1.0 for i in range(257)})
    cm = CellModel(model='tree_mass', molecular_weights={'A': 0.0, 'B': 3})
    assert cm.molecular_weights == {'A': 0.0, 'B': 3.0} and cm.weighted       # a weight of 0.0 stays
    assert not CellModel().weighted and CellModel().molecular_weights is None
    assert cm.vk_params(1.0, 0).model == native.VK_GROWTH_TREE == 2
    assert CellModel(molecular_weights={'A': 1.0}).vk_params(1.0, 0).model == native.VK_GROWTH_PROTEIN


def test_binding_sorts_by_table_row():
    sm = _table()
    tree = CellModel(molecular_weights={'R': 5.0, 'A': 1.0, 'P': 0.0, 'AB': 2.5}).bind(sm)
    assert tree.rows.dtype == np.int32 and tree.rows.tolist() == [0, 2, 3, 5]
    assert tree.weights.tolist() == [1.0, 2.5, 0.0, 5.0] and tree.n_rows == 6 and len(tree) == 4
    assert tree.pairs(sm.initial) == [(1.0, 40), (2.5, 0), (0.0, 7), (5.0, 0)]
    with pytest.raises(ValueError, match="'Z'"):
        CellModel(molecular_weights={'A': 1.0, 'Z': 1.0}).bind(sm)


@pytest.mark.parametrize('rows,weights,n_rows', [
    ([0, 3], [1.0, 1.0], 3), ([-1, 1], [1.0, 1.0], 3), ([1, 1], [1.0, 1.0], 3), ([2, 1], [1.0, 1.0], 3),
    ([0], [1.0, 2.0], 3), ([0], [-1.0], 3), ([0], [float('nan')], 3), (list(range(257)), [1.0] * 257, 300)])
def test_tree_weights_validates_the_rows(rows, weights, n_rows):
    with pytest.raises(ValueError, match='TreeWeights'):
        TreeWeights(rows, weights, n_rows)


def test_tree_weights_at_the_limits():
    assert len(TreeWeights([], [], 0)) == 0
    assert len(TreeWeights(list(range(256)), [0.0] * 256, 256)) == 256


@pytest.mark.parametrize('model', ['tree_mass', 'growth_protein'])
def test_initial_rows_equal_the_restatement(model):
    sm = _table()
    cm = CellModel(model=model, initial_mass=1000.0, molecular_weights={'P': 3e9, 'A': 2e10, 'Q': 1e12})
    tree = cm.bind(sm)
    n = 3
    with pytest.raises(ValueError, match='weighted'):
        cm.initial_rows(n)
    rows, m2c = cm.initial_rows(n, weighted=tree.pairs(sm.initial))
    counts = sm.initial_counts(n, n)
    for a in range(n):
        bare = CellModel(initial_mass=1000.0)                     # the aggregate protein's node alone
        first = tref.F(1000.0) if model == 'tree_mass' else tref.F(bare.tree_mass(bare.initial_protein()))
        m = tref.fold(cm, first, tree.rows, tree.weights, counts[:, a])
        want = (m,) + tuple(tref.derive(cm, m)[i] for i in (0, 2, 3))
        assert tuple(rows[:4, a]) == want and m2c[a] == tref.derive(cm, m)[1]
        assert m > first                                          # the contents weigh something
    assert np.all(rows[native.VK_CELL_PROTEIN] == (0.0 if model == 'tree_mass' else cm.initial_protein()))
    # per-agent counts and per-agent initial masses
    rows2, _ = cm.initial_rows(2, mass=[10.0, 20.0], weighted=[(2e10, np.array([1, 2]))])
    if model == 'tree_mass':
        assert rows2[0, 0] == tref.fold(cm, 10.0, [0], [2e10], [1]) and rows2[0, 1] == tref.fold(cm, 20.0, [0], [2e10], [2])


def test_a_model_without_weights_is_what_it_was():
    cm = CellModel()
    rows, m2c = cm.initial_rows(2)
    p0 = cm.initial_protein()
    assert rows[0, 0] == 0.0 + (cm.protein_mw * (p0 / cm.avogadro)) * (1 / 1e-15) == cm.tree_mass(p0)
    g = CellModel(model='growth')
    assert g.initial_rows(2, mass=[5.0, 6.0])[0][0].tolist() == [5.0, 6.0]


# -- Colony's refusals (before anything is built: no device is touched) -----------------------
def test_colony_refuses_weights_without_a_table():
    from lens_amd.colony import Colony
    cm = CellModel(molecular_weights={'A': 1.0})
    with pytest.raises(ValueError, match='stochastic='):
        Colony(configs.glc_lct_config(), 2, cells=cm)
    with pytest.raises(ValueError, match="'Z'"):
        Colony(configs.glc_lct_config(), 2, cells=CellModel(molecular_weights={'Z': 1.0}), stochastic=_table())
    assert Colony.initial_mass is None and Colony._tree is None


# -- the population table -------------------------------------------------------------------
def test_population_table_has_the_initial_mass_row():
    table = dict(population._ALL_AGENT_ARRAYS)
    assert table['initial_mass'] == population._SPLIT == native.VK_DIVIDE_SPLIT
    assert ('initial_mass', population._SPLIT) in population.STOCHASTIC_ARRAYS
    from lens_amd.colony import Colony
    col = Colony.__new__(Colony)
    assert 'initial_mass' not in col.agent_array_names()          # only a tree_mass colony holds it
    col.initial_mass = torch.zeros(4, dtype=torch.float64)
    assert col.agent_array_names() == ['initial_mass']


# -- StochasticModel(dividers=) ---------------------------------------------------------------
def test_dividers_accepted_and_refused():
    sm = _table(dividers={'P': 'set', 'A': 'set', 'B': 'split', 'Q': 'set'})
    assert sm.dividers == {'P': 'set', 'A': 'set', 'B': 'split', 'Q': 'set'}
    assert sm.set_runs() == [(0, 1), (3, 5)]
    assert _table().dividers == {} and _table().set_runs() == []
    assert _table(dividers={'AB': 'set', 'P': 'set'}).set_runs() == [(2, 4)]       # across the passive edge
    with pytest.raises(ValueError, match='unknown row'):
        _table(dividers={'Z': 'set'})
    for bad in ('zero', 'SET', None, 0):
        with pytest.raises(ValueError, match='divider of'):
            _table(dividers={'A': bad})


def test_dividers_leave_the_packed_arrays_alone():
    from lens_amd.stochastic import _PACKED
    a, b = _table(), _table(dividers={'A': 'set', 'R': 'set'})
    for name in _PACKED + ('initial', 'matrix'):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert (a.rows, a.seed, a.max_events, a.max_order) == (b.rows, b.seed, b.max_events, b.max_order)


# -- configs -----------------------------------------------------------------------------------
def test_flagella_molecular_weights_against_the_fixtures():
    tl = FIX['translation']
    w = configs.flagella_molecular_weights(tl)
    products = {p for _, p in tl['transcripts']}
    assert w == {p: tl['molecular_weight'][p] for p in products} and len(w) == 49
    w = configs.flagella_molecular_weights(tl, complexes=COMPLEXES)
    assert len(w) == 54 and w['flagella'] == 8815743.0 and w['flhDC'] == 96396.0
    models = configs.flagella_gene_expression(*(FIX[k] for k in ('transcription', 'translation', 'complexation',
                                                                 'degradation')))
    tx, rows = models['transcription'], models['stochastic'].rows
    w = configs.flagella_molecular_weights(tl, tx, COMPLEXES)
    assert set(w) <= set(rows)
    for name in list(FIX['complexation']['monomer_ids']) + list(FIX['complexation']['complex_ids']):
        want = tl['molecular_weight'].get(name, COMPLEXES.get(name))
        assert w.get(name) == want, name                          # every protein and complex of the table
    # the reference's name collision: the operon's transcript weighs what the namesake weighs
    assert w['fliL_RNA'] == tl['molecular_weight']['fliL'] == w['fliL']
    assert w['flhDC_RNA'] == COMPLEXES['flhDC'] == w['flhDC']
    operons = {o for o, _ in tl['transcripts']}
    named = set(tl['molecular_weight']) | set(COMPLEXES)
    assert {k[:-4] for k in w if k.endswith('_RNA')} == operons & named
    assert 'flhDC_RNA' not in configs.flagella_molecular_weights(tl, tx)       # without the complexes' weights
    assert not any(k in w for k in configs.FLAGELLA_SET_DIVIDERS)


def test_gene_expression_cell_and_the_set_dividers():
    four = [FIX[k] for k in ('transcription', 'translation', 'complexation', 'degradation')]
    cm = configs.gene_expression_cell(FIX['translation'], complexes=COMPLEXES, division_volume=1.3)
    assert (cm.model, cm.initial_mass, cm.division_volume) == ('tree_mass', 1339.0, 1.3) and len(cm.molecular_weights) == 54
    assert configs.flagella_gene_expression(*four)['stochastic'].dividers == {}
    sm = configs.flagella_gene_expression(*four, set_dividers=True)['stochastic']
    assert sm.dividers == {name: 'set' for name in ('CpxR', 'CRP', 'Fnr', 'endoRNAse')}
    assert sum(hi - lo for lo, hi in sm.set_runs()) == 4
    kw = configs.chemotaxis_expression_flagella(*four, complexes=COMPLEXES, seed=3)
    assert set(kw) == {'stochastic', 'transcription', 'translation', 'degradation', 'cells', 'motility'}
    assert kw['stochastic'].dividers == sm.dividers and kw['stochastic'].n_rows == 77
    cells, motility = kw['cells'], kw['motility']
    assert (cells.model, cells.growth_rate, cells.initial_mass) == ('growth_protein', 0.000275, 1339.0)
    assert set(cells.molecular_weights) <= set(kw['stochastic'].rows) and 'flhDC_RNA' in cells.molecular_weights
    assert len(cells.bind(kw['stochastic'])) == len(cells.molecular_weights)
    assert (motility.ligand_id, motility.initial_ligand, motility.division, motility.seed) == ('MeAsp', 0.1, 'merged', 3)
    assert motility.flagella.complexes == 'flagella'


# -- the boundary ------------------------------------------------------------------------------
def test_the_prototype_matches_the_header():
    text = open(os.path.join(REPO, 'include', 'vk_kinetics.h')).read()
    decl = re.search(r'^int vk_cell_step_tree\((.*?)\);', text, re.M | re.S).group(1)
    args = [' '.join(a.split()) for a in decl.split(',')]
    kinds = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'vk_stream_t': ctypes.c_void_p}
    want = []
    for a in args:
        if a.startswith('const vk_cell_params *'):
            want.append(ctypes.POINTER(native.VkCellParams))
        elif '*' in a:
            want.append(ctypes.c_void_p)
        else:
            want.append(kinds[a.split()[0]])
    got, res = native._SIGS['vk_cell_step_tree']
    assert got == want and len(got) == 18 and res is ctypes.c_int
    assert 'vk_cell_step_tree' in native.EXPORTS
    assert re.search(r'VK_GROWTH_TREE = 2\b', text) and re.search(r'#define VK_TREE_MAX_WEIGHTED 256\b', text)
    assert native.VK_TREE_MAX_WEIGHTED == 256
