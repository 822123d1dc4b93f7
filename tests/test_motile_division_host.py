"""The restatement of motile division (tests/motile_division_ref.py) on the CPU: the
reference's dividers written out with Python dicts, the bitmask forms against them, the
int split, the keys, the reference's default expression rates, and the models' refusals."""

import copy

import numpy as np
import pytest

from oracle.colony import philox_uniform

import motile_division_ref as ref

FI = ref.FI


# -- the reference's behaviour, literally ------------------------------------------------

def split_dict(state):
    """divide_split_dict (vivarium/core/registry.py:246-262)."""
    items = list((state or {}).items())
    return [dict(items[len(items) // 2:]), dict(items[:len(items) // 2])]


def deep_merge(dct, merge_dct):
    """vivarium/library/dict_utils.py:51-66: recursive, in place, only adds or overwrites."""
    for k, v in merge_dct.items():
        if k in dct and isinstance(dct[k], dict) and isinstance(v, dict):
            deep_merge(dct[k], v)
        else:
            dct[k] = v
    return dct


def store_divide(mother):
    """What Store.apply_update hands the daughters (core/experiment.py:664-697): ONE deep
    copy of the mother, into which each daughter's divided values are merged in turn."""
    initial_state = copy.deepcopy(mother)
    divided = split_dict(mother['flagella'])
    out = []
    for state in divided:
        initial_state = deep_merge(initial_state, {'flagella': state})
        out.append(copy.deepcopy(initial_state))      # set_value copies the leaves into the daughter's stores
    return out


def _flagella(n, rng):
    return {'flagellum_%02d' % i: int(rng.choice([-1, 1])) for i in range(n)}     # 1: CW


def _mask(flagella):
    return sum(1 << i for i, v in enumerate(flagella.values()) if v == 1)


def _as_i32(mask):
    return np.array([mask], dtype=np.uint32).view(np.int32)


@pytest.mark.parametrize('n', [0, 1, 2, 5, 32])
def test_split_dict_and_its_bitmask_form(n):
    rng = np.random.default_rng(n)
    f = _flagella(n, rng)
    d0, d1 = split_dict(f)
    assert list(d0) == list(f)[n // 2:] and list(d1) == list(f)[:n // 2]
    assert len(d0) + len(d1) == n and not set(d0) & set(d1)
    (h0, m0), (h1, m1) = ref.divide_have_mask([n], _as_i32(_mask(f)), ref.SPLIT_DICT)
    assert (int(h0[0]), int(m0.view(np.uint32)[0])) == (len(d0), _mask(d0))
    assert (int(h1[0]), int(m1.view(np.uint32)[0])) == (len(d1), _mask(d1))
    for h, m in ((h0, m0), (h1, m1)):                  # no bit at or above have
        assert int(m.view(np.uint32)[0]) >> int(h[0]) == 0


@pytest.mark.parametrize('n', [0, 1, 2, 5, 32])
def test_the_store_hands_both_daughters_every_flagellum(n):
    """deep_merge into a copy of the mother neutralises split_dict: the union."""
    rng = np.random.default_rng(100 + n)
    mother = {'flagella': _flagella(n, rng), 'proteins': {'flagella': n}}
    a, b = store_divide(mother)
    assert a['flagella'] == mother['flagella'] and b['flagella'] == mother['flagella']
    (h0, m0), (h1, m1) = ref.divide_have_mask([n], _as_i32(_mask(mother['flagella'])), ref.MERGED)
    for h, m in ((h0, m0), (h1, m1)):
        assert int(h[0]) == n and int(m.view(np.uint32)[0]) == _mask(mother['flagella'])


def test_stored_garbage_is_read_as_the_motor_reads_it():
    """split_dict on have / mask outside the invariant: have clamped into 0..32, bits at and
    above it dropped first."""
    (h0, m0), (h1, m1) = ref.divide_have_mask([40, -3, 5], np.array([-1, -1, -1], dtype=np.int32), ref.SPLIT_DICT)
    assert h0.tolist() == [16, 0, 3] and h1.tolist() == [16, 0, 2]
    assert m0.view(np.uint32).tolist() == [0xFFFF, 0, 0b111] and m1.view(np.uint32).tolist() == [0xFFFF, 0, 0b11]


def test_int_split_conserves_and_follows_the_coin():
    t = np.arange(0, 33)
    for u in (0.0, 0.25, np.nextafter(0.5, 0.0), 0.5, 0.75):
        a, b = ref.split_int(t, np.full(t.shape, u))
        assert np.array_equal(a + b, t)
        assert np.array_equal(np.minimum(a, b), t // 2)
        odd = t % 2 == 1
        assert np.array_equal(a[odd] > b[odd], np.full(odd.sum(), u < 0.5))
        assert np.array_equal(a[~odd], b[~odd])


def test_the_split_draw_is_its_own():
    """Keyed by the mother's lineage under a seed of its own domain: not the growth draw of
    the same lineage and step, not the coarse switch's draw (s, k, 0) of an agent whose key
    equals the root of a mother with depth 0 and path 0."""
    seed, step, root = 11, 14, 3
    u = ref.divide_draw(seed, step, root, 0, 0)
    assert u == philox_uniform(seed ^ ref.DOMAIN, step, root, 0, 0)
    assert u != philox_uniform(seed, step, root, 0, 0)
    assert ref.divide_draw(seed, step, root, 1, 0b1) != ref.divide_draw(seed, step, root, 1, 0b0)
    assert 0.0 <= u < 1.0


def test_fresh_keys_over_three_generations():
    """Every key ever handed out is distinct; a survivor keeps hers."""
    rng = np.random.default_rng(3)
    n, keys, key_base = 5, np.arange(5), 5
    seen = set(keys.tolist())
    lineage = (np.arange(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64))
    for generation in range(3):
        div = rng.random(n) < 0.6
        div[0] = True
        keep, moth = np.flatnonzero(~div), np.flatnonzero(div)
        order = np.concatenate([keep, np.repeat(moth, 2)])
        flag_int = np.stack([rng.integers(0, 33, n), rng.integers(0, 33, n), np.zeros(n, dtype=np.int64)]).astype(np.int32)
        out, new = ref.divide_flagella(flag_int, keys, order, len(keep), ref.MERGED, 7, generation, lineage, key_base)
        assert np.array_equal(new[:len(keep)], keys[keep])
        fresh = new[len(keep):].tolist()
        assert len(set(fresh)) == len(fresh) == 2 * len(moth) and not seen & set(fresh)
        assert fresh == list(range(key_base, key_base + len(fresh)))
        assert np.array_equal(out[FI['target'], len(keep)::2] + out[FI['target'], len(keep) + 1::2],
                              flag_int[FI['target'], moth])
        seen |= set(fresh)
        key_base += len(fresh)
        daughter = np.arange(len(order)) >= len(keep)
        k = np.where(daughter, (np.arange(len(order)) - len(keep)) % 2, 0)
        lineage = (lineage[0][order], lineage[1][order] + daughter, np.where(daughter, lineage[2][order] * 2 + k,
                                                                             lineage[2][order]))
        keys, n = new, len(order)
    assert len(set(keys.tolist())) == n and n > 5


def test_counts_deriver_truncates_clamps_and_flags():
    m2c = 7.3e5
    conc = np.array([0.0, 0.999 / m2c, 5.5 / m2c, -0.5 / m2c, -2.0 / m2c, 32.9 / m2c, 33.5 / m2c, 1e9, np.nan])
    t, flag = ref.flagella_counts(conc, np.full(conc.shape, m2c))
    assert t.tolist() == [0, 0, 5, 0, 0, 32, 32, 32, 0] and flag and t.dtype == np.int32
    for inside in ([0.0, 5.5 / m2c, 32.9 / m2c], [-0.0]):
        assert not ref.flagella_counts(np.array(inside), np.full(len(inside), m2c))[1]
    for outside in (-0.5 / m2c, 33.5 / m2c, np.nan):
        assert ref.flagella_counts(np.array([outside]), np.array([m2c]))[1]


def test_the_reference_rates_through_one_cell_cycle():
    """get_flagella_expression's rates through a 2520-s cycle of GrowthProtein at its default
    rate, in the step order of the colony.  The transcript settles at rate / degradation =
    5e-5 mM and the protein then gains 8e-5 * 5e-5 = 4e-9 mM/s: 9.88e-6 mM after the cycle.
    That is 7.24 flagella at the initial mmol_to_counts and 14.48 at the doubled cell's, and
    2.02 after 630 s -- what the reference's own comment expects ("a cell cycle of 2520 sec
    is expected to express 8 flagella.  2 flagella expected in 630 seconds.",
    chemotaxis_flagella.py:485-486).  So the default rates do grow flagella; an estimate of
    1e-8 mM (count 0 for the whole cycle) drops a factor of 1000."""
    from lens_amd import configs
    from lens_amd.cells import CellModel
    from lens_amd.motility import FlagellaModel
    fm = FlagellaModel(0, expression=configs.flagella_expression())
    cm = CellModel()
    expr = fm.expression_initial[:, None].copy()
    mass = cm.initial_mass
    m2c0 = m2c = cm.derive(mass)[1]
    factor = float(np.exp(cm.growth_rate * 1.0))
    counts = []
    for step in range(2520):
        expr = ref.expression_step(fm.expression_table, expr, 1.0)
        t, flag = ref.flagella_counts(expr[fm.count_row], np.array([m2c]))
        assert not flag
        counts.append(int(t[0]))
        mass *= factor                                   # DeriveGlobals runs after the counts deriver
        m2c = cm.derive(mass)[1]
    protein = float(expr[fm.count_row, 0])
    print('flag_RNA %.6e mM, flagella %.6e mM, counts at 630 s %d, at 2520 s %d' % (expr[0, 0], protein, counts[629],
                                                                                 counts[-1]))
    assert abs(expr[0, 0] - 5e-5) < 1e-9 and abs(protein - 9.88e-6) < 1e-8
    assert counts[0] == 0 and counts[629] == 2 and counts[-1] == 14
    assert int(protein * m2c0) == 7                      # at constant volume: the comment's "8 flagella"
    assert counts == sorted(counts) and set(range(15)) == set(counts)
    assert 1.99 < mass / cm.initial_mass < 2.01


def test_expression_step_is_the_oracles():
    """The restatement's expression update against oracle.expression.next_update."""
    from oracle import expression as oe
    from lens_amd import configs
    from lens_amd.motility import FlagellaModel
    cfg = configs.flagella_expression()
    cfg['transcription_rates']['flag_RNA'] = 1.25e-4
    fm = FlagellaModel(0, expression=cfg)
    expr = np.array([[6.5e-3], [2.5e-6]])
    new = ref.expression_step(fm.expression_table, expr, 1.0)
    upd = oe.next_update(cfg, 1.0, {'internal': {'flag_RNA': 6.5e-3, 'flagella': 2.5e-6}})['internal']
    assert new[0, 0] == 6.5e-3 + upd['flag_RNA'] and new[1, 0] == 2.5e-6 + upd['flagella']


def test_whole_colony_restatement_divides_and_sheds():
    """The loop the GPU test compares against, on its own: the population quadruples, keys
    stay distinct, the count climbs through 0..8 before the first division, both modes agree
    until it, and a 'merged' daughter sheds her surplus in her first inner update."""
    runs = {}
    for mode in (ref.MERGED, ref.SPLIT_DICT):
        c = ref.MotileColony(*ref.colony_case(mode))
        field = np.zeros((16, 16))
        hist, margins = [], {}
        for step in range(30):
            before = c.flag_int.copy()
            mothers = c.step(field, 1.0, margins)
            hist.append((c.n, mothers, c.flag_int.copy(), before))
        assert all(v >= 1e-9 for v in margins.values()) and 'split' in margins, margins
        assert c.n >= 3 * 24 and len(set(c.keys.tolist())) == c.n and not c.flagged
        runs[mode] = hist
    first = next(s for s, h in enumerate(runs[ref.MERGED]) if h[1])
    seen = {int(t) for h in runs[ref.MERGED][:first] for t in h[2][FI['target']]}
    assert set(range(9)) <= seen
    for s in range(first):
        assert np.array_equal(runs[ref.MERGED][s][2], runs[ref.SPLIT_DICT][s][2])
    n_keep = 2 * runs[ref.MERGED][first - 1][0] - runs[ref.MERGED][first][0]
    after, mother = runs[ref.MERGED][first][2], runs[ref.MERGED][first][3]
    assert (after[FI['have'], n_keep:] > after[FI['target'], n_keep:]).all()       # every flagellum of the mother
    assert (runs[ref.SPLIT_DICT][first][2][FI['have'], n_keep:] < mother[FI['have']].max()).all()
    # her first motility launch after the division: have falls to the split target
    assert np.array_equal(runs[ref.MERGED][first + 1][2][FI['have']], after[FI['target']])


def test_model_checks():
    from lens_amd import configs
    from lens_amd.motility import FlagellaModel, MotilityModel
    with pytest.raises(ValueError, match='division'):
        MotilityModel(division='halves')
    for mode in (None, 'merged', 'split_dict'):
        assert MotilityModel(division=mode).division == mode
    e = configs.flagella_expression()
    with pytest.raises(ValueError, match='internal port'):
        FlagellaModel(0, expression=dict(e, regulators=[('external', 'glc__D_e')]))
    with pytest.raises(ValueError, match='not a state row'):
        FlagellaModel(0, expression=dict(e, regulation={'flag_RNA': 'if (external, glc__D_e) > 0.1'}))
    with pytest.raises(ValueError, match='transcription_leak'):
        FlagellaModel(0, expression=dict(e, transcription_leak={'rate': 0.01, 'magnitude': 1e-6}))
    with pytest.raises(ValueError, match='count_of'):
        FlagellaModel(0, expression=e, count_of='pili')
    ok = FlagellaModel(0, expression=dict(e, regulators=[('internal', 'flagella')],
                                          regulation={'flag_RNA': 'if (internal, flagella) > 1.0'},
                                          transcription_leak={'rate': 0.0, 'magnitude': 0.0}))
    assert ok.expression_names == ['flag_RNA', 'flagella'] and ok.count_row == 1
    assert FlagellaModel(5).expression is None
    # the count is derived: set_flagella refuses before it touches the device
    import types
    from lens_amd.colony import Colony
    with pytest.raises(ValueError, match='derived'):
        Colony.set_flagella(types.SimpleNamespace(motility=MotilityModel(flagella=ok)), 3)
    both = configs.chemotaxis_ode_expression_flagella(substeps=10)
    assert both['cells'].growth_rate == 0.000275 and both['cells'].initial_mass == 1339.0
    m = both['motility']
    assert (m.ligand_id, m.initial_ligand, m.division, m.substeps) == ('MeAsp', 1e-2, 'merged', 10)
    assert m.flagella.counts(3).tolist() == [0, 0, 0] and m.flagella.expression == configs.flagella_expression()
