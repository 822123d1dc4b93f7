"""RNA degradation and passive rows on the host: what DegradationModel, StochasticModel(passive=),
TranscriptionModel.product_sequences, the configs and the population table accept and refuse, and
the restatement (tests/degradation_ref.py) on the reference's toy.  No GPU."""

import copy
import json
import os

import numpy as np
import pytest

import degradation_ref as dref
import transcription_ref as xref

from lens_amd import configs, population
from lens_amd.degradation import KM_TO_MM, DegradationModel
from lens_amd.stochastic import MAX_PASSIVE, StochasticModel

KM = 1e-23


def _golden(name):
    with open(os.path.join(dref.GOLDEN, name)) as f:
        return json.load(f)


def _config(**change):
    data = copy.deepcopy(dref.toy_data())
    cfg = {k: data[k] for k in ('sequences', 'catalytic_rates', 'michaelis_constants')}
    cfg.update(change)
    return cfg


# -- DegradationModel -----------------------------------------------------------------------
def test_model_orders_and_packing():
    m = DegradationModel(**_config())
    assert m.transcript_order == ['oA', 'oAZ', 'oB', 'oBY'] and m.enzyme_order == ['endoRNAse']
    assert m.species() == ['oA', 'oAZ', 'oB', 'oBY', 'endoRNAse']
    assert m.molecule_ids == ['ATP', 'GTP', 'UTP', 'CTP', 'ADP'] and (m.atp_row, m.adp_row) == (0, 4)
    # GCC: 1 G, 2 C; AGUUGACGG: 2 A, 4 G, 2 U, 1 C
    assert m.composition[0].tolist() == [0, 1, 0, 2] and m.composition[3].tolist() == [2, 4, 2, 1]
    assert m.length.tolist() == [3, 9, 6, 9]
    assert m.pair_ptr.tolist() == [0, 1, 2, 3, 4] and m.pair_enzyme.tolist() == [0] * 4
    assert m.pair_kcat.tolist() == [0.1] * 4 and m.pair_km.tolist() == [KM * KM_TO_MM] * 4
    assert KM_TO_MM == 1e18                      # mol / fL -> mmol / L


def test_pairs_follow_catalytic_rates_order_and_a_transcript_may_have_none():
    cfg = _config(catalytic_rates={'b': 0.3, 'a': 0.2},
                  michaelis_constants={'transcripts': {'a': {'oA': 2e-23, 'oB': 3e-23}, 'b': {'oA': 4e-23}}})
    m = DegradationModel(**cfg)
    assert m.enzyme_order == ['b', 'a']
    assert m.pair_ptr.tolist() == [0, 2, 2, 3, 3]                # oA: b then a; oAZ: none; oB: a; oBY: none
    assert m.pair_enzyme.tolist() == [0, 1, 1] and m.pair_kcat.tolist() == [0.3, 0.2, 0.2]
    assert m.pair_km.tolist() == [4e-23 * KM_TO_MM, 2e-23 * KM_TO_MM, 3e-23 * KM_TO_MM]


@pytest.mark.parametrize('change', [
    dict(michaelis_constants={'transcripts': {'endoRNAse': {'oA': KM}, 'rnaseX': {'oA': KM}}}),    # no rate
    dict(michaelis_constants={'transcripts': {'endoRNAse': {'oC': KM}}}),                        # no sequence
    dict(sequences={'oA': 'GCT'}, michaelis_constants={'transcripts': {}}),                    # no monomer
    dict(michaelis_constants={'transcripts': {'endoRNAse': {'oA': 0.0}}}),
    dict(michaelis_constants={'transcripts': {'endoRNAse': {'oA': float('nan')}}}),
    dict(michaelis_constants={'transcripts': {'endoRNAse': {'oA': float('inf')}}}),
    dict(michaelis_constants={'transcripts': {'endoRNAse': {'oA': -KM}}}),
    dict(catalytic_rates={'endoRNAse': 0.0}),
    dict(catalytic_rates={'endoRNAse': float('inf')}),
    dict(catalytic_rates={'endoRNAse': 'fast'}),
    dict(sequences={'t%d' % i: 'G' for i in range(65)}, michaelis_constants={'transcripts': {}}),
    dict(catalytic_rates={'e%d' % i: 1.0 for i in range(9)}, michaelis_constants={'transcripts': {}}),
    dict(sequences={'t%d' % i: 'G' for i in range(64)}, catalytic_rates={'e%d' % i: 1.0 for i in range(8)},
         michaelis_constants={'transcripts': {'e%d' % e: {'t%d' % t: KM for t in range(64)} for e in range(5)}}),
    dict(monomer_ids=['ATP', 'GTP', 'UTP', 'CTP', 'XTP']),
    dict(monomer_ids=['ATP', 'GTP', 'UTP', 'ADP']),
    dict(transcript_species={'oC': 'oC_RNA'}),
    dict(transcript_species={'oA': 'endoRNAse'}),
])
def test_model_refusals(change):
    with pytest.raises(ValueError, match='degradation'):
        DegradationModel(**_config(**change))


def test_limits_are_accepted():
    m = DegradationModel({'t%d' % i: 'GACU' for i in range(64)}, {'e%d' % i: 1.0 for i in range(8)},
                         {'transcripts': {'e%d' % e: {'t%d' % t: KM for t in range(64) if (t + e) % 2 == 0}
                                          for e in range(8)}})
    assert (m.n_transcripts, m.n_enzymes, m.n_pairs, m.n_monomers) == (64, 8, 256, 4)


def test_bind_over_active_and_passive_rows():
    m, tm = dref.toy_model(), xref.toy_model()
    sm = StochasticModel(['X', 'oA', 'endoRNAse'], {'r': {'X': 1}}, {'r': 1.0}, passive=['oB', 'oBY', 'oAZ'])
    transcript_row, enzyme_row = m.bind(sm, tm)
    assert transcript_row.tolist() == [1, 5, 3, 4] and enzyme_row.tolist() == [2]
    with pytest.raises(ValueError, match='lacks the species'):
        m.bind(StochasticModel(['oA', 'oAZ', 'oB', 'oBY'], {'r': {'oA': 1}}, {'r': 1.0}), tm)
    with pytest.raises(ValueError, match='lacks the species'):
        m.bind(StochasticModel(['oA', 'endoRNAse'], {'r': {'oA': 1}}, {'r': 1.0}, passive=['oB', 'oBY']), tm)
    with pytest.raises(ValueError, match='StochasticModel'):
        m.bind('not a model', tm)
    with pytest.raises(ValueError, match='TranscriptionModel'):
        m.bind(sm, None)
    with pytest.raises(ValueError, match='pools'):
        m.bind(sm, xref.toy_model(monomer_ids=['GTP', 'UTP', 'CTP', 'ATP']))


def test_product_sequences_on_the_toy_chromosome():
    """Slices taken by hand from toy_chromosome.json: ATACGGCACGTGACCGTCAACTTA, pA at 3 forward with
    terminators at 6 and 12, pB at -3 backward with terminators at -9 and -12."""
    data = xref.toy_data()
    s, rna = data['sequence'], {'A': 'U', 'T': 'A', 'C': 'G', 'G': 'C'}
    by_hand = {'oA': s[3:6], 'oAZ': s[3:12], 'oB': s[-3:-9:-1], 'oBY': s[-3:-12:-1]}
    by_hand = {k: ''.join(rna[b] for b in v) for k, v in by_hand.items()}
    assert by_hand['oA'] == 'GCC' and by_hand['oBY'] == 'AGUUGACGG'
    tm = xref.toy_model()
    assert tm.product_sequences() == by_hand
    assert list(tm.product_sequences()) == ['oA', 'oAZ', 'oB', 'oBY']
    # they are the sequences of the reference's own TOY_CONFIG
    assert tm.product_sequences() == dref.toy_data()['sequences']


def test_product_sequences_a_later_promoter_overwrites():
    data = copy.deepcopy(configs.TOY_CHROMOSOME)
    data['promoters']['pR']['terminators'][0]['products'] = ['oP']         # pR's first terminator names oP too
    tm = configs.toy_transcription(data)
    s = tm.product_sequences()
    assert s['oP'] == tm.sequences[1][:6] and s['oPQ'] == tm.sequences[0][:11] and 'oR' not in s


def test_from_transcription_takes_names_and_monomers():
    tm = configs.flagella_transcription(xref.flagella_data(), operons=['fliC', 'flhDC'])
    m = configs.flagella_degradation(dref.flagella_data(), tm)
    assert m.transcript_order == list(tm.product_sequences()) and set(m.transcript_order) == {'fliC', 'flhDC'}
    assert m.transcript_names() == [o + '_RNA' for o in m.transcript_order]
    assert m.pair_kcat.tolist() == [0.02, 0.02] and m.length.tolist() == [len(tm.product_sequences()[o])
                                                                         for o in m.transcript_order]


# -- passive rows ------------------------------------------------------------------------
def _network(**kw):
    return StochasticModel(['A', 'B', 'AB'], {'bind': {'A': -1, 'B': -1, 'AB': 1}}, {'bind': 0.5},
                           initial=kw.pop('initial', {'A': 3}), seed=5, **kw)


def test_passive_rows_are_rows_not_species():
    plain, sm = _network(), _network(passive=['P', 'Q'], initial={'A': 3, 'Q': 9})
    assert sm.species == ['A', 'B', 'AB'] and sm.passive == ['P', 'Q'] and sm.rows == ['A', 'B', 'AB', 'P', 'Q']
    assert (sm.n_species, sm.n_rows) == (3, 5) and (plain.n_species, plain.n_rows) == (3, 3)
    assert sm.index('AB') == 2 and sm.index('Q') == 4
    with pytest.raises(ValueError, match='no species'):
        sm.index('R')
    x = sm.initial_counts(2, 4)
    assert x.shape == (5, 4) and x.dtype == np.int32
    assert x[:, :2].tolist() == [[3, 3], [0, 0], [0, 0], [0, 0], [9, 9]] and not x[:, 2:].any()
    # the network is the active one: every packed array is what it is without passive rows
    for name in ('react_ptr', 'react_species', 'react_order', 'stoich_ptr', 'stoich_species', 'stoich_delta', 'rates',
                 'inv', 'matrix'):
        assert np.array_equal(getattr(sm, name), getattr(plain, name)), name
        assert getattr(sm, name).dtype == getattr(plain, name).dtype, name
    assert sm.max_order == plain.max_order and plain.passive == [] and plain.rows == plain.species
    assert plain.initial.shape == (3,) and plain.initial_counts(2, 4).shape == (3, 4)


def test_passive_refusals():
    with pytest.raises(ValueError, match='passive row'):
        StochasticModel(['A'], {'r': {'A': -1, 'P': 1}}, {'r': 1.0}, passive=['P'])
    with pytest.raises(ValueError, match='distinct'):
        _network(passive=['A'])
    with pytest.raises(ValueError, match='distinct'):
        _network(passive=['P', 'P'])
    with pytest.raises(ValueError, match='initial names the unknown'):
        _network(passive=['P'], initial={'Z': 1})
    assert _network(passive=['p%d' % i for i in range(MAX_PASSIVE)]).n_rows == 3 + 192
    with pytest.raises(ValueError, match='passive'):
        _network(passive=['p%d' % i for i in range(MAX_PASSIVE + 1)])
    with pytest.raises(ValueError, match='species'):
        StochasticModel(['s%d' % i for i in range(65)], {'r': {'s0': 1}}, {'r': 1.0}, passive=['P'])


def test_translation_and_transcription_bind_over_rows():
    tm = xref.toy_model()
    active = ['X', 'tfA', 'RNA Polymerase']
    sm = StochasticModel(active, {'r': {'X': 1}}, {'r': 1.0}, passive=['oA', 'oAZ', 'oB', 'oBY', 'tfB'])
    prod_ptr, prod, thr, rnap = tm.bind(sm)
    assert prod.tolist() == [3, 4, 5, 6] and thr.tolist() == [1, 7] and rnap == 2
    with pytest.raises(ValueError, match='lacks the species'):
        tm.bind(StochasticModel(active, {'r': {'X': 1}}, {'r': 1.0}, passive=['oA', 'oAZ', 'oB', 'oBY']))
    tl = configs.flagella_translation(_golden('flagella_translation.json'), operons=['fliC'])
    sm = StochasticModel(['X'], {'r': {'X': 1}}, {'r': 1.0}, passive=['Ribosome', 'fliC', 'fliC_RNA'])
    operon, prod, ribosome = tl.bind(sm)
    assert operon.tolist() == [3] and prod.tolist() == [2] and ribosome == 1


# -- the configs --------------------------------------------------------------------------
def _fixtures():
    return (_golden('flagella_transcription.json'), _golden('flagella_translation.json'),
            _golden('flagella_complexation.json'), dref.flagella_data())


def test_fixture_is_the_references_config():
    deg = dref.flagella_data()
    assert deg['catalytic_rates'] == {'endoRNAse': 0.02}
    kms = deg['michaelis_constants']['transcripts']
    assert list(kms) == ['endoRNAse'] and list(kms['endoRNAse']) == list(_fixtures()[0]['genes'])
    assert set(kms['endoRNAse'].values()) == {1e-23}
    state = deg['initial_state']
    assert state['proteins'] == {'CpxR': 10, 'CRP': 10, 'Fnr': 10, 'endoRNAse': 1, 'flagella': 8, 'Ribosome': 100,
                                 'RNA Polymerase': 100}
    assert all(state['molecules'][m] == 5000000 for m in ('ATP', 'GTP', 'UTP', 'CTP'))
    assert state['molecules']['Alanine'] == 1000000 and len(state['molecules']) == 24
    assert state['transcripts'] == {o: 0 for o in kms['endoRNAse']}


def test_whole_chromosome_fits():
    tx, tl, cx, deg = _fixtures()
    cfg = configs.flagella_gene_expression(tx, tl, cx, deg, operons=None, max_rnaps=16, max_ribosomes=16)
    assert set(cfg) == {'stochastic', 'transcription', 'translation', 'degradation'}
    sm, tm, lm, dm = cfg['stochastic'], cfg['transcription'], cfg['translation'], cfg['degradation']
    assert sm.n_species <= 64 and sm.n_reactions == 7 and list(sm.reactions) == list(cx['stoichiometry'])
    assert sm.species == cx['monomer_ids'] + cx['complex_ids']
    # the rows, derived from the four fixtures: monomers and complexes, a transcript per operon, every
    # translated protein, the factors the promoters' thresholds name, what the initial state names
    rows = set(cx['monomer_ids']) | set(cx['complex_ids'])
    rows |= {o + '_RNA' for o in tx['genes']}
    rows |= {p for _, p in tl['transcripts']}
    rows |= {f for p in tx['promoters'].values() for s in p['sites'] for f in s['thresholds']}
    rows |= set(deg['initial_state']['proteins'])
    assert sm.n_rows == len(rows) and set(sm.rows) == rows and sm.n_rows > 64
    assert sm.passive[:15] == tm.products == dm.transcript_names() and len(tm.products) == 15
    assert tm.n_templates == 15 and lm.n_templates == len(tl['transcripts'])
    assert (tm.max_rnaps, lm.max_ribosomes) == (16, 16)
    # every transcript has a degradation pair, with the fixture's numbers
    assert dm.n_transcripts == 15 and np.all(np.diff(dm.pair_ptr) == 1)
    assert dm.pair_kcat.tolist() == [0.02] * 15 and dm.pair_km.tolist() == [1e-23 * KM_TO_MM] * 15
    # every model finds its rows
    tm.bind(sm), lm.bind(sm), dm.bind(sm, tm)
    x = sm.initial_counts(1, 1)[:, 0]
    assert {name: int(x[sm.index(name)]) for name in deg['initial_state']['proteins']} == deg['initial_state']['proteins']
    assert int(x.sum()) == sum(deg['initial_state']['proteins'].values())
    with pytest.raises(ValueError, match='passive row'):        # no reaction may name a transcript
        StochasticModel(sm.species, {'decay': {'fliC_RNA': -1}}, {'decay': 1.0}, passive=sm.passive)


def test_operons_cut_the_model_down():
    cfg = configs.flagella_gene_expression(*_fixtures(), operons=['fliC', 'flhDC'])
    assert cfg['degradation'].transcript_names() == cfg['transcription'].products
    assert set(cfg['transcription'].products) == {'fliC_RNA', 'flhDC_RNA'}
    assert cfg['stochastic'].n_species == 37 and cfg['stochastic'].n_reactions == 7


# -- the restatement on the reference's toy ---------------------------------------------
def test_toy_conserves_the_nucleotides():
    """test_rna_degradation (degradation.py:185-207): 10 of every species, endoRNAse 10, T = 1, 10
    steps.  Per nucleotide the pool plus the bases still in transcripts stays what it was."""
    data = dref.toy_data()
    m = dref.toy_model()
    table = m.species()
    rows = dref.bind(m, table)
    state = data['initial_state']
    counts = np.array([[state['transcripts'].get(s, state['proteins'].get(s))] for s in table], dtype=np.int32)
    molecules = np.array([[state['molecules'][s]] for s in m.molecule_ids], dtype=np.int32)
    partial = np.zeros((4, 1))

    def held(i):
        return int(molecules[i, 0]) + int((counts[rows[0], 0].astype(np.int64) * m.composition[:, i]).sum())

    start = [held(i) for i in range(4)]
    total, trajectory = 0, []
    for _ in range(data['total_time']):
        degraded, status = dref.step(m, rows, counts, partial, molecules, np.array([1.0]), data['time_step'])
        assert not status.any() and np.all((0 <= partial) & (partial < 1))
        total += int(degraded[0])
        trajectory.append(counts[rows[0], 0].tolist())
        for i, name in enumerate(m.molecule_ids[:4]):
            if name != 'ATP':                    # GTP, UTP, CTP; ATP also gains the hydrolysis quirk
                assert held(i) == start[i], name
    assert total > 0 and trajectory[-1] == [10 - total // 4] * 4
    # the reference's signs: ATP rose and ADP fell by a base per base degraded
    bases = int(((10 - counts[rows[0], 0]) * m.length).sum())
    assert held(0) == start[0] + bases and int(molecules[4, 0]) == 10 - bases


def test_restatement_refuses_without_writing():
    m = dref.toy_model()
    table = m.species()
    rows = dref.bind(m, table)
    for m2c, pool, bits in ((0.0, 10, dref.NONFINITE), (float('inf'), 10, dref.NONFINITE), (float('nan'), 10, dref.NONFINITE),
                            (-1.0, 10, dref.NONFINITE), (1.0, 2 ** 31 - 2, dref.OVERFLOW)):
        counts = np.array([10, 10, 10, 10, 1000], dtype=np.int32)
        partial = np.full(4, 0.5)
        molecules = np.array([100, pool, 10, 10, 10], dtype=np.int32)
        before = counts.copy(), partial.copy(), molecules.copy()
        degraded, status = dref.step_agent(m, rows, counts, partial, molecules, m2c, 1.0)
        assert (degraded, status) == (0, bits)
        assert all(np.array_equal(a, b) for a, b in zip(before, (counts, partial, molecules)))


# -- population ---------------------------------------------------------------------------
def test_population_table():
    assert population.DEGRADATION_ARRAYS == (('deg_partial', population._ZERO),)
    assert population._ALL_AGENT_ARRAYS[-1] == ('deg_partial', population._ZERO)
    assert population._ALL_AGENT_ARRAYS[:-1] == (population.AGENT_ARRAYS + population.STOCHASTIC_ARRAYS +
                                                 population.TRANSLATION_ARRAYS + population.TRANSCRIPTION_ARRAYS)
    assert sorted(population.DIVIDERS) == ['counts', 'flagella', 'given', 'lineage', 'locations', 'molecules',
                                           'ribosomes']
    assert 'deg_partial' not in dict(population.AGENT_ARRAYS)


def test_passive_seed_has_a_domain_and_the_chunk():
    from lens_amd import native
    from lens_amd.stochastic import passive_seed
    assert passive_seed(5, 0) == 5 ^ native.VK_SSA_PASSIVE_DOMAIN and passive_seed(5, 2) == passive_seed(5, 0) + 2
    assert len({passive_seed(5, c) for c in range(3)} | {5}) == 4
    assert native.VK_SSA_PASSIVE_DOMAIN not in (native.VK_SSA_DOMAIN, native.VK_SSA_DIVIDE_DOMAIN)


def test_colony_refusals_come_first(monkeypatch):
    """degradation= without stochastic= and transcription=, or over a table that lacks a row, is
    refused before anything is built (no device is touched)."""
    torch = pytest.importorskip('torch')
    from lens_amd.colony import Colony

    def refuse(*args, **kw):
        raise AssertionError('a buffer was allocated before the refusal')

    dm, tm = dref.toy_model(), xref.toy_model()
    full = StochasticModel(xref.SPECIES, {'decay': {'oA': -1, 'X': 1}}, {'decay': 0.05}, passive=['endoRNAse'])
    cases = [dict(degradation=dm), dict(degradation=dm, stochastic=full), dict(degradation=dm, transcription=tm),
             dict(degradation='not a model', stochastic=full, transcription=tm),
             dict(degradation=dm, stochastic=xref.toy_stochastic(), transcription=tm)]        # no endoRNAse row
    monkeypatch.setattr(torch, 'zeros', refuse)
    monkeypatch.setattr(torch, 'full', refuse)
    for kw in cases:
        with pytest.raises(ValueError, match='degradation|transcription needs'):
            Colony(configs.glc_lct_config(), 4, device='cpu', environment='held', **kw)
