"""The transcription model on the host (lens_amd.transcription) and the restatement of its step
(tests/transcription_ref.py): sequences, terminators, the affinity table, elongation, the books
with their ATP quirk, occlusion, the refusals and two distribution checks.  No GPU."""

import copy
import math

import numpy as np
import pytest

import ssa_ref as sref
import transcription_ref as xref
from lens_amd import configs
from lens_amd.transcription import TranscriptionModel, pack, rna_bases, sub_intervals, unpack

S = xref.SPECIES
POOLS = [50, 50, 50, 50, 0]          # ATP, GTP, UTP, CTP, ADP
# k elongating sub-intervals at rate 10 and a partial one: the reference's float loop makes of 0.3 s
# two sub-intervals of 0.1 and one of 0.09999999999999998, which elongates nothing
T = lambda k: 0.1 * k + 0.05


def counts(**named):
    x = np.zeros(len(S), dtype=np.int64)
    for name, value in named.items():
        x[S.index(name.replace('_', ' '))] = value
    return x


def run(model, rnaps, molecules, x, timestep=1.0, key=5, m2c=10.0, step_index=0, max_events=None, trace=None):
    """One agent through the restatement: (rnaps, molecules, counts, events, status)."""
    rnaps, mol, x = copy.deepcopy(rnaps), np.array(molecules, dtype=np.int64), np.array(x, dtype=np.int64)
    events, status, _ = xref.step_agent(model, model.bind(xref.toy_stochastic()), rnaps, mol, x, m2c, key, timestep,
                                        model.seed, step_index, max_events, trace)
    return rnaps, mol, x, events, status


def test_toy_sequences_and_terminators():
    """Hand-written: pA reads sequence[3:12], pB reads sequence[-3:-12:-1], both through rna_bases."""
    model = xref.toy_model()
    assert model.promoter_order == ['pA', 'pB']
    dna = 'ATACGGCACGTGACCGTCAACTTA'
    assert dna[3:12] == 'CGGCACGTG' and dna[-3:-12:-1] == 'TCAACTGCC'
    assert rna_bases('ATCG') == 'UAGC'
    assert model.sequences == ['GCCGUGCAC', 'AGUUGACGG']
    assert model.term_pos_rel == [[3, 9], [6, 9]]
    assert list(model.n_term) == [2, 2] and list(model.term_pos) == [3, 9, 0, 0, 6, 9, 0, 0]
    assert list(model.term_strength) == [0.5, 1.0, 0, 0, 0.5, 1.0, 0, 0]
    assert list(model.term_from) == [1.5, 1.0, 0, 0, 1.5, 1.0, 0, 0]
    row = {'A': 0, 'G': 1, 'U': 2, 'C': 3}
    assert list(model.seq) == [row[c] for c in 'GCCGUGCAC' + 'AGUUGACGG'] and list(model.seq_ptr) == [0, 9, 18]
    # 2 bits per base, 16 to a word
    bases = [(int(model.seq2[b >> 4]) >> (2 * (b & 15))) & 3 for b in range(18)]
    assert bases == list(model.seq)
    assert model.molecule_ids == ['ATP', 'GTP', 'UTP', 'CTP', 'ADP'] and (model.atp_row, model.adp_row) == (0, 4)
    assert model.terminator_products == [[['oA'], ['oAZ']], [['oB'], ['oBY']]]
    assert list(model.copy) == [1, 1]
    own = configs.toy_transcription()                        # the engine's own toy of the same shape
    assert own.n_templates == 2 and [len(s) for s in own.sequences] == [11, 12] and own.term_pos_rel[1] == [6, 12]


def test_affinity_table():
    model = xref.toy_model()
    assert model.affinity_of(0, (None,)) == 1.0 and model.affinity_of(0, ('tfA',)) == 10.0
    rows = model.bind(xref.toy_stochastic())
    # either side of 0.3 mM (pA) and 0.5 mM (pB) at 10 counts per mM
    for a, b, want in ((2, 4, [1.0, 1.0]), (3, 4, [10.0, 1.0]), (2, 5, [1.0, 10.0]), (4, 6, [10.0, 10.0])):
        got, _ = xref.affinity_vector(model, rows[2], counts(tfA=a, tfB=b), 10.0)
        assert got == want
    assert model.binding_state(0, {'tfA': 0.3}) == ('tfA',) and model.binding_state(0, {'tfA': 0.29}) == (None,)
    # a two-site flagella promoter: four states, the missing (p, None, None) is 0.0
    flag = configs.flagella_transcription(xref.flagella_data())
    p = flag.promoter_order.index('fliLp1')
    assert flag.site_factors[p] == [['flhDC'], ['fliA']] and flag.site_thresholds[p] == [[1e-06], [1.3e-05]]
    assert [flag.affinity_of(p, s) for s in ((None, None), ('flhDC', None), (None, 'fliA'), ('flhDC', 'fliA'))] == [
        0.0, 1.2, 0.25, 1.2 + 0.25]
    assert flag.affinity_of(0, ('CRP',)) == 0.01 and flag.affinity_of(0, (None,)) == 0.0
    assert flag.binding_state(p, {'flhDC': 2e-6, 'fliA': 0.0}) == ('flhDC', None)
    # first factor wins, in the site's dict order
    tpl = copy.deepcopy(xref.toy_data()['promoters'])
    tpl['pA']['sites'][0]['thresholds'] = {'tfB': 0.5, 'tfA': 0.3}
    both = TranscriptionModel('ATACGGCACGTGACCGTCAACTTA', tpl, {}, {('pA', 'tfA'): 2.0, ('pA', 'tfB'): 3.0,
                                                                      ('pB', None): 1.0}, ['tfA', 'tfB'], 10.0, 5)
    assert both.site_factors[0] == [['tfB', 'tfA']] and list(both.affinity[:3]) == [0.0, 3.0, 2.0]
    assert both.binding_state(0, {'tfA': 1.0, 'tfB': 1.0}) == ('tfB',)
    assert both.binding_state(0, {'tfA': 1.0, 'tfB': 0.1}) == ('tfA',)
    got, _ = xref.affinity_vector(both, both.bind(xref.toy_stochastic())[2], counts(tfA=9, tfB=9), 10.0)
    assert got == [3.0, 0.0]                                 # pB is bound by tfB, a state without a key


def test_sub_intervals_are_translations():
    model = xref.toy_model()
    assert model.plan(0.55) == sub_intervals(0.55, 10.0) == xref.plan(0.55, 10.0)
    assert [e for _, e in model.plan(0.55)] == [True] * 5 + [False]


def test_deterministic_elongation_and_stalls():
    model = xref.toy_model(affinity=0.0)                     # nothing binds: a freed RNAP stays free
    # pA = GCCGUGCAC: from 0, three steps reach the first terminator (no RNAP is free: no initiation)
    trace = []
    r, mol, x, events, status = run(model, [[0, 1, 4, False]], POOLS, counts(), timestep=T(3), trace=trace)
    assert r == [[0, 1, 7, False]] and events == 0 and status == 0
    assert list(mol) == [50 - 3, 49, 49, 49, 3]                  # U, G, C taken: ATP pays 3 though no A was used
    # the last terminator always terminates: oAZ and one free RNAP
    r, mol, x, events, status = run(model, [[0, 1, 7, False]], POOLS, counts(), timestep=T(2), m2c=1e9)
    assert r == [] and x[S.index('oAZ')] == 1 and x[S.index('RNA Polymerase')] == 1 and x[S.index('oA')] == 0
    # a stall: no UTP, the RNAP waits at the U (position 4) while CTP and GTP stay
    r, mol, x, events, status = run(model, [[0, 1, 3, False]], [50, 50, 0, 50, 0], counts(), timestep=T(5))
    assert r == [[0, 1, 4, False]] and list(mol) == [49, 49, 0, 50, 1]
    # the last-monomer contest: the earlier in the list takes the only GTP
    r, mol, x, events, status = run(model, [[0, 1, 5, False], [0, 1, 3, False]], [50, 1, 50, 50, 0], counts(),
                                    timestep=0.1)
    assert r == [[0, 1, 6, False], [0, 1, 3, False]] and mol[1] == 0
    r, mol, x, events, status = run(model, [[0, 1, 3, False], [0, 1, 5, False]], [50, 1, 50, 50, 0], counts(),
                                    timestep=0.1)
    assert r == [[0, 1, 4, False], [0, 1, 5, False]]
    # occluding RNAPs elongate too (is_polymerizing), and order is kept when one leaves
    r, mol, x, events, status = run(model, [[1, 1, 6, True], [0, 1, 8, False], [1, 1, 7, False]], POOLS, counts(),
                                    timestep=0.1, m2c=1e9)
    assert r == [[1, 1, 7, False], [1, 1, 8, False]]


def test_books_with_the_atp_quirk():
    model = xref.toy_model(affinity=0.0)
    # pA from 3: G U G C A C -> g = 2, u = 1, c = 2, a = 1
    r, mol, x, events, status = run(model, [[0, 1, 3, False]], [10, 10, 10, 10, 0], counts(), timestep=T(6), m2c=1e9)
    assert r == [] and list(mol) == [10 - 6, 10 - 2, 10 - 1, 10 - 2, 6]      # ATP -= a+g+u+c, not 2a+g+u+c
    # the stored ATP goes below zero while limit['ATP'] never did: one ATP, one A among five bases
    r, mol, x, events, status = run(model, [[0, 1, 3, False]], [1, 10, 10, 10, 0], counts(), timestep=T(5))
    assert r == [[0, 1, 8, False]] and list(mol) == [1 - 5, 8, 9, 9, 5] and status == 0
    # ... and with no ATP the A stalls her, the others were paid for all the same
    r, mol, x, events, status = run(model, [[0, 1, 3, False]], [0, 10, 10, 10, 0], counts(), timestep=T(6))
    assert r == [[0, 1, 7, False]] and list(mol) == [-4, 8, 9, 9, 4]
    # ATP as no monomer: a row of its own in front of ADP
    data = xref.toy_data()
    other = TranscriptionModel(data['sequence'], data['promoters'], data['genes'],
                               {}, ['tfA', 'tfB'], 10.0, 5,
                               symbol_to_monomer={'A': 'a', 'G': 'g', 'U': 'u', 'C': 'c'}, monomer_ids=['a', 'g', 'u', 'c'])
    assert other.molecule_ids == ['a', 'g', 'u', 'c', 'ATP', 'ADP'] and (other.atp_row, other.adp_row) == (4, 5)
    r, mol, x, events, status = run(other, [[0, 1, 3, False]], [10, 10, 10, 10, 100, 0], counts(), timestep=T(6), m2c=1e9)
    assert list(mol) == [9, 8, 9, 8, 94, 6]


def test_blocked_promoters_and_unocclusion():
    """occlusion 5, rate 10, one free RNAP, pB without affinity.  A stored occluding RNAP blocks pA
    from the start; pA reopens (her own template) in the sub-interval her RNAP reaches position 5."""
    data = xref.toy_data()
    data['promoter_affinities'] = [[['pA', None], 1e6]]
    model = configs.toy_transcription(data, seed=11)
    trace = []
    r, mol, x, events, status = run(model, [[0, 0, 1, True]], POOLS, counts(RNA_Polymerase=1), timestep=1.0,
                                    trace=trace, m2c=1e9)
    binds = [t for t in trace if t[1] == 'bind']
    opens = [t for t in trace if t[1] == 'unocclude']
    # position 1 -> 5 takes sub-intervals 0..3 (a read-through at 3 may end her: then free rises instead)
    first = trace[0]
    assert first[:2] == (0, 'elongate')
    if opens:
        assert opens[0][0] == 3 and opens[0][2] == 0
        assert binds and binds[0] == (4, 'bind', 0)              # blocked until then, bound right after
    # a newly bound RNAP first moves in the next sub-interval
    r, mol, x, events, status = run(model, [], POOLS, counts(RNA_Polymerase=1), timestep=T(3), trace=(trace := []), m2c=1e9)
    assert trace[0] == (0, 'bind', 0) and trace[1][:2] == (1, 'elongate') and trace[1][3] == 1
    assert events == 1 and r == [[0, 0, 2, True]] and x[S.index('RNA Polymerase')] == 0
    # blocked derives from the stored occluding RNAPs: two of them leave open = -1, nothing binds
    r, mol, x, events, status = run(model, [[0, 0, 0, True], [0, 0, 0, True]], [0, 0, 0, 0, 0],
                                    counts(RNA_Polymerase=3), timestep=T(3))
    assert events == 0 and len(r) == 2


def test_conservation_of_rnaps():
    for n in (63, 65):
        model, sm, lists, mol, x, m2c, keys = xref.step_case(n)
        before = x[S.index('RNA Polymerase'), :n] + np.array([len(l) for l in lists])
        out, _ = xref.trajectory(model, model.bind(sm), lists, mol, x, m2c, keys, xref.TIMESTEP, 3)
        for lists_k, _, x_k, _, _ in out:
            assert np.array_equal(x_k[S.index('RNA Polymerase'), :n] + np.array([len(l) for l in lists_k]), before)
        assert np.all(mol[:, n:] == 7) and np.all(x[:, n:] == 7)


def test_status_rules():
    model = xref.toy_model(2, affinity=500.0)
    r, _, _, events, status = run(model, [[0, 1, 6, False], [1, 1, 7, False]], [0] * 5, counts(RNA_Polymerase=5))
    assert status == xref.SLOTS_FULL and events == 0 and len(r) == 2
    model = xref.toy_model()
    r, mol, x, events, status = run(model, [[0, 0, 0, True]], POOLS, counts(RNA_Polymerase=5), key=2 ** 31)
    assert status == xref.BAD_KEY and r == [[0, 0, 0, True]] and list(mol) == POOLS
    r, mol, x, events, status = run(model, [[0, 1, 8, False], [1, 1, 7, False]], POOLS, counts(oAZ=2 ** 31 - 1))
    assert status == xref.OVERFLOW and r == [[0, 1, 8, False], [1, 1, 7, False]] and list(mol) == POOLS
    model = xref.toy_model(affinity=500.0, polymerase_occlusion=0)
    r, _, _, events, status = run(model, [], [0] * 5, counts(RNA_Polymerase=9), max_events=2)
    assert status == xref.MAX_EVENTS and events == 2 and len(r) == 2


def test_pack_roundtrip():
    for t, i, p, occ in ((0, 0, 0, True), (63, 3, 2 ** 22 - 1, False), (5, 2, 1234, True)):
        assert unpack(pack(t, i, p, occ)) == (t, i, p, occ)
        assert 0 <= pack(t, i, p, occ) < 2 ** 32
    model = xref.toy_model()
    words = model.check_rnaps([(1, 1, 8, True), (0, 0, 2, False)])
    assert [unpack(w) for w in words] == [(1, 1, 8, True), (0, 0, 2, False)]
    for bad in ([(2, 0, 0, True)], [(0, 2, 0, True)], [(0, 0, 3, True)], [(0, 1, 2, True)], [(0, 1, 9, True)],
                [(0, 0, -1, True)], [(0, 0, 0, True)] * 9):
        with pytest.raises(ValueError):
            model.check_rnaps(bad)


def _config(**changes):
    data = xref.toy_data()
    cfg = dict(sequence=data['sequence'], templates=data['promoters'], genes=data['genes'],
               promoter_affinities={tuple(k): v for k, v in data['promoter_affinities']},
               transcription_factors=['tfA', 'tfB'], elongation_rate=10.0, polymerase_occlusion=5)
    cfg.update(changes)
    return cfg


def test_refusals():
    TranscriptionModel(**_config())

    def templates(promoter='pA', **changes):
        t = copy.deepcopy(_config()['templates'])
        t[promoter].update(changes)
        return t

    term = lambda position, strength=1.0, products=('oA',): {'position': position, 'strength': strength,
                                                             'products': list(products)}
    site = lambda **thresholds: {'thresholds': thresholds}
    child = {0: {'id': 0, 'lead': 0, 'lag': 0, 'children': [1, 2]}, 1: {'id': 1, 'children': []},
             2: {'id': 2, 'children': []}}
    for what, cfg in (
            ('replication domains', _config(domains=child)),
            ('a root with children alone', _config(domains={0: child[0]})),
            ('five terminators', _config(templates=templates(terminators=[term(p) for p in (4, 5, 6, 7, 12)]))),
            ('no terminator', _config(templates=templates(terminators=[]))),
            ('terminators not increasing', _config(templates=templates(terminators=[term(8), term(6)]))),
            ('a terminator at the promoter', _config(templates=templates(terminators=[term(3), term(6)]))),
            ('a terminator behind a +1 promoter', _config(templates=templates(terminators=[term(1)]))),
            ('a sequence too short for the last terminator', _config(templates=templates(terminators=[term(40)]))),
            ('direction 0', _config(templates=templates(direction=0))),
            ('five sites', _config(templates=templates(sites=[site(tfA=0.1)] * 5))),
            ('five thresholds on a site', _config(
                transcription_factors=list('abcde'), templates=templates(sites=[site(a=1, b=1, c=1, d=1, e=1)]))),
            ('a threshold that is no factor', _config(templates=templates(sites=[site(tfC=0.1)]))),
            ('a symbol without a monomer', _config(symbol_to_monomer={'A': 'ATP', 'G': 'GTP', 'U': 'UTP'})),
            ('a monomer not among monomer_ids', _config(monomer_ids=['ATP', 'GTP', 'UTP'])),
            ('five monomers', _config(monomer_ids=['ATP', 'GTP', 'UTP', 'CTP', 'XTP'])),
            ('a product that is a factor', _config(templates=templates(terminators=[term(12, products=['tfA'])]))),
            ('a product that is the free RNAP', _config(templates=templates(
                terminators=[term(12, products=['RNA Polymerase'])]))),
            ('a product named twice', _config(templates=templates(terminators=[term(12, products=['oA', 'oA'])]))),
            ('a negative affinity', _config(promoter_affinities={('pA', None): -1.0})),
            ('an infinite affinity', _config(promoter_affinities={('pA', None): math.inf})),
            ('a NaN strength', _config(templates=templates(terminators=[term(6, math.nan), term(12)]))),
            ('a negative strength', _config(templates=templates(terminators=[term(6, -0.5), term(12)]))),
            ('a strength sum of 0 where a draw is needed', _config(templates=templates(
                terminators=[term(6, 0.0), term(12, 0.0)]))),
            ('a negative threshold', _config(templates=templates(sites=[site(tfA=-0.1)]))),
            ('a NaN threshold', _config(templates=templates(sites=[site(tfA=math.nan)]))),
            ('an affinity key of an unknown promoter', _config(promoter_affinities={('pC', None): 1.0})),
            ('an affinity key with a factor its site cannot take', _config(promoter_affinities={('pA', 'tfB'): 1.0})),
            ('an affinity key of the wrong length', _config(promoter_affinities={('pA', None, None): 1.0})),
            ('sequence', _config(sequence_path='registers')),
            ('max_rnaps', _config(max_rnaps=129)),
            ('max_rnaps', _config(max_rnaps=0)),
            ('rate', _config(elongation_rate=0.0)),
            ('65 promoters', _config(templates={'p%d' % i: dict(_config()['templates']['pA'], id='p%d' % i)
                                                for i in range(65)}, promoter_affinities={})),
            ('transcript_species of an unknown operon', _config(transcript_species={'oC': 'x'}))):
        with pytest.raises(ValueError):
            TranscriptionModel(**cfg)
            pytest.fail(what)
    # a last terminator of strength 0 needs no draw
    TranscriptionModel(**_config(templates=templates(terminators=[term(12, 0.0)])))
    # a species missing from the StochasticModel: a product, a factor, the free RNAP
    from lens_amd.stochastic import StochasticModel
    model = xref.toy_model()
    for missing in ('oAZ', 'tfB', 'RNA Polymerase'):
        sm = StochasticModel([s for s in S if s != missing], {'r': {'X': 1}}, {'r': 1.0})
        with pytest.raises(ValueError, match=missing):
            model.bind(sm)
    with pytest.raises(ValueError):
        model.bind(None)


def test_colony_refusals():
    """Checked before anything is built: no GPU is touched."""
    from lens_amd.colony import Colony
    from lens_amd.stochastic import StochasticModel
    empty = {'reactions': {}, 'kinetic_parameters': {}}
    with pytest.raises(ValueError, match='stochastic'):
        Colony(empty, 4, transcription=xref.toy_model())
    with pytest.raises(ValueError, match='TranscriptionModel'):
        Colony(empty, 4, stochastic=xref.toy_stochastic(), transcription=object())
    with pytest.raises(ValueError, match='lacks the species'):
        Colony(empty, 4, transcription=xref.toy_model(), stochastic=StochasticModel(['X'], {'r': {'X': 1}}, {'r': 1.0}))
    # everything stochastic= refuses holds with transcription= too
    from lens_amd.response import CellResponse
    with pytest.raises(ValueError, match='response'):
        Colony(empty, 4, environment='nonspatial', stochastic=xref.toy_stochastic(), transcription=xref.toy_model(),
               response=CellResponse.__new__(CellResponse))


def test_philox_pair_against_the_ssa_restatement():
    rng = np.random.default_rng(4)
    for _ in range(50):
        seed, step = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 31))
        key, e = int(rng.integers(0, 2 ** 31)), int(rng.integers(0, 2 ** 40))
        u1, u2 = sref.philox_pair(seed, step, np.array([key]), np.array([e]))
        assert xref.philox_pair(seed, step, key, e) == (float(u1[0]), float(u2[0]))


def test_initiation_fraction():
    """One elongating sub-interval (T = 0.1, rate 10), one free RNAP, pA alone with affinity a: she
    binds with probability 1 - exp(-a 0.1); 4096 keys, 5 sigma."""
    a, n = 4.0, 4096
    data = xref.toy_data()
    data['promoter_affinities'] = [[['pA', None], a]]
    model = configs.toy_transcription(data, seed=77)
    assert model.plan(0.1) == [(0.1, True)]
    hits = 0
    for key in range(n):
        r, _, x, events, status = run(model, [], POOLS, counts(RNA_Polymerase=1), timestep=0.1, key=key * 7919 + 1)
        assert status == 0 and events in (0, 1) and x[S.index('RNA Polymerase')] == 1 - events
        assert r == [[0, 0, 0, True]] * events
        hits += events
    p = 1.0 - math.exp(-a * 0.1)
    assert abs(hits / n - p) <= 5.0 * math.sqrt(p * (1.0 - p) / n), (hits / n, p)


def test_read_through_fraction():
    """pA's first terminator (strength 0.5 of 0.5 + 1.0) ends an RNAP with probability 0.5 / 1.5;
    4096 keys, 5 sigma."""
    n, model = 4096, xref.toy_model(seed=78)
    ended = 0
    for key in range(n):
        r, _, x, events, status = run(model, [[0, 0, 2, False]], POOLS, counts(), timestep=0.1, key=key * 104729 + 3,
                                      m2c=1e9)
        assert status == 0 and x[S.index('oA')] + len(r) == 1 and x[S.index('oAZ')] == 0
        assert r in ([], [[0, 1, 3, False]])
        ended += int(x[S.index('oA')])
    p = 0.5 / 1.5
    assert abs(ended / n - p) <= 5.0 * math.sqrt(p * (1.0 - p) / n), (ended / n, p)


def test_flagella_fixture_builds_the_model():
    """tests/golden/flagella_transcription.json through configs.flagella_transcription: the
    reference's 15 promoters, thresholds after apply_thresholds, affinities, rate and occlusion; a
    seeded genome over the compact layout (the fixture holds no sequence)."""
    data = xref.flagella_data()
    assert len(data['promoters']) == 15 and data['elongation_rate'] == 50 and data['polymerase_occlusion'] == 30
    assert data['sequence'] is None
    assert data['promoters']['fliLp1']['sites'][0]['thresholds'] == {'flhDC': 1e-06}        # not the 4e-06 written there
    model = configs.flagella_transcription(data)
    assert model.n_templates == 15 and len(model.seq) == 36927 and model.promoter_order[0] == 'flhDp'
    lengths = [abs(p['terminators'][-1]['position'] - p['position']) for p in data['promoters'].values()]
    assert [model.length(t) for t in range(15)] == lengths
    assert 'fliL_RNA' in model.species() and 'RNA Polymerase' in model.species() and 'flhDC' in model.species()
    assert model.factors_used() == ['CRP', 'flhDC', 'fliA']
    assert sum(e for _, e in model.plan(10.0)) == 500 and len(model.plan(10.0)) in (500, 501)
    again = configs.flagella_transcription(data)
    assert np.array_equal(model.seq, again.seq)                         # seeded
    some = configs.flagella_transcription(data, operons=['flhDC', 'fliC'])
    assert some.promoter_order == ['flhDp', 'fliCp'] and [some.length(t) for t in range(2)] == [931, 1496]
    assert some.products == ['flhDC_RNA', 'fliC_RNA']
    # a genome of one's own at the fixture's positions
    real = 'ACGT' * 600000
    given = configs.flagella_transcription(data, operons=['fliC'], sequence=real)
    assert given.sequences[0] == rna_bases(real[2002110:2003606])
