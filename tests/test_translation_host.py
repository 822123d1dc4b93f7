"""The translation step on the host: the sub-interval plan, the restatement
tests/translation_ref.py against the rules include/vk_kinetics.h states above
vk_translation_step, the model's refusals, and one distribution check.  No GPU."""

import copy
import math

import numpy as np
import pytest

import ssa_ref as sref
import translation_ref as tref
from lens_amd.translation import TranslationModel, pack, sub_intervals, unpack

X = tref.SPECIES.index
POOLS = [50, 50, 50, 50, 1000, 0]


def literal_loop(timestep, rate):
    """translation.py:469-533 with everything but the clock taken out."""
    out, time = [], 0
    while time < timestep:
        distance = 1 / rate
        interval = min(distance, timestep - time)
        out.append((interval, interval == distance))
        time += interval
    return out


@pytest.mark.parametrize('T, rate, elongating, partial', [
    (1, 5, 4, 0.19999999999999996), (1, 22, 22, 3.3e-16), (10, 22, 219, 1 / 22.0), (1, 3, 3, None),
    (0.1, 5, 0, 0.1), (0.25, 4, 1, None)])
def test_plan_is_the_literal_float_loop(T, rate, elongating, partial):
    model = tref.small_model(rate=rate)
    plan = model.plan(T)
    assert plan == literal_loop(T, rate) == sub_intervals(T, rate) == tref.plan(T, rate)
    assert sum(1 for _, e in plan if e) == elongating
    assert all(e for _, e in plan[:elongating])
    if partial is None:
        assert len(plan) == elongating
    else:
        assert len(plan) == elongating + 1 and not plan[-1][1]          # the trailing partial elongates nothing
        assert plan[-1][0] == pytest.approx(partial, rel=0.2 if partial < 1e-12 else 1e-12)


def run(model, ribosomes, molecules, counts, timestep=1.0, key=3, step_index=0, max_events=None, trace=None):
    sm = tref.small_stochastic()
    mol, x = np.array(molecules, dtype=np.int64), np.array(counts, dtype=np.int64)
    ribosomes = copy.deepcopy(ribosomes)
    events, status, _, _ = tref.step_agent(model, model.bind(sm), ribosomes, mol, x, key, timestep, model.seed,
                                           step_index, max_events, trace)
    return ribosomes, mol, x, events, status


def counts(**named):
    x = np.zeros(len(tref.SPECIES), dtype=np.int64)
    for name, value in named.items():
        x[X(name)] = value
    return x


def test_deterministic_elongation():
    model = tref.small_model(rate=4.0, occlusion=2)
    # three elongations in 0.75 s: template 0 (3 residues) completes, template 1 moves 0 -> 3
    r, mol, x, events, status = run(model, [[0, 0, True], [1, 0, True]], POOLS, counts(), timestep=0.75)
    assert r == [[1, 3, False]] and events == 0 and status == 0
    assert x[X('pX')] == 1 and x[X('Ribosome')] == 1 and x[X('pY')] == 0
    # 'abc' + 'abc': two of each of the first three monomers; 6 residues cost 12 ATP
    assert list(mol) == [48, 48, 48, 50, 1000 - 12, 12]


def test_multi_product_terminator_and_stable_order():
    model = tref.small_model(rate=4.0, occlusion=2)
    r, mol, x, _, _ = run(model, [[2, 1, False], [1, 11, False], [0, 0, False], [2, 4, False], [1, 2, True]], POOLS,
                          counts(pW=7), timestep=0.25)
    # the second and the fourth complete; the rest keep their order
    assert r == [[2, 2, False], [0, 1, False], [1, 3, False]]
    assert x[X('pY')] == 1 and x[X('pW')] == 8 and x[X('pZ')] == 1 and x[X('Ribosome')] == 2


def test_stalling_and_the_last_monomer():
    model = tref.small_model(rate=4.0, occlusion=2)
    # both want 'a' (Ala) and one is left: the earlier in the list gets it, the other stalls
    r, mol, x, _, _ = run(model, [[1, 0, True], [0, 0, True]], [1, 50, 50, 50, 100, 0], counts(), timestep=0.25)
    assert r == [[1, 1, True], [0, 0, True]] and mol[0] == 0
    r, mol, x, _, _ = run(model, [[0, 0, True], [1, 0, True]], [1, 50, 50, 50, 100, 0], counts(), timestep=0.25)
    assert r == [[0, 1, True], [1, 0, True]]
    # a stalled ribosome stays for good while the pool is empty; the books count what was taken
    r, mol, x, _, _ = run(model, [[1, 0, True]], [1, 1, 0, 50, 100, 0], counts(), timestep=1.0)
    assert r == [[1, 2, False]] and list(mol) == [0, 0, 0, 50, 96, 4]


def test_invariants():
    for release in ('reference', 'template'):
        model, sm, lists, molecules, x, keys = tref.step_case(65, release)
        rows = model.bind(sm)
        for step_index in range(3):
            before = copy.deepcopy(lists), molecules.copy(), x.copy()
            tref.step(model, rows, lists, molecules, x, keys, 1.0, model.seed, step_index)
            for a in range(65):
                # Ribosome plus the list length is conserved
                assert x[X('Ribosome'), a] + len(lists[a]) == before[2][X('Ribosome'), a] + len(before[0][a])
                used = int((before[1][:4, a] - molecules[:4, a]).sum())
                assert used >= 0 and molecules[4, a] == before[1][4, a] - 2 * used
                assert molecules[5, a] == before[1][5, a] + 2 * used
                # the sum of the position advances: what stayed, what was bound, what completed
                done = {s: int(x[X(s), a] - before[2][X(s), a]) for s in ('pX', 'pY', 'pZ')}
                lengths = {'pX': 3, 'pY': 12, 'pZ': 5}
                end = sum(p for _, p, _ in lists[a]) + sum(lengths[s] * done[s] for s in done)
                assert used == end - sum(p for _, p, _ in before[0][a])
            assert np.array_equal(molecules[:, 65:], before[1][:, 65:]) and np.array_equal(x[:, 65:], before[2][:, 65:])


def test_release_modes_where_bound_0_goes_negative():
    """One template-2 ribosome passes the occlusion: the reference releases a transcript of
    template 0 (bound[0] = -1: one more unbound than there are), 'template' one of template 2."""
    for release, template, unbound in (('reference', 0, 4), ('template', 2, 2)):
        model = tref.small_model(release, rate=4.0, occlusion=2)
        trace = []
        r, _, _, events, _ = run(model, [[2, 0, True]], POOLS, counts(o1=3, o2=1), timestep=0.5, trace=trace)
        assert events == 0 and r == [[2, 2, False]]
        assert [t for t in trace if t[1] == 'release'] == [(1, 'release', template, unbound)]
    # and the outcomes differ: a free ribosome then finds one more template-0 transcript or none
    hits = {}
    for release in ('reference', 'template'):
        model = tref.small_model(release, rate=4.0, occlusion=1, affinities=(40.0, 0.0, 0.0))
        hits[release] = 0
        for key in range(200):
            _, _, _, events, _ = run(model, [[2, 0, True]], POOLS, counts(o1=0, o2=1, Ribosome=1), timestep=0.5, key=key)
            hits[release] += events
    assert hits['template'] == 0 and hits['reference'] > 150


def test_a_ribosome_initiated_in_a_sub_interval_does_not_move_in_it():
    model = tref.small_model(rate=4.0, occlusion=2, affinities=(5.0, 5.0, 5.0))
    trace = []
    r, _, _, events, _ = run(model, [], POOLS, counts(o1=4, o2=4, Ribosome=6), timestep=0.25, trace=trace)
    assert events > 0 and all(p == 0 and occ for _, p, occ in r)
    model = tref.small_model(rate=4.0, occlusion=2, affinities=(0.2, 0.2, 0.2))
    trace = []
    r, _, _, events, _ = run(model, [], POOLS, counts(o1=4, o2=4, Ribosome=6), timestep=0.75, trace=trace)
    born = {}
    for k, what, *rest in trace:
        if what == 'bind':
            born.setdefault(k, 0)
            born[k] += 1
    # a ribosome bound in sub-interval k has moved once per later elongating sub-interval
    want = sorted((2 - k for k, c in born.items() for _ in range(c)), reverse=True)
    assert sorted((p for _, p, _ in r), reverse=True) == want and len(born) > 1


def test_status_rules():
    model = tref.small_model(max_ribosomes=2, affinities=(50.0, 50.0, 50.0))
    r, _, _, events, status = run(model, [[1, 0, True], [1, 1, True]], POOLS, counts(o1=5, o2=5, Ribosome=5))
    assert status == tref.SLOTS_FULL and events == 0 and len(r) == 2
    model = tref.small_model()
    r, mol, x, events, status = run(model, [[0, 0, True]], POOLS, counts(o1=5, Ribosome=5), key=2 ** 31)
    assert status == tref.BAD_KEY and r == [[0, 0, True]] and list(mol) == POOLS
    r, mol, x, events, status = run(model, [[0, 2, False], [2, 0, False]], POOLS, counts(pX=2 ** 31 - 1))
    assert status == tref.OVERFLOW and r == [[0, 2, False], [2, 0, False]] and list(mol) == POOLS
    model = tref.small_model(affinities=(50.0, 50.0, 50.0))
    r, _, _, events, status = run(model, [], POOLS, counts(o1=9, o2=9, Ribosome=9), max_events=2)
    assert status == tref.MAX_EVENTS and events == 2 and len(r) == 2


def test_pack_roundtrip():
    for t, p, occ in ((0, 0, True), (63, 2 ** 24 - 1, False), (5, 1234, True)):
        assert unpack(pack(t, p, occ)) == (t, p, occ)
    model = tref.small_model()
    words = model.check_ribosomes([(1, 11, True), (0, 2, False)])
    assert [unpack(w) for w in words] == [(1, 11, True), (0, 2, False)]
    for bad in ([(3, 0, True)], [(0, 3, True)], [(0, -1, True)], [(0, 0, True)] * 9):
        with pytest.raises(ValueError):
            model.check_ribosomes(bad)


def _config(**changes):
    cfg = tref.small_config()
    cfg.update(changes)
    return cfg


def test_refusals():
    TranslationModel(**_config())
    key = ('o1', 'pX')

    def templates(**changes):
        t = copy.deepcopy(_config()['templates'])
        t[key].update(changes)
        return t

    two = [{'position': 2, 'strength': 1.0, 'products': ['pX']}, {'position': 3, 'strength': 1.0, 'products': ['pX']}]
    for what, cfg in (
            ('more than one terminator', _config(templates=templates(terminators=two))),
            ('no terminator', _config(templates=templates(terminators=[]))),
            ('a terminator not at len(sequence)', _config(templates=templates(terminators=two[:1]))),
            ('sites', _config(templates=templates(sites=[{'thresholds': {'CRP': 1e-5}}]))),
            ('direction -1', _config(templates=templates(direction=-1))),
            ('keys not grouped by operon', _config(transcript_affinities={
                ('o1', 'pX'): 0.3, ('o2', 'pZ'): 0.5, ('o1', 'pY'): 0.2})),
            ('a symbol without a monomer', _config(sequences={**tref.SEQUENCES, key: 'abx'})),
            ('a monomer not among the molecules', _config(molecules=['Ala', 'Gly', 'Ser'])),
            ('a missing sequence', _config(sequences={k: v for k, v in tref.SEQUENCES.items() if k != key})),
            ('release', _config(release='both')),
            ('max_ribosomes', _config(max_ribosomes=129)),
            ('max_ribosomes', _config(max_ribosomes=0)),
            ('rate', _config(elongation_rate=0.0)),
            ('a product that is a transcript', _config(templates=templates(
                terminators=[{'position': 3, 'strength': 1.0, 'products': ['o2']}])))):
        with pytest.raises(ValueError):
            TranslationModel(**cfg)
            pytest.fail(what)
    # a species missing from the StochasticModel
    from lens_amd.stochastic import StochasticModel
    model = tref.small_model()
    for missing in ('o2', 'pW', 'Ribosome'):
        sm = StochasticModel([s for s in tref.SPECIES if s != missing], {'r': {'C1': 1}}, {'r': 1.0})
        with pytest.raises(ValueError, match=missing):
            model.bind(sm)
    with pytest.raises(ValueError):
        model.bind(None)


def test_colony_refuses_translation_without_stochastic():
    """Checked before anything is built: no GPU is touched."""
    from lens_amd.colony import Colony
    with pytest.raises(ValueError, match='stochastic'):
        Colony({'reactions': {}, 'kinetic_parameters': {}}, 4, translation=tref.small_model())
    with pytest.raises(ValueError, match='TranslationModel'):
        Colony({'reactions': {}, 'kinetic_parameters': {}}, 4, stochastic=tref.small_stochastic(), translation=object())
    from lens_amd.stochastic import StochasticModel
    with pytest.raises(ValueError, match='lacks the species'):
        Colony({'reactions': {}, 'kinetic_parameters': {}}, 4, translation=tref.small_model(),
               stochastic=StochasticModel(['C1'], {'r': {'C1': 1}}, {'r': 1.0}))


def test_initiation_fraction():
    """One elongating sub-interval (T = 0.25, rate 4), one free ribosome, G copies of one
    transcript: she binds with probability 1 - exp(-a G 0.25); 4096 keys, 5 sigma."""
    a, G, n = 0.5, 4, 4096
    model = tref.small_model(rate=4.0, affinities=(0.0, 0.0, a), seed=77)
    assert model.plan(0.25) == [(0.25, True)]
    hits = 0
    for key in range(n):
        r, _, x, events, status = run(model, [], POOLS, counts(o2=G, Ribosome=1), timestep=0.25, key=key * 7919 + 1)
        assert status == 0 and events in (0, 1) and x[X('Ribosome')] == 1 - events and r == [[2, 0, True]] * events
        hits += events
    p = 1.0 - math.exp(-a * G * 0.25)
    assert abs(hits / n - p) <= 5.0 * math.sqrt(p * (1.0 - p) / n), (hits / n, p)


def test_philox_pair_against_the_ssa_restatement():
    rng = np.random.default_rng(3)
    for _ in range(50):
        seed, step = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 31))
        key, e = int(rng.integers(0, 2 ** 31)), int(rng.integers(0, 2 ** 40))
        u1, u2 = sref.philox_pair(seed, step, np.array([key]), np.array([e]))
        assert tref.philox_pair(seed, step, key, e) == (float(u1[0]), float(u2[0]))


def test_flagella_fixture_builds_the_model():
    """tests/golden/flagella_translation.json through configs.flagella_translation: the
    reference's keys, affinities, rate and occlusion; sequences synthesised at the estimated
    lengths (the fixture holds none)."""
    import json
    import os
    from lens_amd import configs
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'flagella_translation.json')) as f:
        data = json.load(f)
    assert len(data['transcripts']) == 52 and data['elongation_rate'] == 22 and data['polymerase_occlusion'] == 50
    assert data['sequences'] is None
    affinity = dict(zip(map(tuple, data['transcripts']), data['transcript_affinities']))
    assert affinity[('flgE', 'flgE')] == pytest.approx(12.0) and affinity[('flhDC', 'flhD')] == pytest.approx(0.1)
    model = configs.flagella_translation(data, max_ribosomes=128)
    assert model.n_templates == 52 and model.n_monomers == 20 and model.transcript_order[0] == ('flhDC', 'flhD')
    assert len(model.species()) == 15 + 49 + 1 and 'fliL_RNA' in model.species() and 'fliL' in model.species()
    assert [model.length(t) for t in range(52)] == [data['estimated_length'][p] for _, p in model.transcript_order]
    assert model.plan(10.0)[-1] == (pytest.approx(1 / 22.0, rel=1e-9), False) and len(model.plan(10.0)) == 220
    again = configs.flagella_translation(data, max_ribosomes=128)
    assert np.array_equal(model.seq, again.seq)                         # seeded
    some = configs.flagella_translation(data, operons=['flhDC', 'fliC'],
                                        sequences={'flhD': 'MHTSELLK', 'flhC': 'MSEKSIV', 'fliC': 'MAQVINTNSL'})
    assert some.n_templates == 3 and [some.length(t) for t in range(3)] == [8, 7, 10]
