"""The antibiotic response on the host: the NumPy restatement against the
reference's golden file, the death known answers, DeathFreezeState in the
Experiment loop, model validation and every refusal.  No GPU."""

import csv
import math
import os

import numpy as np
import pytest

import response_ref as ref
from lens_amd.cells import CellModel
from lens_amd.rate_law_compiler import compile_rate_laws
from lens_amd.response import (ANTIBIOTICS_DEFAULTS, CellResponse, DeathFreezeState, BatchedCellEnvironmentDiffusion,
                               antibiotic_transport_config, from_antibiotics)

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'antibiotics_compartment_subset.csv')
N_A = 6.022140857e23
RNA = 'AcrAB-TolC_RNA'


def _antibiotics(config=None):
    kin, resp = from_antibiotics(config)
    t = compile_rate_laws(kin['reactions'], kin['kinetic_parameters'])
    return kin, resp, t, resp.bind(t)


def test_fixture_is_the_stated_subset():
    with open(FIXTURE) as f:
        rows = list(csv.DictReader(f))
    times = [int(float(r['time'])) for r in rows]
    assert times == sorted(set(range(64)) | set(range(0, 2401, 60)) | set(range(2340, 2401)))
    assert os.path.getsize(FIXTURE) < 64 * 1024


def test_layout_goes_through_the_cell_store():
    kin, resp, t, L = _antibiotics()
    assert t.species == [('internal', 'antibiotic'), ('pump_port', 'AcrAB-TolC')]
    # the expression's ('internal', 'AcrAB-TolC') is the kinetics' pump; RNA, the external
    # row (no rate law mentions it) and the porin are appended after the table's rows
    assert L.keys == t.species + [('internal', RNA), ('external', 'antibiotic'), ('membrane', 'porin')]
    assert L.row(('internal', 'AcrAB-TolC')) == L.row(('membrane', 'AcrAB-TolC')) == 1
    assert L.expr_rows.tolist() == [2, 1] and L.expression.tl_mrna_row.tolist() == [2]
    assert L.mol_int_row.tolist() == [0] and L.mol_ext_row.tolist() == [3] and L.porin_row.tolist() == [4]
    # the quirk: permeability_per_porin (5e-3) is never read; the process default 1e-1 holds
    assert L.porin_perm.tolist() == [0.1] and L.initial == {3: 1.0, 4: 1e-20}
    assert L.det_row.tolist() == [0] and L.det_thr.tolist() == [0.95]
    assert kin['kinetic_parameters']['export'][('pump_port', 'AcrAB-TolC')]['kcat_f'] == 5e-4
    assert kin['initial_state']['internal']['antibiotic'] == 0.5 and kin['initial_state']['pump_port']['AcrAB-TolC'] == 0.0
    assert antibiotic_transport_config()['kinetic_parameters']['export'][('pump_port', 'AcrAB-TolC')]['kcat_f'] == 2e-4


def test_restatement_reproduces_the_golden_bit_for_bit():
    """Every column but global_divide (the lone compartment has no MetaDivision) and
    fluxes_import (not a quantity of this engine), every fixture row."""
    kin, resp, t, L = _antibiotics()
    cm = CellModel(model='growth', growth_rate=ANTIBIOTICS_DEFAULTS['growth']['growth_rate'],
                   division_volume=float('inf'))
    rc = ref.nonspatial_ref(t, L, kin, 1, env_volume_L=1e-12, avogadro=N_A, cells=cm)
    with open(FIXTURE) as f:
        rows = list(csv.DictReader(f))
    assert set(rows[0]) - {'global_divide', 'fluxes_import'} == {
        'global_mass', 'global_volume', 'global_width', 'global_length', 'global_surface_area', 'global_dead',
        'cell_counts_AcrAB-TolC_RNA', 'cell_counts_AcrAB-TolC', 'cell_AcrAB-TolC_RNA', 'cell_AcrAB-TolC',
        'cell_antibiotic', 'cell_porin', 'external_antibiotic', 'time'}
    step = 0
    for row in rows:
        while step < int(float(row['time'])):
            rc.step(1.0)
            step += 1
        got = {
            'global_mass': rc.cell[0, 0], 'global_volume': rc.cell[1, 0] * 1e-15, 'global_width': float(cm.width),
            'global_length': rc.cell[2, 0], 'global_surface_area': rc.cell[3, 0], 'global_dead': float(rc.dead[0]),
            'cell_counts_AcrAB-TolC_RNA': rc.cell_counts(2)[0], 'cell_counts_AcrAB-TolC': rc.cell_counts(1)[0],
            'cell_AcrAB-TolC_RNA': rc.conc[2, 0], 'cell_AcrAB-TolC': rc.conc[1, 0], 'cell_antibiotic': rc.conc[0, 0],
            'cell_porin': rc.conc[4, 0], 'external_antibiotic': rc.conc[3, 0], 'time': float(step)}
        for name, value in got.items():
            assert float(row[name]) == value, (step, name, row[name], repr(value))


def test_todays_avogadro_misses_the_golden():
    """With CODATA 2018's N_A the external column is off (8e-12 relative): the golden was
    produced with the legacy constant, as the C1 fixture was."""
    kin, resp, t, L = _antibiotics()
    cm = CellModel(model='growth', growth_rate=math.log(2) / 2400, division_volume=float('inf'), avogadro=6.02214076e23)
    rc = ref.nonspatial_ref(t, L, kin, 1, env_volume_L=1e-12, avogadro=6.02214076e23, cells=cm)
    with open(FIXTURE) as f:
        rows = {int(float(r['time'])): r for r in csv.DictReader(f)}
    for _ in range(60):
        rc.step(1.0)
    want = float(rows[60]['external_antibiotic'])
    assert rc.conc[3, 0] != want and abs(rc.conc[3, 0] - want) / want < 1e-10


def _death_run(steps=64):
    kin, resp, t, L = _antibiotics({'diffusion': {'permeabilities': {'porin': 0.1}}})
    n = len(ref.DEATH_CASES)
    conc = ref.initial_state(t, L, kin, n)
    assert (conc[0] == 0.5).all()
    conc[L.row(('membrane', 'porin'))] = [c[0] for c in ref.DEATH_CASES]
    env = np.array([[c[1] for c in ref.DEATH_CASES]])
    rc = ref.nonspatial_ref(t, L, kin, n, env_volume_L=1e-12, avogadro=N_A, conc=conc, environment=env)
    hist, mass = [rc.conc.copy()], [rc.m2c.copy()]
    first = [None] * n
    for i in range(1, steps + 1):
        rc.step(1.0)
        hist.append(rc.conc.copy())
        for a in range(n):
            if rc.dead[a] and first[a] is None:
                first[a] = i
    return rc, np.stack(hist), first


def test_death_known_answers():
    rc, hist, first = _death_run()
    assert first == [c[2] for c in ref.DEATH_CASES]
    assert first[:5] == [38, 19, 10, 3, None] and first[5:] == [None] * 6
    for a, row in enumerate(first):
        drug, pump, rna = hist[:, 0, a], hist[:, 1, a], hist[:, 2, a]
        if row is None:
            assert (drug <= 0.95).all() or rc.frozen[a]
            assert pump[-1] != pump[-2]                      # alive: the pump is still being made
            continue
        # detection reads the step-start state, strictly above the threshold, one step late
        assert drug[row - 1] > 0.95 and (drug[:row - 1] <= 0.95).all()
        assert (pump[row:] == pump[row]).all() and (rna[row:] == rna[row]).all()      # frozen, bitwise
        assert (np.diff(drug[row:]) > 0).all()               # the membrane keeps leaking
        assert (rc.counts[:, a] == 0).all()


def test_detection_is_strict():
    kin, resp, t, L = _antibiotics()
    conc = ref.initial_state(t, L, kin, 2)
    conc[0] = [0.95, np.nextafter(0.95, 1.0)]
    conc[4] = 0.0                                            # no porin: nothing leaks
    rc = ref.nonspatial_ref(t, L, kin, 2, env_volume_L=1e-12, avogadro=N_A, conc=conc)
    rc.step(1.0)
    assert rc.dead.tolist() == [0, 1] and rc.frozen.tolist() == [0, 1]
    # the step of detection still applied every update (the pump's RNA was made)
    assert rc.conc[2, 1] == 1e-3
    before = rc.conc[:, 1].copy()
    rc.step(1.0)
    assert np.array_equal(rc.conc[:3, 1], before[:3])
    assert rc.conc[1, 0] == 1e-3 and rc.conc[1, 1] == 0.0    # the live cell translated its RNA, the frozen one not


def test_interleaved_exchange_differs_from_two_passes():
    bva = 1.2e9
    ints, floats = [253513, -376082, -196806], [-27901.266, -219574.982, -58132.208]
    a = ref.interleaved_exchange(1.0, ints, floats, bva)
    b = ref.two_pass_exchange(1.0, ints, floats, bva)
    assert a != b and abs(a - b) < 1e-15


# -- DeathFreezeState in the Experiment loop (death.py:222-339's toy compartment) -----

def test_death_freeze_state_in_the_experiment_loop():
    from lens_amd.engine import Experiment
    from lens_amd.process import Process

    class Injector(Process):
        name = 'toy_antibiotic_injector'

        def __init__(self, parameters=None):
            parameters = parameters or {}
            self.rate = parameters.get('injection_rate', 1.0)
            self.key = parameters.get('antibiotic_name', 'antibiotic')
            super().__init__(parameters)

        def ports_schema(self):
            return {'internal': {self.key: {'_default': 0.0, '_emit': True}}}

        def next_update(self, timestep, states):
            return {'internal': {self.key: timestep * self.rate}}

    death = DeathFreezeState({'detectors': {'antibiotic': {'antibiotic_threshold': 5.0}},
                              'targets': ['injector', 'death']})
    assert death.name == 'death' and death.targets == ['injector', 'death']
    assert death.next_update(1.0, {'internal': {'antibiotic': 5.0}}) == {}
    assert death.next_update(1.0, {'internal': {'antibiotic': 5.5}}) == {
        'global': {'dead': 1}, 'processes': {'_delete': [('injector',), ('death',)]}}
    processes = {'cell_0': {
        'death': death, 'injector': Injector({'injection_rate': 2.0}),
        'enduring_injector': Injector({'injection_rate': 2.0, 'antibiotic_name': 'enduring_antibiotic'})}}
    topology = {'cell_0': {
        'death': {'internal': ('cell',), 'global': ('global',), 'processes': ()},
        'injector': {'internal': ('cell',)}, 'enduring_injector': {'internal': ('cell',)}}}
    exp = Experiment({'processes': processes, 'topology': topology, 'initial_state': {
        'cell_0': {'cell': {'antibiotic': 0.0, 'enduring_antibiotic': 0.0}, 'global': {'dead': 0}}}})
    series = {'antibiotic': [0.0], 'enduring_antibiotic': [0.0], 'dead': [0]}
    for _ in range(10):
        exp.update(1.0)
        s = exp.state['cell_0']
        series['antibiotic'].append(s['cell']['antibiotic'])
        series['enduring_antibiotic'].append(s['cell']['enduring_antibiotic'])
        series['dead'].append(s['global']['dead'])
    # threshold 5, rate 2: death is detected one iteration after the antibiotic exceeds it
    assert series['antibiotic'] == [2.0 * t if t <= 3 else 8.0 for t in range(11)]
    assert series['dead'] == [0 if t <= 3 else 1 for t in range(11)]
    assert series['enduring_antibiotic'] == [2.0 * t for t in range(11)]
    assert list(exp.processes['cell_0']) == ['enduring_injector']


def test_cell_environment_diffusion_schema():
    p = BatchedCellEnvironmentDiffusion(dict(ANTIBIOTICS_DEFAULTS['diffusion']))
    assert p.name == 'cell_environment_diffusion'
    assert p.parameters['permeabilities'] == {'porin': 1e-1}          # permeability_per_porin is not read
    s = p.ports_schema()
    assert s['membrane'] == {'porin': {'_default': 1e-20, '_emit': True}}
    assert s['internal']['antibiotic'] == {'_default': 0.5, '_divider': 'set'}
    assert s['external']['antibiotic'] == {'_default': 1, '_divider': 'set'}
    assert s['global']['volume']['_default'] == 1.2 and s['dimensions']['depth']['_default'] == 1


# -- validation ---------------------------------------------------------------------------

def test_cell_response_validates_its_input():
    ok = ANTIBIOTICS_DEFAULTS
    CellResponse(expression=ok['ode_expression'])
    CellResponse(membrane=ok['diffusion'])
    CellResponse(death={'detectors': ok['death']['detectors']})
    CellResponse(death=ok['death'])                                   # the compartment's own targets
    bad = [
        dict(),
        dict(expression=ok['ode_expression'], cell_ports=()),
        dict(expression=ok['ode_expression'], cell_ports=('internal', 'external')),
        dict(expression={'translation_rates': {'P': 1.0}}),
        dict(expression={'translation_rates': {'P': 1.0}, 'protein_map': {'P': 'M'}}),
        dict(expression=dict(ok['ode_expression'], transcription_leak={'rate': 0.1, 'magnitude': 1e-3})),
        dict(expression=dict(ok['ode_expression'], transcription_rates=[1])),
        dict(membrane={'molecules_to_diffuse': []}),
        dict(membrane={'molecules_to_diffuse': ['a', 'a']}),
        dict(membrane={'molecules_to_diffuse': ['a'], 'permeabilities': {'porin': float('nan')}}),
        dict(death={'detectors': {}}),
        dict(death={'detectors': {'heat': {}}}),
        dict(death={'detectors': {'antibiotic': {'limit': 1.0}}}),
        dict(death={'detectors': {'antibiotic': {'antibiotic_threshold': float('nan')}}}),
        dict(death={'detectors': ok['death']['detectors'], 'targets': ['growth']}),      # the freeze set is fixed
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            CellResponse(**kw)
    with pytest.raises(SyntaxError):
        CellResponse(expression=dict(ok['ode_expression'], regulation={RNA: 'if (external antibiotic'}))


def test_keys_that_resolve_to_no_row_are_refused():
    kin, resp, t, L = _antibiotics()
    with pytest.raises(ValueError, match='detector key'):
        CellResponse(death={'detectors': {'antibiotic': {'antibiotic_key': 'penicillin'}}}).bind(t)
    with pytest.raises(ValueError, match='porin'):
        CellResponse(membrane={'molecules_to_diffuse': ['antibiotic'], 'permeabilities': {'ompF': 0.2},
                               'default_state': {'membrane': {'ompF': 1e-16}}}).bind(t)       # 'porin' has no row
    both = CellResponse(membrane={'molecules_to_diffuse': ['antibiotic'], 'permeabilities': {'ompF': 0.2},
                                  'default_state': {'membrane': {'ompF': 1e-16, 'porin': 2e-16}}}).bind(t)
    assert both.porins == ['porin', 'ompF'] and both.porin_perm.tolist() == [0.1, 0.2]


def test_colony_refusals_come_before_anything_is_built(monkeypatch):
    """Each raises ValueError in Colony.__init__ before the device is touched (this test
    has no GPU: reaching the kinetics engine would raise something else)."""
    from lens_amd import colony as colony_mod
    from lens_amd.lattice import Lattice
    from lens_amd.motility import MotilityModel
    kin, resp, t, L = _antibiotics()

    def lattice(molecules, **kw):
        lat = Lattice.__new__(Lattice)                    # no device: only what the checks read
        lat.molecules = list(molecules)
        lat.pad_top = lat.pad_bot = kw.get('pad', 0)
        lat.edge_top = lat.edge_bot = not kw.get('pad', 0)
        return lat

    def built(*a, **k):
        raise AssertionError('the device was touched before the refusal')

    monkeypatch.setattr(colony_mod, 'KineticsEngine', built)
    monkeypatch.setattr(colony_mod.native, 'resolve_device', built)
    Colony = colony_mod.Colony
    with pytest.raises(ValueError, match='held'):
        Colony(kin, 4, table=t, response=resp)
    with pytest.raises(ValueError, match='held'):
        Colony(kin, 4, table=t, response=resp, environment='held')
    with pytest.raises(ValueError, match='plane'):
        Colony(kin, 4, table=t, response=resp, environment=lattice(['glc__D_e']))
    with pytest.raises(ValueError, match='row bands'):
        Colony(kin, 4, table=t, response=resp, environment=lattice(['antibiotic'], pad=1))
    with pytest.raises(ValueError, match='motility'):
        Colony(kin, 4, table=t, response=resp, environment=lattice(['antibiotic']),
               motility=MotilityModel(ligand_id='antibiotic'))
    with pytest.raises(ValueError, match='detector key'):
        Colony(kin, 4, table=t, environment='nonspatial',
               response=CellResponse(death={'detectors': {'antibiotic': {'antibiotic_key': 'penicillin'}}}))
    with pytest.raises(ValueError, match='CellResponse'):
        Colony(kin, 4, table=t, environment='nonspatial', response={'death': {}})
    with pytest.raises(AssertionError):                   # an accepted colony does go on to build
        Colony(kin, 4, table=t, response=resp, environment='nonspatial')


def test_step_many_run_and_overlapped_capture_are_refused():
    """run(), step_many() and capture(overlap=True) of a colony with a response."""
    from lens_amd.colony import Colony
    kin, resp, t, L = _antibiotics()
    col = Colony.__new__(Colony)                          # no device: the refusals read only these
    col.response, col.cells, col.motility, col.mechanics = resp, None, None, None
    col.environment, col.integrator, col.lattice = 'nonspatial', 'dopri5', object()
    with pytest.raises(ValueError, match='response'):
        col.step_many(1.0, 4)
    with pytest.raises(ValueError, match='response'):
        col.run(2.0)
    lat = type('L', (), dict(pad_top=0, pad_bot=0, edge_top=True, edge_bot=True))()
    col.lattice, col.environment = lat, lat
    with pytest.raises(ValueError, match='response'):
        col.capture(1.0, steps=2, overlap=True)
    with pytest.raises(ValueError, match='response'):
        col.capture(1.0, steps=4, steps_per_launch=2)
    col.router, col.overlap_kinetics = object(), False
    with pytest.raises(ValueError, match='router'):
        col.step(1.0)
