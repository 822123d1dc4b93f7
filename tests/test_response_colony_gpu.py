"""Colony(response=CellResponse(...)): the antibiotic-response cell on the device,
against the reference's golden file and the NumPy restatement, bit for bit.

Settings of the golden twin (the reference's lone Antibiotics compartment in a
NonSpatialEnvironment): Euler, environment volume 1e-12 L, the legacy N_A,
division_volume = inf (the lone compartment has no MetaDivision: it raises
``divide`` at row 2352 and keeps growing, so ``global_divide`` is not compared;
``fluxes_import`` is not a quantity this engine carries)."""

import csv
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import response_ref as ref
from lens_amd import native
from lens_amd.rate_law_compiler import compile_rate_laws
from oracle import lattice as olat

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'antibiotics_compartment_subset.csv')
N_A = 6.022140857e23
RNA = 'AcrAB-TolC_RNA'


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _antibiotics(config=None):
    from lens_amd.response import from_antibiotics
    kin, resp = from_antibiotics(config)
    t = compile_rate_laws(kin['reactions'], kin['kinetic_parameters'])
    return kin, resp, t


def golden_columns(snap, a=0):
    """The fixture's columns from a snapshot (volume is emitted in litres there)."""
    g = snap['global']
    return {
        'global_mass': g['mass'][a], 'global_volume': g['volume'][a] * 1e-15, 'global_width': float(g['width'][a]),
        'global_length': g['length'][a], 'global_surface_area': g['surface_area'][a],
        'global_dead': float(g['dead'][a]), 'cell_counts_AcrAB-TolC_RNA': snap['cell_counts'][RNA][a],
        'cell_counts_AcrAB-TolC': snap['cell_counts']['AcrAB-TolC'][a], 'cell_AcrAB-TolC_RNA': snap['internal'][RNA][a],
        'cell_AcrAB-TolC': snap['pump_port']['AcrAB-TolC'][a], 'cell_antibiotic': snap['internal']['antibiotic'][a],
        'cell_porin': snap['membrane']['porin'][a], 'external_antibiotic': snap['external']['antibiotic'][a],
    }


def test_golden_twin_matches_every_fixture_row(dev):
    from lens_amd.cells import CellModel
    from lens_amd.colony import Colony
    kin, resp, t = _antibiotics()
    cm = CellModel(model='growth', growth_rate=math.log(2) / 2400, division_volume=float('inf'))
    col = Colony(kin, 1, device=dev, integrator='euler', environment='nonspatial', env_volume_L=1e-12, avogadro=N_A,
                 table=t, cells=cm, response=resp)
    with open(FIXTURE) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 162 and float(rows[-1]['time']) == 2400.0
    step = 0
    bad = []
    for row in rows:
        while step < int(float(row['time'])):
            col.step(1.0)
            step += 1
        got = golden_columns(col.snapshot())          # read back only at fixture rows
        assert float(row['time']) == col.time
        for name, value in got.items():
            if float(row[name]) != value:
                bad.append((step, name, row[name], repr(value)))
    col.check_status()
    assert not bad, bad[:5]
    assert col.n == 1 and int(col.dead[0]) == 0


def _death_batch(dev, steps=64):
    from lens_amd.colony import Colony
    kin, resp, t = _antibiotics({'diffusion': {'permeabilities': {'porin': 0.1}}})
    L = resp.bind(t)
    n = len(ref.DEATH_CASES)
    conc = ref.initial_state(t, L, kin, n)
    conc[L.row(('membrane', 'porin'))] = [c[0] for c in ref.DEATH_CASES]
    env = np.array([[c[1] for c in ref.DEATH_CASES]])
    col = Colony(kin, n, capacity=n + 3, device=dev, integrator='euler', environment='nonspatial', env_volume_L=1e-12,
                 avogadro=N_A, table=t, response=resp)
    col.set_agents(conc=conc, environment=env)
    rc = ref.nonspatial_ref(t, L, kin, n, env_volume_L=1e-12, avogadro=N_A, conc=conc, environment=env)
    return col, rc, L


def test_death_batch_rows_freeze_and_leak(dev):
    col, rc, L = _death_batch(dev)
    n = col.n
    first = [None] * n
    pump, rna, drug = L.row(('pump_port', 'AcrAB-TolC')), L.row(('internal', RNA)), L.row(('internal', 'antibiotic'))
    history = []
    for i in range(1, 65):
        col.step(1.0)
        rc.step(1.0)
        conc = col.conc[:, :n].cpu().numpy()
        assert np.array_equal(conc, rc.conc), i
        assert np.array_equal(col.env_fields[:, :n].cpu().numpy(), rc.fields), i
        assert np.array_equal(col.dead[:n].cpu().numpy(), rc.dead), i
        assert np.array_equal(col.frozen[:n].cpu().numpy(), rc.frozen), i
        assert np.array_equal(col.counts[:, :n].cpu().numpy(), rc.counts), i
        assert np.array_equal(col.flux[:, :n].cpu().numpy(), rc.flux), i
        history.append(conc)
        for a in range(n):
            if rc.dead[a] and first[a] is None:
                first[a] = i
    assert first == [c[2] for c in ref.DEATH_CASES]
    assert np.array_equal(col.snapshot()['global']['dead'], rc.dead)
    for a, row in enumerate(first):
        if row is None:
            continue
        after = np.stack([h[:, a] for h in history[row - 1:]])        # rows first-dead .. 64
        assert (after[:, pump] == after[0, pump]).all() and (after[:, rna] == after[0, rna]).all()
        assert (np.diff(after[:, drug]) > 0).all()                    # the membrane keeps leaking
        assert (col.counts[:, a] == 0).all()


# -- a lattice colony: cells, mechanics, division, several agents per bin -------------

NX, BOUND, DEPTH, DIFFUSION = 8, 16.0, 2.0, 3.0
N_LAT, CAP_LAT, STEPS_LAT = 40, 44, 10


def _lattice(dev, seed=2):
    from lens_amd.lattice import Lattice
    rng = np.random.default_rng(seed)
    start = {'antibiotic': rng.uniform(0.8, 2.5, (NX, NX)), 'spare': rng.uniform(0.0, 1.0, (NX, NX))}
    return Lattice(['spare', 'antibiotic'], (NX, NX), (BOUND, BOUND), DEPTH, DIFFUSION, device=dev, avogadro=N_A,
                   initial=start), start


def _lattice_colony(dev, exchange, response=True, cells=True, mechanics=True, n=N_LAT, capacity=CAP_LAT):
    from lens_amd.cells import CellModel
    from lens_amd.colony import Colony
    from lens_amd.mechanics import ContactModel
    kin, resp, t = _antibiotics({'diffusion': {'permeabilities': {'porin': 0.1}}})
    L = resp.bind(t)
    rng = np.random.default_rng(23)
    lat, start = _lattice(dev)
    cm = CellModel(model='growth', growth_rate=0.02) if cells else None
    mech = ContactModel(seed=5, jitter=0.01, jitter_angle=0.02, max_length=5.0) if mechanics else None
    col = Colony(kin, n, capacity=capacity, device=dev, integrator='euler', environment=lat, avogadro=N_A, table=t,
                 exchange=exchange, cells=cm, mechanics=mech, response=resp if response else None)
    conc = ref.initial_state(t, L, kin, n) if response else None
    loc = 5.0 + rng.uniform(0.0, 6.0, (2, n))                         # 40 agents over 3 x 3 bins of 2 um
    if response:
        conc[L.row(('membrane', 'porin'))] = rng.uniform(1e-16, 3e-15, n)
        conc[L.row(('internal', 'antibiotic'))] = rng.uniform(0.3, 0.9, n)
        conc[L.row(('pump_port', 'AcrAB-TolC'))] = rng.uniform(0.0, 0.5, n)
        conc[L.row(('internal', 'antibiotic')), 3] = 0.97             # agent 3: dying in the step it divides
        col.set_agents(conc=conc, location=loc)
    else:
        col.set_agents(location=loc)
    if cells:
        mass = rng.uniform(1400.0, 2300.0, n)
        mass[::4] = rng.uniform(2400.0, 2635.0, len(mass[::4]))       # within 5 steps of 2.4 fL at 2 % a step
        mass[3] = 2650.0                                              # divides in the first step
        col.set_cell_mass(mass)
        col.cell[native.VK_CELL_ANGLE, :n] = torch.from_numpy(rng.uniform(0.0, 2.0 * np.pi, n)).to(dev)
    col.gather_external()
    return col, (t, L, kin, start)


def _ref_of(col, t, L, start):
    """The restatement started from the colony's initial state (inputs, not results)."""
    n = col.n
    lat = col.lattice
    fields = np.stack([start[m].reshape(-1) for m in lat.molecules])
    plane = lat.molecules.index('antibiotic')
    rc = ref.RefColony(t, L, col.conc[:, :n].cpu().numpy(), col.params[:, :n].cpu().numpy(), col.m2c[:n].cpu().numpy(),
                       avogadro=N_A, bva=lat.binvol_avogadro, fields=fields, bins=col.bin_lin[:n].cpu().numpy(),
                       gather=[(plane, int(L.mol_ext_row[0]))], exch_int=[(0, plane)], exch_float=[(0, plane)],
                       cells=(col.cells, col.cell[:, :n].cpu().numpy()), nonspatial=False)
    return rc


def _diffuse(rc):
    for f in range(rc.fields.shape[0]):
        rc.fields[f] = olat.diffuse(rc.fields[f].reshape(NX, NX), 1.0, DIFFUSION, (NX, NX), (BOUND, BOUND)).reshape(-1)


def _run_lattice(dev, exchange):
    col, (t, L, kin, start) = _lattice_colony(dev, exchange)
    rc = _ref_of(col, t, L, start)
    assert col.map_exch_count.numel() == 1 and col.map_fexch_count.numel() == 1
    # the bins of the exchange are the contact launch's (mechanics has its own reference):
    # the restatement takes them from the colony at the moment of the exchange
    seen = {}
    exchange_fn = col._step_exchange

    def spy():
        seen['bins'] = col.bin_lin[:col.n].cpu().numpy().astype(np.int64)
        exchange_fn()

    col._step_exchange = spy
    ns, lds, shared = [col.n], [col.ld], 0
    for i in range(STEPS_LAT):
        col.step(1.0)
        rc.bins = seen['bins']
        shared = max(shared, int(np.bincount(rc.bins).max()))
        rc.step(1.0, between=_diffuse)
        rc.apply_division()
        n = col.n
        assert n == rc.n, i
        got = {name: getattr(col, name)[..., :n].cpu().numpy() for name in ('conc', 'm2c', 'dead', 'frozen', 'counts',
                                                                             'flux', 'divide')}
        got['growth'] = col.cell[:5, :n].cpu().numpy()          # mass .. protein; the angle is the contact launch's
        planes = np.stack([col.lattice.owned(m).cpu().numpy().reshape(-1) for m in col.lattice.molecules])
        yield i, got, planes, rc
        ns.append(n)
        lds.append(col.ld)
    col.check_status()
    yield 'end', (ns, lds, shared), None, rc


def test_lattice_colony_with_cells_and_mechanics_sorted(dev):
    for i, got, planes, rc in _run_lattice(dev, 'sorted'):
        if i == 'end':
            ns, lds, shared = got
            break
        for name, value in got.items():
            assert np.array_equal(value, rc.cell[:5] if name == 'growth' else getattr(rc, name)), (i, name)
        assert np.array_equal(planes, rc.fields), i
        if i == 0:
            # agent 3 was detected dying in the step it divided: its daughters (the last two
            # columns) are dead and not frozen ...
            assert rc.n > N_LAT and list(rc.dead[-2:]) == [1, 1] and list(rc.frozen[-2:]) == [0, 0]
        if i == 1:
            # ... they ran one more step and were detected again
            k = [a for a in range(rc.n) if rc.dead[a]]
            assert len(k) >= 2 and all(rc.frozen[a] for a in k)
    print('n per step', ns, 'ld', lds, 'most agents in a bin', shared)
    assert ns[-1] >= ns[0] + N_LAT // 5
    assert lds[0] == CAP_LAT and lds[-1] > CAP_LAT                   # through a reallocation of ld
    assert shared >= 3                                               # several agents per bin
    assert rc.frozen.sum() >= 2 and (rc.frozen == 0).sum() > 0


def test_lattice_colony_atomic_within_the_atomic_bound(dev):
    for i, got, planes, rc in _run_lattice(dev, 'atomic'):
        if i == 'end':
            break
        # the planes within the atomic exchange's bound (tests/test_gpu_parity.py), per step; agents
        # see them through the gather, so their state is compared at that bound too
        np.testing.assert_allclose(planes, rc.fields, rtol=1e-14 * (i + 1), atol=0)
        for name in ('dead', 'frozen', 'divide', 'counts'):
            assert np.array_equal(got[name], getattr(rc, name)), (i, name)
        np.testing.assert_allclose(got['conc'], rc.conc, rtol=1e-14 * (i + 1), atol=0)
        assert np.array_equal(got['growth'], rc.cell[:5])


def _capture_colony(dev):
    col, _ = _lattice_colony(dev, 'sorted', cells=False, n=60, capacity=64)
    return col


def test_three_replays_of_four_steps_equal_twelve_eager_steps(dev):
    a, b = _capture_colony(dev), _capture_colony(dev)
    assert torch.equal(a.conc, b.conc) and torch.equal(a.location, b.location)
    replay = a.capture(1.0, steps=4)
    for _ in range(3):
        replay()
    for _ in range(12):
        b.step(1.0)
    torch.cuda.synchronize()
    n = a.n
    for name in ('conc', 'dead', 'frozen', 'counts', 'flux', 'location', 'bin_lin', 'mech_angle'):
        assert torch.equal(getattr(a, name)[..., :n], getattr(b, name)[..., :n]), name
    for m in a.lattice.molecules:
        assert torch.equal(a.lattice.owned(m), b.lattice.owned(m)), m
    assert a.time == b.time == 12.0
    assert int(b.dead[:n].sum()) > 0 and int(b.dead[:n].sum()) < n    # the replayed steps froze some agents
    with pytest.raises(ValueError):
        a.capture(1.0, steps=2, overlap=True)


def test_a_colony_without_response_is_unchanged(dev):
    a, _ = _lattice_colony(dev, 'sorted', response=False)
    b, _ = _lattice_colony(dev, 'sorted', response=False)
    assert a.agent_array_names() == ['params', 'conc', 'm2c', 'flux', 'counts', 'status', 'nsteps', 'h_state',
                                     'location', 'cell', 'divide', 'lin_root', 'lin_depth', 'lin_path']
    assert a.response is None and not hasattr(a, 'dead') and not hasattr(a, '_resp_buf')
    assert a.conc.shape[0] == a.table.n_species
    assert a._kin_conc() is a.conc
    with_r, _ = _lattice_colony(dev, 'sorted')
    assert with_r.agent_array_names() == a.agent_array_names()[:-5] + ['cell', 'divide', 'lin_root', 'lin_depth',
                                                                      'lin_path', 'dead', 'frozen']
    for i in range(4):
        a.step(1.0)
        b.step(1.0)
    n = a.n
    assert n == b.n
    for name in a.agent_array_names():
        assert torch.equal(getattr(a, name)[..., :n], getattr(b, name)[..., :n]), name
    # the exchange of a colony without response: the antibiotic export's int counts alone
    assert 'cell_counts' not in a.snapshot() and 'dead' not in a.snapshot()['global']
