"""Colony(environment=StaticField(...)): the reference's chemotaxis experiment's shape -- agents
that sense an analytic gradient where they are, with the field deriver's one-step lag -- and
the BatchedStaticField drop-in.

Tolerances.  One inner update agrees with the restatement to 3e-12 on the continuous rows
(tests/test_static_motility_gpu.py); a step here is SUBSTEPS inner updates, so after k steps
the bound is k * SUBSTEPS * 3e-12, the scaling the plane colonies' tests use.  The external
row is the field at the agent's position: the kernel's 1e-13 (tests/test_static_field_gpu.py)
plus what the position's own difference moves it by, |d ln L / d y| = ln(1.3e2) / 1000 per um
times the location bound (relative to the 3000-um plane).  Discrete rows are equal where the
restatement's margins hold (asserted on the restatement alone).
"""

import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import motility_ref as mref
import static_field_ref as sref
from lens_amd import configs
from lens_amd.rate_law_compiler import compile_rate_laws

pytestmark = pytest.mark.gpu

N, STEPS, SUBSTEPS, SEED = 24, 10, 10, 20261020
LIGAND = 'glc__D_e'


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _colony(dev, kind='exponential', motile=True, integrator='dopri5', n=N, **motility):
    from lens_amd.colony import Colony
    cfg = configs.glc_lct_config()
    c = configs.chemotaxis_static(kind, n_agents=n, seed=SEED, substeps=SUBSTEPS, **motility)
    col = Colony(cfg, n, capacity=n + 5, device=dev, integrator=integrator, environment=c['field'],
                 motility=c['motility'] if motile else None)
    col.set_agents(location=c['location'])
    return col, c


def _ext_row(col):
    return col.table.species.index(('external', LIGAND))


def test_motile_colony_follows_the_restated_loop(dev):
    col, c = _colony(dev)
    field, model = c['field'], c['motility']
    motil = model.initial_rows(N, N)
    loc = c['location'].copy()
    row = _ext_row(col)
    assert torch.equal(col.motil[:, :N].cpu(), torch.from_numpy(motil))
    # the derivers ran at t = 0: every agent's external is the reference's INITIAL_LIGAND
    assert np.all(col.conc[row, :N].cpu().numpy() == 4.0 * 1.3e2 ** (300 / 1000))
    margins = {}
    for k in range(STEPS):
        col.step(1.0)
        bins = sref.motility_step(model, field, motil, loc, 1.0, SUBSTEPS, SUBSTEPS * k, margins=margins)
        assert margins['switch'] >= 1e-9 and margins['edge'] >= 1e-9, margins
        tol = (k + 1) * SUBSTEPS * 3e-12
        got_m, got_l = col.motil[:, :N].cpu().numpy(), col.location[:, :N].cpu().numpy()
        for name in ('motor_state', 'thrust'):
            assert np.array_equal(got_m[mref.R[name]], motil[mref.R[name]]), (k, name)
        assert np.array_equal(col.bin_lin[:N].cpu().numpy(), bins), k
        for name in ('n_methyl', 'chemoreceptor_activity', 'CheY_P', 'ccw_motor_bias', 'ccw_to_cw'):
            r = mref.R[name]
            assert np.max(np.abs(got_m[r] - motil[r]) / np.abs(motil[r])) <= tol, (k, name)
        for name in ('angle', 'torque'):
            assert np.max(np.abs(got_m[mref.R[name]] - motil[mref.R[name]])) <= tol, (k, name)
        assert np.max(np.abs(got_l - loc) / np.array(field.bounds)[:, None]) <= tol, k
        want = sref._ligand(field, LIGAND, loc)
        ext = col.conc[row, :N].cpu().numpy()
        assert np.max(np.abs(ext / want - 1)) <= 1e-13 + np.log(1.3e2) / 1000 * tol * 3000, k
        # and exactly the field at the colony's own positions, to the kernel's bound
        assert np.max(np.abs(ext / sref._ligand(field, LIGAND, got_l) - 1)) <= 1e-13, k
    col.check_status()
    assert int(col._motil_counter[0]) == STEPS * SUBSTEPS
    assert float((col.location[:, :N].cpu() - torch.from_numpy(c['location'])).abs().max()) > 10.0
    assert bool((col.motil[:, N:] == 0).all()) and bool((col.location[:, N:] == 0).all())


def test_kinetics_reads_the_field_one_step_late(dev):
    """Step k's fluxes come from the external the gather left at the end of step k - 1 -- the
    field where step k - 1's move ended -- not from where step k's move ends."""
    from lens_amd.colony import Colony
    col, c = _colony(dev, integrator='euler')
    field = c['field']
    row = _ext_row(col)
    held = Colony(configs.glc_lct_config(), N, capacity=N + 5, device=dev, integrator='euler', environment='held')
    for k in range(4):
        before = col.conc.clone()
        loc_before = col.location[:, :N].cpu().numpy()
        # what the last gather left: the field at the position the agents are at now
        assert np.max(np.abs(before[row, :N].cpu().numpy() / sref._ligand(field, LIGAND, loc_before) - 1)) <= 1e-13
        col.step(1.0)
        held.conc.copy_(before)
        held.step(1.0)
        assert torch.equal(col.flux, held.flux), k
        assert bool((col.flux[:, :N] != 0).any())
        # a gather between the move and the kinetics would have fed the kinetics this instead
        late = before.clone()
        late[row] = col.conc[row]
        assert not torch.equal(late[row, :N], before[row, :N])
        held.conc.copy_(late)
        held.step(1.0)
        assert not torch.equal(col.flux, held.flux), k
        # the gather ran after the move: the external is the field at the new position
        loc_after = col.location[:, :N].cpu().numpy()
        assert np.max(np.abs(col.conc[row, :N].cpu().numpy() / sref._ligand(field, LIGAND, loc_after) - 1)) <= 1e-13
        assert np.abs(loc_after - loc_before).max() > 1.0


@pytest.mark.parametrize('flagella', [False, True])
def test_captured_steps_equal_plain_steps(dev, flagella):
    from lens_amd.motility import FlagellaModel
    kw = {'flagella': FlagellaModel(5)} if flagella else {}
    (a, _), (b, _) = _colony(dev, **kw), _colony(dev, **kw)
    a.step(1.0)
    b.step(1.0)
    layout = b._layout
    replay = b.capture(1.0, 1)
    torch.cuda.synchronize()
    names = ('conc', 'counts', 'flux', 'location', 'motil', 'bin_lin') + (('flag', 'flag_int') if flagella else ())
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), ('capture ran nothing', name)
    for _ in range(5):
        a.step(1.0)
        replay()
    torch.cuda.synchronize()
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert b._layout == layout and int(b._motil_counter[0]) == 6 * SUBSTEPS and b.step_index == 6
    # positions set between replays are seen: buffers and layout stay
    b.set_agents(location=np.full((2, N), 123.0))
    assert b._layout == layout


def test_non_motile_colony_keeps_the_field_of_its_positions(dev):
    col, c = _colony(dev, kind='linear', motile=False)
    field = c['field']
    row = _ext_row(col)
    rng = np.random.default_rng(SEED)
    loc = np.stack([rng.uniform(0, 1000, N), rng.uniform(0, 3000, N)])
    col.set_agents(location=loc)                       # regathers
    want = sref._ligand(field, LIGAND, loc)
    assert np.array_equal(col.conc[row, :N].cpu().numpy(), want)          # linear: bitwise
    lcts = col.conc[col.table.species.index(('external', 'lcts_e'))].clone()
    for _ in range(3):
        col.step(1.0)
    assert np.array_equal(col.conc[row, :N].cpu().numpy(), want)
    assert np.array_equal(col.location[:, :N].cpu().numpy(), loc)
    # a molecule without a gradient is never written; padding columns neither
    assert torch.equal(col.conc[col.table.species.index(('external', 'lcts_e'))], lcts)
    assert bool((col.conc[row, N:] == col.conc[row, N:][0]).all())
    bins = (mref.bin_axis(loc[0], 10, 1000.0) * 10 + mref.bin_axis(loc[1], 10, 3000.0)).astype(np.int32)
    assert np.array_equal(col.bin_lin[:N].cpu().numpy(), bins)


def test_static_colony_refuses_the_lattice_schedulers(dev):
    col, _ = _colony(dev, n=4)
    with pytest.raises(ValueError, match='StaticField steps with step'):
        col.run(1.0)
    with pytest.raises(ValueError, match='step_many'):
        col.step_many(1.0, 2)
    with pytest.raises(ValueError, match='row-banded'):
        col.capture_banded(1.0)


def test_batched_static_field_returns_the_references_update(dev):
    from lens_amd.process import BatchedStaticField
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gradients.npz'))
    for kind in sref.FIELD_TYPES:
        p = BatchedStaticField({'molecules': ['a', 'b', 'c'], 'bounds': list(sref.POINT_BOUNDS),
                                'gradient': sref.POINTS[kind], 'device': dev})
        assert p.name == 'static_field'
        schema = p.ports_schema()
        assert list(schema) == ['agents'] and list(schema['agents']) == ['*']
        leaf = schema['agents']['*']['boundary']
        assert leaf['location'] == {'_default': [500.0, 1500.0], '_updater': 'set'}
        assert leaf['external'] == {m: {'_default': 0.0, '_updater': 'set'} for m in 'abc'}
        ids = ['x', 'y', 'z']
        states = {'agents': {a: {'boundary': {'location': z['points'][:, i].tolist(), 'external': {}}}
                             for i, a in enumerate(ids)}}
        update = p.next_update(1.0, states)
        assert list(update) == ['agents'] and list(update['agents']) == ids
        for i, a in enumerate(ids):
            assert list(update['agents'][a]) == ['boundary'] and list(update['agents'][a]['boundary']) == ['external']
            ext = update['agents'][a]['boundary']['external']
            assert list(ext) == ['a', 'b']                       # the gradient's molecules only
            for j, m in enumerate('ab'):
                want = z['points_' + kind][j, i]
                assert isinstance(ext[m], float)
                if kind == 'linear':
                    assert ext[m] == want
                else:
                    assert abs(ext[m] / want - 1) <= 1e-13
        assert p.next_update(1.0, {'agents': {}}) == {'agents': {}}
