"""Colony(motility=MotilityModel(flagella=...)): the multi-flagellar motor in a colony's
step.  The step must equal, bit for bit, the ABI sequence -- the flagella launch on a
plain colony's arrays, ``refresh_bins()``, ``step()`` --, must not depend on the storage
order of the agents, must replay from a captured graph with ``set_flagella`` between
replays, and ``remove()`` must carry the flagella arrays.  ``flagella=None`` is the
coarse motor's path, array for array.

Setup: glc_lct kinetics (DP45) and a MeAsp plane on 32 x 32 bins of 2 um, 600 agents
with 0..32 flagella, steps of 0.25 s in 25 inner updates of the reference's 0.01 s."""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from lens_amd import configs
from lens_amd.rate_law_compiler import compile_rate_laws

pytestmark = pytest.mark.gpu

N, NX, BOUND, DT = 600, 32, 64.0, 0.25
NAMES = ('conc', 'counts', 'flux', 'location', 'motil', 'flag', 'flag_int', 'bin_lin')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _counts():
    return np.arange(N) % 33


def _model(flagella=True):
    from lens_amd.motility import FlagellaModel, MotilityModel
    return MotilityModel(initial_ligand=1e-2, substeps=25, seed=11,
                         flagella=FlagellaModel(_counts()) if flagella else None)


def _colony(dev, motility='flagella', **kw):
    from lens_amd.colony import Colony
    from lens_amd.lattice import Lattice
    cfg = configs.glc_lct_config()
    t = compile_rate_laws(cfg['reactions'], cfg['kinetic_parameters'])
    rng = np.random.default_rng(17)
    x = np.linspace(0.0, 1.0, NX)
    start = {'glc__D_e': configs.gaussian_bump_field((NX, NX)), 'lcts_e': np.full((NX, NX), 10.0),
             'MeAsp': 0.2 * x[:, None] + 0.05 * x[None, :] ** 2}
    lat = Lattice(['glc__D_e', 'lcts_e', 'MeAsp'], (NX, NX), (BOUND, BOUND), 10.0, 5.0, device=dev, initial=start)
    params, conc = configs.heterogeneous_colony(t, cfg, N)
    loc = rng.uniform(0.0, BOUND, (2, N))
    loc[0, :100] = 31.0                              # a crowd in three neighbouring bins
    loc[1, :100] = 21.0 + 2.0 * (np.arange(100) % 3)
    if motility == 'flagella':
        kw['motility'] = _model()
    elif motility == 'coarse':
        kw['motility'] = _model(flagella=False)
    elif motility == 'coarse, no argument':
        from lens_amd.motility import MotilityModel
        kw['motility'] = MotilityModel(initial_ligand=1e-2, substeps=25, seed=11)
    col = Colony(cfg, N, device=dev, integrator='dopri5', environment=lat, table=t, **kw)
    col.set_agents(params=params, conc=conc, location=loc)
    col.gather_external()
    return col


def _same(a, b, names, where, perm=None):
    n = a.n
    assert a.n == b.n, where
    for m in a.lattice.molecules:
        assert torch.equal(a.lattice.owned(m), b.lattice.owned(m)), (where, m)
    for name in names:
        x, y = getattr(a, name)[..., :n], getattr(b, name)[..., :n]
        if perm is not None:
            x = x[..., perm]
        assert torch.equal(x, y), (where, name)


def test_flagella_step_equals_the_abi_sequence(dev):
    from lens_amd.motility import flagella_step
    a, b = _colony(dev), _colony(dev, motility=None)
    model = _model()
    b.motil = torch.from_numpy(model.initial_rows(N, b.ld)).to(dev).contiguous()
    flag, flag_int = model.flagella.initial_rows(N, b.ld, model.seed)
    b.flag, b.flag_int = torch.from_numpy(flag).to(dev), torch.from_numpy(flag_int).to(dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    assert torch.equal(a.motil, b.motil) and torch.equal(a.flag, b.flag) and torch.equal(a.flag_int, b.flag_int)
    assert a.flag_int.dtype == torch.int32 and a.flag.dtype == torch.float64
    layout = a._layout
    loc0 = a.location.clone()
    for step in range(3):
        a.step(DT)
        flagella_step(model, b.lattice, b.location, b.motil, b.flag, b.flag_int, N, DT, counter)
        b.refresh_bins()
        b.step(DT)
        torch.cuda.synchronize()
        _same(a, b, NAMES, step)
    a.check_status()
    assert a._layout == layout and int(a._motil_counter[0]) == int(counter[0]) == 75
    names = a.agent_array_names()
    assert 'motil' in names and 'flag' in names and 'flag_int' in names
    snap = a.snapshot()
    assert sorted(snap['flagella']) == sorted(('CheY', 'CheY_P', 'cw_bias', 'motile_state', 'PMF', 'target', 'have',
                                               'mask'))
    assert np.array_equal(snap['flagella']['have'], _counts()) and snap['flagella']['mask'].dtype == np.uint32
    assert set(np.unique(snap['flagella']['motile_state'])) == {-1.0, 0.0, 1.0}
    assert np.array_equal(snap['motility']['motor_state'], (snap['flagella']['mask'] != 0).astype(np.float64))
    assert np.array_equal(snap['flagella']['motile_state'] == 0, _counts() == 0)
    # the coarse motor's rows are not touched; agents without flagella stand still, the others moved
    m0 = model.initial_rows(N, a.ld)
    for row in ('CheY_P', 'ccw_motor_bias', 'ccw_to_cw'):
        assert np.array_equal(snap['motility'][row], m0[('n_methyl', 'chemoreceptor_activity', 'CheY_P',
                                                        'ccw_motor_bias', 'ccw_to_cw').index(row), :N])
    moved = (a.location[:, :N] - loc0[:, :N]).abs().max(0).values.cpu().numpy()
    assert (moved[_counts() == 0] == 0).all() and (moved[_counts() >= 2] > 0).all()


def test_flagella_step_does_not_depend_on_storage_order(dev):
    a, b = _colony(dev), _colony(dev)
    order = b.sort_by_bin()
    assert not torch.equal(order, torch.arange(N, device=dev))
    assert torch.equal(a.flag_int[:, order], b.flag_int[:, :N])
    for step in range(3):
        a.step(DT)
        b.step(DT)
    torch.cuda.synchronize()
    _same(a, b, NAMES, 'sorted twin', perm=order)


def _new_counts(kind, dev):
    if kind == 'int':
        return 3
    counts = (_counts()[::-1] * 7) % 33              # every agent another count: growth and shrinkage
    if kind == 'host':
        return counts
    return torch.from_numpy(counts.astype(np.int32)).to(dev)


@pytest.mark.parametrize('kind', [None, 'int', 'host', 'device'])
def test_captured_steps_equal_eager_steps(dev, kind):
    """After one eager step each: capture(dt, 3) replayed twice equals six eager steps;
    with set_flagella between the two replays, the same call between eager steps 3 and 4."""
    a, b = _colony(dev), _colony(dev)
    a.step(DT)
    b.step(DT)
    replay = b.capture(DT, 3)
    flag_int = b.flag_int
    torch.cuda.synchronize()
    _same(a, b, ('conc', 'location', 'motil', 'flag', 'flag_int'), 'capture ran nothing')
    for step in range(6):
        if step == 3 and kind is not None:
            a.set_flagella(_new_counts(kind, dev))
        a.step(DT)
    replay()
    if kind is not None:
        b.set_flagella(_new_counts(kind, dev))
    replay()
    torch.cuda.synchronize()
    _same(a, b, NAMES, 'replayed')
    assert b.flag_int is flag_int                        # copied into the tensor the graph holds
    assert int(b._motil_counter[0]) == 175 and b.step_index == 7
    if kind is not None:
        want = np.full(N, 3) if kind == 'int' else (_counts()[::-1] * 7) % 33
        assert np.array_equal(b.flag_int[:2, :N].cpu().numpy(), np.stack([want, want]))
        assert not np.array_equal(want, _counts())
    with pytest.raises(ValueError, match='overlap'):
        b.capture(DT, 1, overlap=True)


def test_remove_keeps_the_flagella_arrays_with_their_agents(dev):
    a = _colony(dev)
    a.step(DT)
    a.flag[4, :N] = torch.arange(N, dtype=torch.float64, device=dev) + 50.0          # PMF: a tag per agent
    mask = torch.zeros(N, dtype=torch.int32, device=dev)
    mask[::3] = 1
    keep = torch.nonzero(mask == 0).flatten()
    before = {name: getattr(a, name)[..., keep].clone() for name in ('flag', 'flag_int', 'motil', 'location')}
    assert a.remove(mask) == 200 and a.n == 400
    for name, want in before.items():
        assert torch.equal(getattr(a, name)[..., :400], want), name
        assert getattr(a, name).shape[-1] == a.ld
    assert a.flag_int.dtype == torch.int32
    a.step(DT)                                           # and the colony steps on
    torch.cuda.synchronize()
    a.check_status()
    assert torch.equal(a.flag[4, :400], keep.to(torch.float64) + 50.0)


def test_every_refusal_raises(dev):
    from lens_amd.cells import CellModel
    from lens_amd.colony import Colony
    from lens_amd.distributed import AgentRouter
    from lens_amd.lattice import Lattice
    from lens_amd.mechanics import ContactModel
    from lens_amd.motility import FlagellaModel, MotilityModel
    from lens_amd.response import ANTIBIOTICS_DEFAULTS, CellResponse
    cfg = configs.glc_lct_config()
    m = _model()
    lattice = lambda **kw: Lattice(['glc__D_e', 'lcts_e', 'MeAsp'], (8, 8), (8.0, 8.0), 10.0, 5.0, device=dev, **kw)
    mk = lambda **kw: Colony(cfg, 4, device=dev, motility=MotilityModel(flagella=FlagellaModel(5)), **kw)
    with pytest.raises(ValueError, match='Lattice environment'):
        mk(environment='held')
    with pytest.raises(ValueError, match='unbanded'):
        mk(environment=lattice(row_band=(0, 4), halo=1))
    with pytest.raises(ValueError, match='cells'):
        mk(environment=lattice(), cells=CellModel())
    with pytest.raises(ValueError, match='mechanics with motility'):
        mk(environment=lattice(), mechanics=ContactModel())
    with pytest.raises(ValueError, match='response with motility'):
        mk(environment=lattice(), response=CellResponse(membrane=ANTIBIOTICS_DEFAULTS['diffusion']))
    a = _colony(dev)
    with pytest.raises(ValueError, match='router'):
        AgentRouter(a, 0, 1, agent_offset=0)
    with pytest.raises(ValueError, match='overlap'):
        a.capture(DT, 1, overlap=True)
    with pytest.raises(ValueError, match='step\\(\\)'):
        a.run(1.0)
    for bad in (33, -1, np.full(N, 40), np.arange(N - 1) % 3, 2.5):
        with pytest.raises(ValueError):
            a.set_flagella(bad)
    with pytest.raises(ValueError, match='int32'):
        a.set_flagella(torch.zeros(N, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match='set_flagella'):
        _colony(dev, motility='coarse').set_flagella(5)
    assert np.array_equal(a.flag_int[0, :N].cpu().numpy(), _counts())                # nothing was written


def test_flagella_none_is_the_coarse_path(dev):
    """A colony built with flagella=None produces the same arrays as one built without
    the argument, and has none of the flagella arrays."""
    a, b = _colony(dev, motility='coarse'), _colony(dev, motility='coarse, no argument')
    for _ in range(3):
        a.step(DT)
        b.step(DT)
    torch.cuda.synchronize()
    _same(a, b, ('conc', 'counts', 'flux', 'location', 'motil', 'bin_lin'), 'flagella=None')
    assert a.agent_array_names() == b.agent_array_names() and 'flag' not in a.agent_array_names()
    assert not hasattr(a, 'flag') and not hasattr(a, 'flag_int') and 'flagella' not in a.snapshot()
    assert set(np.unique(a.snapshot()['motility']['thrust'])) <= {100.0, 250.0}
