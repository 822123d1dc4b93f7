"""Colony.remove(mask): agents leave the colony on the device.

After a removal every per-agent array must equal NumPy's compaction of what it
held, bit for bit, and the colony's next step must equal that of a fresh colony
set to the compacted state -- on a lattice colony, on a nonspatial response
colony that drops its dead, and on a motile colony (its ``motil`` rows, its bins
and the device occupancy).  An all-zero mask changes nothing, an all-one mask
leaves an empty colony that still steps, and a routed colony refuses."""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import response_ref
from lens_amd import configs
from lens_amd.rate_law_compiler import compile_rate_laws

pytestmark = pytest.mark.gpu

NX, BOUND, N = 64, 128.0, 1500
N_A = 6.022140857e23


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _lattice_colony(dev, n=N, motile=False):
    from lens_amd.colony import Colony
    from lens_amd.lattice import Lattice
    from lens_amd.motility import MotilityModel
    cfg = configs.glc_lct_config()
    t = compile_rate_laws(cfg['reactions'], cfg['kinetic_parameters'])
    x = np.linspace(0.0, 1.0, NX)
    start = {'glc__D_e': configs.gaussian_bump_field((NX, NX)), 'lcts_e': np.full((NX, NX), 10.0),
             'MeAsp': 0.2 * x[:, None] + 0.05 * x[None, :] ** 2}
    lat = Lattice(['glc__D_e', 'lcts_e', 'MeAsp'], (NX, NX), (BOUND, BOUND), 10.0, 5.0, device=dev, initial=start)
    col = Colony(cfg, n, capacity=N + 36, device=dev, integrator='dopri5', environment=lat, table=t,
                 motility=MotilityModel(initial_ligand=0.1, substeps=10, seed=11) if motile else None)
    if n:
        params, conc = configs.heterogeneous_colony(t, cfg, n)
        loc = np.random.default_rng(17).uniform(0.0, BOUND, (2, n))
        loc[:, :n // 5] = 61.0 + np.random.default_rng(18).uniform(0.0, 4.0, (2, n // 5))    # crowded bins
        col.set_agents(params=params, conc=conc, location=loc)
        col.gather_external()
    return col


def _response_colony(dev, n=None):
    """tests/test_response_colony_gpu.py's death batch: agents that die at known steps."""
    from lens_amd.colony import Colony
    from lens_amd.response import from_antibiotics
    kin, resp = from_antibiotics({'diffusion': {'permeabilities': {'porin': 0.1}}})
    t = compile_rate_laws(kin['reactions'], kin['kinetic_parameters'])
    L = resp.bind(t)
    cases = response_ref.DEATH_CASES
    n_all = len(cases)
    col = Colony(kin, n_all if n is None else n, capacity=n_all + 3, device=dev, integrator='euler',
                 environment='nonspatial', env_volume_L=1e-12, avogadro=N_A, table=t, response=resp)
    if n is None:
        conc = response_ref.initial_state(t, L, kin, n_all)
        conc[L.row(('membrane', 'porin'))] = [c[0] for c in cases]
        col.set_agents(conc=conc, environment=np.array([[c[1] for c in cases]]))
    return col


def _host(col):
    return {name: getattr(col, name)[..., :col.n].cpu().numpy().copy() for name in col.agent_array_names()}


def _fill(fresh, col):
    """Set a fresh colony of col.n agents to col's state."""
    n = col.n
    assert fresh.n == n and fresh.agent_array_names() == col.agent_array_names()
    for name in col.agent_array_names():
        getattr(fresh, name)[..., :n].copy_(getattr(col, name)[..., :n])
    fresh.time, fresh.step_index = col.time, col.step_index
    if getattr(col, 'agent_order', None) is not None:
        fresh.agent_order = col.agent_order.clone()
    if col.lattice is not None:
        fresh.lattice.fields.copy_(col.lattice.fields)
        fresh.refresh_bins()
    if col.motility is not None:
        fresh._motil_counter.copy_(col._motil_counter)


def _same(a, b, where):
    assert a.n == b.n
    n = a.n
    if a.lattice is not None:
        assert torch.equal(a.lattice.fields, b.lattice.fields), where
    names = a.agent_array_names() + (['bin_lin', 'bin_ix'] if a.lattice is not None else [])
    for name in names:
        assert torch.equal(getattr(a, name)[..., :n], getattr(b, name)[..., :n]), (where, name)


def _remove_and_compare(col, mask, fresh_of, steps_after=2):
    before = _host(col)
    n, ld, layout = col.n, col.ld, col._layout
    keep = ~mask.cpu().numpy().astype(bool)[:n]
    removed = col.remove(mask)
    assert removed == n - int(keep.sum()) and col.n == int(keep.sum()) and col.ld == ld and col._layout > layout
    after = _host(col)
    assert list(after) == list(before)
    for name in before:
        assert after[name].dtype == before[name].dtype and getattr(col, name).shape[-1] == ld, name
        assert np.array_equal(after[name], before[name][..., keep]), name
    if col.lattice is not None:
        lin, ix = col.lattice.bin_sites(col.location, col.n)
        assert torch.equal(lin[:col.n], col.bin_lin[:col.n]) and torch.equal(ix[:col.n], col.bin_ix[:col.n])
    fresh = fresh_of(col.n)
    _fill(fresh, col)
    for s in range(steps_after):
        col.step(1.0)
        fresh.step(1.0)
        torch.cuda.synchronize()
        _same(col, fresh, s)
    col.check_status()
    return before, keep


def test_lattice_colony_random_mask(dev):
    col = _lattice_colony(dev)
    col.step(1.0)                                            # fluxes, counts, attempts, step sizes: all set
    mask = torch.from_numpy(np.random.default_rng(5).random(col.ld) < 0.3).to(dev)          # bool, over ld >= n
    before, keep = _remove_and_compare(col, mask, lambda n: _lattice_colony(dev, n))
    assert 900 < keep.sum() < 1200 and before['counts'].any() and before['flux'].any() and before['nsteps'].any()


def test_lattice_colony_stored_in_bin_order(dev):
    """After sort_by_bin the colony carries ``agent_order`` (n keys): it is compacted too, and
    the exchange keeps ordering each bin by it."""
    col = _lattice_colony(dev)
    col.sort_by_bin()
    col.step(1.0)
    order = col.agent_order.cpu().numpy().copy()
    mask = torch.from_numpy(np.random.default_rng(7).random(col.n) < 0.3).to(dev)
    before, keep = _remove_and_compare(col, mask, lambda n: _lattice_colony(dev, n))
    assert np.array_equal(col.agent_order.cpu().numpy(), order[keep]) and col.agent_order.shape[0] == col.n


def test_response_colony_drops_its_dead(dev):
    col = _response_colony(dev)
    for _ in range(64):
        col.step(1.0)
    n_dead = int(col.dead[:col.n].sum())
    assert 0 < n_dead < col.n
    before, keep = _remove_and_compare(col, col.dead[:col.n] != 0, lambda n: _response_colony(dev, n))
    assert int(col.dead[:col.n].sum()) == 0 and col.n == len(keep) - n_dead
    assert 'env_fields' in before and 'frozen' in before and before['frozen'].sum() == n_dead


def test_motile_colony(dev):
    col = _lattice_colony(dev, motile=True)
    col.step(1.0)
    mask = torch.from_numpy((np.random.default_rng(6).random(col.n) < 0.4).astype(np.int32)).to(dev)      # int32
    before, keep = _remove_and_compare(col, mask, lambda n: _lattice_colony(dev, n, motile=True))
    assert 'motil' in before and 800 < keep.sum() < 1000
    assert col._occ_dev.order[:col.n].sort().values.tolist() == list(range(col.n))           # this step's occupancy


def test_all_zero_mask_changes_nothing(dev):
    a, b = _lattice_colony(dev, 300), _lattice_colony(dev, 300)
    a.step(1.0)
    b.step(1.0)
    layout = a._layout
    assert a.remove(torch.zeros(300, dtype=torch.int32, device=dev)) == 0
    assert a.n == 300 and a._layout == layout
    a.step(1.0)
    b.step(1.0)
    torch.cuda.synchronize()
    _same(a, b, 'all-zero mask')


def test_all_one_mask_leaves_an_empty_colony_that_steps(dev):
    for col in (_lattice_colony(dev, 300), _lattice_colony(dev, 300, motile=True), _response_colony(dev)):
        col.step(1.0)
        n = col.n
        fields = col.lattice.fields.clone() if col.lattice is not None else None
        assert col.remove(torch.ones(n, dtype=torch.bool, device=dev)) == n and col.n == 0
        col.step(1.0)
        col.check_status()
        torch.cuda.synchronize()
        assert col.n == 0 and col.step_index == 2
        assert col.remove(torch.ones(0, dtype=torch.bool, device=dev)) == 0
        if fields is not None:
            # nobody exchanges: the planes only diffuse
            ref = _lattice_colony(dev, 0)
            ref.refresh_bins()
            ref.lattice.fields.copy_(fields)
            ref.step(1.0)
            assert torch.equal(ref.lattice.fields, col.lattice.fields)


def test_bad_masks_and_a_routed_colony_raise(dev):
    col = _lattice_colony(dev, 100)
    for bad in (np.zeros(100, dtype=bool), torch.zeros(100, dtype=torch.bool),                # not on the device
                torch.zeros(100, dtype=torch.int64, device=dev), torch.zeros(99, dtype=torch.bool, device=dev),
                torch.zeros((1, 100), dtype=torch.bool, device=dev)):
        with pytest.raises(ValueError, match='mask'):
            col.remove(bad)
    col.router = object()              # what distributed.AgentRouter sets: the order lives on other ranks
    with pytest.raises(ValueError, match='router'):
        col.remove(torch.zeros(100, dtype=torch.bool, device=dev))
    assert col.n == 100
