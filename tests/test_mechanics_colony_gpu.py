"""Colony(mechanics=...): growing, dividing capsules that push each other apart,
re-binned on the device.

The step must equal, bit for bit, the host route to the same state -- the
contact launch on a plain colony's arrays, ``refresh_bins()`` (host sorts, host
reads, a re-layout), then ``step()`` -- through divisions and through the
reallocation when the colony outgrows its capacity; without cells it must not
depend on the storage order and must replay from a captured graph; and a colony
without ``mechanics`` must step exactly as before.

Setup: glc_lct kinetics (DP45) on 64 x 64 bins of 2 um; 200 growing cells
(CellModel 'growth', 2 % per step) crowded into a 24 um patch, a quarter of them
within 5 steps of the division volume, capacity 220 so that ``ld`` grows once."""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import mechanics_ref as ref
from lens_amd import configs, native
from lens_amd.rate_law_compiler import compile_rate_laws

pytestmark = pytest.mark.gpu

NX, BOUND, STEPS = 64, 128.0, 5
N_CELLS, CAPACITY = 200, 220
N_PLAIN = 600


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _model(**kw):
    from lens_amd.mechanics import ContactModel
    kw.setdefault('jitter', 0.01)
    kw.setdefault('jitter_angle', 0.02)
    return ContactModel(seed=11, **kw)


def _cells(rate=0.02):
    from lens_amd.cells import CellModel
    return CellModel(model='growth', growth_rate=rate)


def _lattice(dev):
    from lens_amd.lattice import Lattice
    start = {'glc__D_e': configs.gaussian_bump_field((NX, NX)), 'lcts_e': np.full((NX, NX), 10.0)}
    return Lattice(['glc__D_e', 'lcts_e'], (NX, NX), (BOUND, BOUND), 10.0, 5.0, device=dev, initial=start)


def _colony(dev, n, *, mechanics=None, cells=None, capacity=None, patch=24.0, mass=None, angles=None, seed=17,
            exchange='sorted'):
    from lens_amd.colony import Colony
    cfg = configs.glc_lct_config()
    t = compile_rate_laws(cfg['reactions'], cfg['kinetic_parameters'])
    rng = np.random.default_rng(seed)
    params, conc = configs.heterogeneous_colony(t, cfg, n)
    loc = 64.0 - patch / 2 + rng.uniform(0.0, patch, (2, n))
    col = Colony(cfg, n, capacity=capacity, device=dev, integrator='dopri5', environment=_lattice(dev), table=t,
                 exchange=exchange, cells=cells, mechanics=mechanics)
    col.set_agents(params=params, conc=conc, location=loc)
    if cells is not None:
        if mass is None:
            # division at 2.4 fL = 2640 fg; 2 % a step is x 1.104 in 5 steps
            mass = rng.uniform(1400.0, 2300.0, n)
            mass[::4] = rng.uniform(2400.0, 2635.0, len(mass[::4]))
        col.set_cell_mass(mass)
        if angles is None:
            angles = rng.uniform(0.0, 2.0 * np.pi, n)
        col.cell[native.VK_CELL_ANGLE, :n] = torch.from_numpy(np.asarray(angles, dtype=np.float64)).to(dev)
    col.gather_external()
    return col


def _same(a, b, names, where, perm=None):
    assert a.n == b.n, where
    n = a.n
    for m in a.lattice.molecules:
        assert torch.equal(a.lattice.owned(m), b.lattice.owned(m)), (where, m)
    for name in names:
        x, y = getattr(a, name)[..., :n], getattr(b, name)[..., :n]
        if perm is not None:
            x = x[..., perm]
        assert torch.equal(x, y), (where, name)


def test_mechanics_step_equals_the_host_route_through_division(dev):
    from lens_amd.mechanics import ContactBuffers, contact_step
    model = _model()
    a = _colony(dev, N_CELLS, mechanics=model, cells=_cells(), capacity=CAPACITY)
    b = _colony(dev, N_CELLS, cells=_cells(), capacity=CAPACITY)
    grid = model.grid(b.lattice.bounds)
    buf = ContactBuffers(b.ld, grid[0] * grid[1], dev)
    layout_a, layout_b = a._layout, b._layout
    loc0 = a.location[:, :N_CELLS].clone()
    ns, lds = [a.n], [a.ld]
    for step in range(STEPS):
        a.step(1.0)
        if b.ld > buf.ld:                                        # the twin outgrew its buffers too
            buf = ContactBuffers(b.ld, grid[0] * grid[1], dev, counter=int(buf.counter[0]))
        contact_step(model, b.lattice, b.location, b.cell[native.VK_CELL_ANGLE], b.n, buf,
                     length=b.cell[native.VK_CELL_LENGTH])
        b.refresh_bins()
        b.step(1.0)
        torch.cuda.synchronize()
        _same(a, b, ('location', 'cell', 'counts', 'conc', 'bin_lin'), step)
        ns.append(a.n)
        lds.append(a.ld)
    a.check_status()
    print('n per step', ns, 'ld', lds)
    assert ns[-1] > ns[0] and all(x <= y for x, y in zip(ns, ns[1:]))
    assert N_CELLS // 5 <= ns[-1] - ns[0] <= N_CELLS // 3            # about a quarter divided
    assert lds[0] == CAPACITY and lds[-1] > CAPACITY and len(set(lds)) == 2        # ld grew once ...
    assert ns[lds.index(lds[-1])] < ns[-1]                                         # ... and n kept growing after
    assert a._mech.ld == a.ld and a._occ_dev.order.numel() == a.ld
    assert int(a._mech.counter[0]) == int(buf.counter[0]) == model.iterations * STEPS
    # the contact launch itself re-lays nothing out: the twin's extra bumps are its refresh_bins()
    assert (a._layout - layout_a) == (b._layout - layout_b) - STEPS
    moved = (a.location[:, :N_CELLS] - loc0).abs().max(0).values
    assert float(moved.max()) > 0.1
    snap = a.snapshot()
    assert np.array_equal(snap['mechanics']['angle'], snap['global']['angle'])
    assert 'mech_angle' not in a.agent_array_names()


def _plain(dev, **kw):
    """600 agents of constant length 2 um without cells, crowded into a 30 um patch."""
    return _colony(dev, N_PLAIN, mechanics=_model(), patch=30.0, **kw)


def test_without_cells_the_storage_order_does_not_matter(dev):
    a, b = _plain(dev), _plain(dev)
    assert 'mech_angle' in a.agent_array_names() and torch.equal(a.mech_angle, b.mech_angle)
    order = b.sort_by_bin()
    assert not torch.equal(order, torch.arange(N_PLAIN, device=dev))
    layout = b._layout
    for _ in range(STEPS):
        a.step(1.0)
        b.step(1.0)
    torch.cuda.synchronize()
    _same(a, b, ('conc', 'counts', 'flux', 'location', 'mech_angle', 'bin_lin'), 'sorted twin', perm=order)
    assert b._layout == layout                                   # no re-layout by the contact launch
    assert float((a.location[:, :N_PLAIN] - _plain(dev).location[:, :N_PLAIN]).abs().max()) > 0.1
    a.check_status()
    assert np.array_equal(a.snapshot()['mechanics']['angle'], a.mech_angle[:N_PLAIN].cpu().numpy())


def test_captured_steps_equal_eager_steps(dev):
    a, b = _plain(dev), _plain(dev)
    a.step(1.0)
    b.step(1.0)
    layout = b._layout
    replay = b.capture(1.0, 3)
    torch.cuda.synchronize()
    _same(a, b, ('conc', 'location', 'mech_angle'), 'capture ran nothing')
    for _ in range(6):
        a.step(1.0)
    replay()
    replay()
    torch.cuda.synchronize()
    _same(a, b, ('conc', 'counts', 'flux', 'location', 'mech_angle', 'bin_lin'), 'replayed')
    assert b._layout == layout and a._layout == layout
    assert int(b._mech.counter[0]) == 7 * b.mechanics.iterations and b.step_index == 7
    with pytest.raises(ValueError, match='overlap'):
        b.capture(1.0, 1, overlap=True)
    with pytest.raises(ValueError, match='step\\(\\)'):
        b.run(1.0)
    with pytest.raises(ValueError, match='division'):            # with cells capture stays refused
        _colony(dev, 8, mechanics=_model(), cells=_cells()).capture(1.0, 1)


def test_atomic_exchange_needs_only_the_bins(dev):
    """As for the motile colony: the fields agree with the ordered exchange to
    rounding, the agents exactly until the fields differ -- compared after one step."""
    a, b = _plain(dev), _plain(dev, exchange='atomic')
    a.step(1.0)
    b.step(1.0)
    torch.cuda.synchronize()
    for name in ('conc', 'counts', 'location', 'mech_angle', 'bin_lin'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.allclose(a.lattice.fields, b.lattice.fields, rtol=1e-12, atol=0.0)


def test_too_long_agents_are_reported_by_check_status(dev):
    a = _colony(dev, 16, mechanics=_model(length=4.5))          # cell edge 128 / 32 = 4 um
    a.step(1.0)
    with pytest.raises(ValueError, match='longer than max_length'):
        a.check_status()


def _overlap(col):
    n = col.n
    loc = col.location[:, :n].cpu().numpy()
    cell = col.cell[:, :n].cpu().numpy()
    return ref.overlap_sum(loc[0], loc[1], cell[native.VK_CELL_ANGLE], cell[native.VK_CELL_LENGTH], 1.0)


def test_a_growing_lineage_spreads_instead_of_piling_up(dev):
    """8 cells, 20 steps at 5 % growth a step (every lineage divides at least once):
    with mechanics the summed pair overlap stays below that of the same colony
    without, whose daughters sit at +-L/4 on their mother's axis for good."""
    kw = dict(cells=None, capacity=64, patch=12.0, mass=np.linspace(1500.0, 2500.0, 8),
              angles=np.linspace(0.0, 3.0, 8))
    a = _colony(dev, 8, mechanics=_model(), **dict(kw, cells=_cells(0.05)))
    b = _colony(dev, 8, **dict(kw, cells=_cells(0.05)))
    for _ in range(20):
        a.step(1.0)
        b.step(1.0)
    torch.cuda.synchronize()
    assert a.n == b.n and a.n >= 16
    oa, ob = _overlap(a), _overlap(b)
    print('cells', a.n, 'summed overlap with mechanics', oa, 'without', ob)
    assert ob > 1.0 and oa < ob
    a.check_status()


def test_colony_without_mechanics_takes_the_old_path(dev):
    """Kinetics, gather, diffusion, host occupancy + vk_exchange_sorted, launched
    by hand as step() launched them before mechanics existed, against step()."""
    from lens_amd.lattice import occupancy
    a, b = _colony(dev, N_PLAIN), _colony(dev, N_PLAIN)
    for step in range(3):
        a.step(1.0)
        b.kinetics(1.0)
        b.gather_external()
        b.lattice.diffuse(1.0)
        b.lattice.exchange_sorted(occupancy(b.bin_lin, N_PLAIN), b.counts, b.map_exch_count, b.map_exch_field)
        torch.cuda.synchronize()
        _same(a, b, ('conc', 'counts', 'flux', 'location', 'bin_lin'), step)
    assert a.mechanics is None and not hasattr(a, 'mech_angle') and not hasattr(a, '_mech')
    assert 'mech_angle' not in a.agent_array_names() and 'mechanics' not in a.snapshot()
