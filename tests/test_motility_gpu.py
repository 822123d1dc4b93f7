"""vk_motility_step against its NumPy restatement (tests/motility_ref.py, draws
from oracle.colony.philox_uniform), at the ABI level.

Tolerances.  n_methyl is pure + - x in the same order under -ffp-contract=off:
bitwise after one update.  P_on = 1 / (1 + exp(F)) with |F| <= 18 (3 + ln 501)
~ 170: two <= 1-ulp logs on each side, multiplied by at most 12, give |dF| <~
5e-14, one <= 1-ulp exp follows, so P_on is good to ~1e-13 relative; CheY_P, the
bias and ccw_to_cw are a few more correctly rounded operations on it.  1e-12
leaves a 10x margin.  Angle and location add one sin / cos / log / sqrt each, of
magnitude <= a few, to values of magnitude <= the bound: 1e-12 absolute (times
the bound for locations).  Torque is tumble_sigma * z with z's absolute error a
few 1e-16: 1e-12 absolute.

The discrete results (motor state, wall hits, bins) can only be required to
agree when the restatement's own decision is not a tie within rounding: no
|u0 - p| < 1e-9 and no moved coordinate within 1e-9 bin widths of a bin edge or
wall.  Both are asserted on the restatement alone.  With ~4k draws the chance
of a violation is ~1e-5, so any seed does; SEED is the one recorded here.
"""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import motility_ref as ref

pytestmark = pytest.mark.gpu

SEED = 20261019
NX, NY = 17, 23
BOUNDS = (34.0, 57.5)          # bins of 2.0 x 2.5 um
DT = 0.1                       # one run step: 1.4 um
REL = ('chemoreceptor_activity', 'CheY_P', 'ccw_motor_bias', 'ccw_to_cw')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _model(**kw):
    from lens_amd.motility import MotilityModel
    return MotilityModel(seed=SEED, **kw)


def _field(rng):
    f = 10.0 * rng.random((NX, NY))
    f[0, 0], f[-1, -1] = 0.0, 10.0          # 0 to 10 mM
    return f


def _states(rng, n, model):
    """Random states: n_methyl over [-0.5, 8.5] (both clamp branches, every
    offset-energy segment), both motor states, and the first n // 4 agents within
    one run step of a wall -- every wall and every corner."""
    motil = rng.random((9, n))
    motil[ref.R['n_methyl']] = rng.uniform(-0.5, 8.5, n)
    motil[ref.R['motor_state']] = rng.integers(0, 2, n)
    motil[ref.R['angle']] = rng.uniform(-np.pi, 3 * np.pi, n)
    loc = np.stack([rng.uniform(0, BOUNDS[0], n), rng.uniform(0, BOUNDS[1], n)])
    reach = model.run_speed * DT
    for a in range(n // 4):
        side = a % 8                         # 4 walls, 4 corners
        near = lambda b, hi: (b - rng.uniform(0, reach)) if hi else rng.uniform(0, reach)
        if side in (0, 4, 5):
            loc[0, a] = near(BOUNDS[0], False)
        if side in (1, 6, 7):
            loc[0, a] = near(BOUNDS[0], True)
        if side in (2, 4, 6):
            loc[1, a] = near(BOUNDS[1], False)
        if side in (3, 5, 7):
            loc[1, a] = near(BOUNDS[1], True)
    return motil, loc


class _Device:
    """The arrays of one colony's worth of agents on the device, ld >= n."""

    def __init__(self, dev, model, field, motil, loc, ld=None, counter=0):
        from lens_amd.lattice import Lattice
        n = motil.shape[1]
        self.n, self.ld = n, ld or n
        self.model = model
        self.lat = Lattice(['MeAsp'], (NX, NY), BOUNDS, 10.0, 5.0, device=dev, initial={'MeAsp': field})
        pad = lambda a, fill: np.concatenate([a, np.full((a.shape[0], self.ld - n), fill)], axis=1)
        self.motil = torch.from_numpy(pad(motil, -7.0)).to(dev).contiguous()
        self.loc = torch.from_numpy(pad(loc, -7.0)).to(dev).contiguous()
        self.bins = torch.full((self.ld,), -7, dtype=torch.int32, device=dev)
        self.ix = torch.full((self.ld,), -7, dtype=torch.int32, device=dev)
        self.counter = torch.tensor([counter], dtype=torch.int64, device=dev)

    def step(self, dt, substeps, key=None):
        from lens_amd.motility import motility_step
        motility_step(self.model, self.lat, self.loc, self.motil, self.n, dt, self.counter, key=key,
                      bin_lin=self.bins, bin_ix=self.ix, substeps=substeps)
        torch.cuda.synchronize()

    def host(self):
        n = self.n
        return self.motil[:, :n].cpu().numpy(), self.loc[:, :n].cpu().numpy(), self.bins[:n].cpu().numpy()


def _compare(got, want, scale, where):
    """scale 1: the single-update tolerances of the module docstring."""
    (gm, gl, gb), (wm, wl, wb) = got, want
    worst = {}
    for name in REL + ('n_methyl',):
        r = ref.R[name]
        worst[name] = float(np.max(np.abs(gm[r] - wm[r]) / np.maximum(np.abs(wm[r]), 1e-300)))
    worst['angle'] = float(np.max(np.abs(gm[ref.R['angle']] - wm[ref.R['angle']])))
    worst['torque'] = float(np.max(np.abs(gm[ref.R['torque']] - wm[ref.R['torque']])))
    worst['location'] = float(max(np.max(np.abs(gl[0] - wl[0])) / BOUNDS[0], np.max(np.abs(gl[1] - wl[1])) / BOUNDS[1]))
    print(where, worst)
    assert np.array_equal(gm[ref.R['motor_state']], wm[ref.R['motor_state']]), where
    assert np.array_equal(gm[ref.R['thrust']], wm[ref.R['thrust']]), where
    assert np.array_equal(gb, wb), where
    for name in REL:
        assert worst[name] <= scale * 1e-12, (where, name, worst[name])
    for name in ('angle', 'torque', 'location'):
        assert worst[name] <= scale * 1e-12, (where, name, worst[name])
    return worst


def test_one_update_from_random_states(dev):
    n = 4096
    rng = np.random.default_rng(SEED)
    model = _model()
    field = _field(rng)
    motil, loc = _states(rng, n, model)
    d = _Device(dev, model, field, motil, loc, counter=7)
    margins = {}
    bins = ref.step(model, motil, loc, field, BOUNDS, DT, 1, 7, margins=margins)
    # the conditions, on the restatement alone
    assert margins['switch'] >= 1e-9 and margins['edge'] >= 1e-9, margins
    # the cases the states were drawn for did occur
    nm = motil[ref.R['n_methyl']]
    assert (nm == 0.0).any() and (nm == 8.0).any()
    assert all(((nm > lo) & (nm < hi)).any() for lo, hi in ((0, 2), (2, 4), (4, 6), (6, 7), (7, 8)))
    assert set(np.unique(motil[ref.R['motor_state']])) == {0.0, 1.0}
    d.step(DT, 1)
    got = d.host()
    _compare(got, (motil, loc, bins), 1, 'one update')
    assert np.array_equal(got[0][ref.R['n_methyl']], nm)                 # bitwise
    assert int(d.counter[0]) == 8
    assert np.array_equal(d.ix[:n].cpu().numpy(), bins // NY)
    assert (got[1] >= 0).all() and (got[1][0] < BOUNDS[0]).all() and (got[1][1] < BOUNDS[1]).all()


def test_trajectory_and_substeps(dev):
    """20 calls of dt = 0.1 equal 2 calls of dt = 1 with 10 substeps bit for bit
    (the device counter carries the inner-update index), and stay within 20x the
    single-update tolerances of the restatement.  n_methyl is bitwise only for one
    update (it integrates P_on, which is not): over the trajectory it gets the
    relative tolerance of the other rows."""
    n = 512
    rng = np.random.default_rng(SEED + 1)
    model = _model()
    field = _field(rng)
    motil, loc = _states(rng, n, model)
    motil[ref.R['n_methyl']] = rng.uniform(0.5, 7.5, n)
    a = _Device(dev, model, field, motil, loc, counter=100)
    b = _Device(dev, model, field, motil, loc, counter=100)
    for _ in range(20):
        a.step(DT, 1)
    for _ in range(2):
        b.step(1.0, 10)
    assert torch.equal(a.motil, b.motil) and torch.equal(a.loc, b.loc) and torch.equal(a.bins, b.bins)
    assert int(a.counter[0]) == int(b.counter[0]) == 120
    margins = {}
    for s in range(20):
        bins = ref.step(model, motil, loc, field, BOUNDS, DT, 1, 100 + s, margins=margins)
    assert margins['switch'] >= 1e-9 and margins['edge'] >= 1e-9, margins
    worst = _compare(a.host(), (motil, loc, bins), 20, 'trajectory')
    assert worst['n_methyl'] <= 20 * 1e-12


def test_keys_not_columns_pick_the_draws(dev):
    """Agents stored in another column order, with their keys, take the same walk."""
    n = 300
    rng = np.random.default_rng(SEED + 2)
    model = _model(substeps=3)
    field = _field(rng)
    motil, loc = _states(rng, n, model)
    perm = rng.permutation(n)
    a = _Device(dev, model, field, motil, loc, counter=5)
    b = _Device(dev, model, field, motil[:, perm], loc[:, perm], counter=5)
    key = torch.from_numpy(perm.astype(np.int64)).to(dev)
    for _ in range(3):
        a.step(0.3, None)
        b.step(0.3, None, key=key)
    p = torch.from_numpy(perm).to(dev)
    assert torch.equal(a.motil[:, p], b.motil) and torch.equal(a.loc[:, p], b.loc) and torch.equal(a.bins[p], b.bins)


@pytest.mark.parametrize('n,ld', [(0, 4), (1, 1), (1, 64), (257, 300)])
def test_edge_sizes_leave_the_padding_untouched(dev, n, ld):
    rng = np.random.default_rng(SEED + 3)
    model = _model()
    field = _field(rng)
    motil, loc = _states(rng, max(n, 1), model)
    motil, loc = motil[:, :n], loc[:, :n]
    d = _Device(dev, model, field, motil, loc, ld=ld, counter=3)
    d.step(DT, 2)
    assert int(d.counter[0]) == 5                      # inner updates, counted for an empty colony too
    assert bool((d.motil[:, n:] == -7.0).all()) and bool((d.loc[:, n:] == -7.0).all())
    assert bool((d.bins[n:] == -7).all()) and bool((d.ix[n:] == -7).all())
    if n:
        margins = {}
        bins = ref.step(model, motil, loc, field, BOUNDS, DT, 2, 3, margins=margins)
        assert margins['switch'] >= 1e-9 and margins['edge'] >= 1e-9, margins
        got = d.host()
        assert np.array_equal(got[2], bins)
        assert np.array_equal(got[0][ref.R['motor_state']], motil[ref.R['motor_state']])
        assert np.max(np.abs(got[1] - loc)) <= 2e-12 * max(BOUNDS)
