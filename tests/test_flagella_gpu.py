"""vk_flagella_step against its NumPy restatement (tests/flagella_ref.py, draws from
oracle.colony.philox_uniform), at the ABI level.

The bound, 1e-12.  The receptor rows are the coarse launch's: n_methyl bitwise after
one update, P_on to 1e-12 relative (tests/test_motility_gpu.py).  The rest is + - x /
in the reference's order under -ffp-contract=off, identical on both sides, around five
library functions.  The device library's FP64 functions are held to the OpenCL
accuracy limits: sqrt correctly rounded, exp and log <= 3 ulp, sin and cos <= 4 ulp,
pow <= 16 ulp; NumPy's are within 1 ulp (ulp = 2.2e-16 relative).
  z = sqrt(-2 log(1 - u1)) cos(2 pi u2): |log| <= 36.8 (1 - u1 >= 2^-53), so the root is
  <= 8.6 with (3 + 1) / 2 ulp relative error, the cosine has (4 + 1) ulp absolute error:
  |dz| <= 8.6 * (2 + 5) * 1.1e-16 < 7e-15.
  CheY_P, CheY (<= 10 uM): amp * dz with amp = sqrt(2 h / tau) <= 1 for h <= 0.1: < 7e-15,
  plus the roundings both sides share.  Absolute.
  cw_bias = y^H / (K^H + y^H): its slope in y is at most H / (4 K_d) = 0.83, so 6e-15 from
  CheY_P, and b (1 - b) * 2 * 17 ulp < 2e-15 from the two powers.  Absolute.
  angle += tumble_sigma h z (2.09 rad/s): < 2e-15 for h <= 0.1; torque = tumble_sigma z:
  < 1.5e-14.  Absolute.
  location += speed h cos(angle), speed <= 14 * 942 / 250 = 53 um/s: < 1e-14 um, compared
  relative to the bound as in the coarse test.
The largest term is the torque's 1.5e-14: 1e-12 leaves a 60-fold margin, the same
bound the coarse launch's test uses.  Over k updates the bound is k * 1e-12 (CheY_P's
own error contracts by 1 - h / tau per update; locations and angles accumulate).

The discrete results (flagella masks and counts, motile state, thrust, wall hits, bins)
can only be required to agree where the restatement's own decisions are not ties
within rounding: no switch draw within 1e-9 of its probability, no structural draw
within 1e-9 of its threshold, no moved coordinate within 1e-9 bin widths of a bin edge
or wall.  All three are asserted on the restatement alone.  The largest case here
makes ~60k draws: the chance of a violation is ~2e-4 per seed; SEED is the recorded one.
"""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import flagella_ref as ref

pytestmark = pytest.mark.gpu

SEED = 20261019
NX, NY = 17, 23
BOUNDS = (34.0, 57.5)          # bins of 2.0 x 2.5 um
H = 0.01                       # the reference's time_step
HS = 2.0 ** -7                 # for split launches: k * HS / k is HS exactly
BOUND = 1e-12
SPECIAL = (0, 1, 31, 32)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _model(**flagella):
    from lens_amd.motility import FlagellaModel, MotilityModel
    return MotilityModel(seed=SEED, initial_ligand=1e-2, flagella=FlagellaModel(5, **flagella))


def _field(rng):
    f = 10.0 * rng.random((NX, NY))
    f[0, 0], f[-1, -1] = 0.0, 10.0
    return f


def _states(rng, n):
    """Random states: have and target each over 0..32 with every pair of the special
    counts 0, 1, 31, 32 (growth, shrinkage, no change), random masks, CheY_P in [0, 6]
    with exact zeros, PMF in [50, 200], n_methyl over both clamp branches, and the
    first n // 4 agents within a fast run's reach of a wall."""
    motil = rng.random((9, n))
    motil[ref.R['n_methyl']] = rng.uniform(-0.5, 8.5, n)
    motil[ref.R['angle']] = rng.uniform(-np.pi, 3 * np.pi, n)
    motil[ref.R['CheY_P']], motil[ref.R['ccw_motor_bias']], motil[ref.R['ccw_to_cw']] = 0.25, 0.375, 0.625
    flag = rng.random((5, n))
    flag[ref.F['CheY']] = rng.uniform(0.0, 6.0, n)
    flag[ref.F['CheY_P']] = rng.uniform(0.0, 6.0, n)
    flag[ref.F['PMF']] = rng.uniform(50.0, 200.0, n)
    flag_int = np.zeros((3, n), dtype=np.int32)
    have, target = rng.integers(0, 33, n), rng.integers(0, 33, n)
    pairs = [(a, b) for a in SPECIAL for b in SPECIAL]
    for k, (a, b) in enumerate(pairs[:n]):
        have[k], target[k] = a, b
    mask = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    mask &= (np.uint64(1) << have.astype(np.uint64)) - np.uint64(1)
    if n > 40:
        flag[ref.F['CheY_P'], 16:24] = 0.0
        mask[24:32], have[24:32] = 0, np.maximum(have[24:32], 1)     # flagella, none of them CW: runs
        flag[ref.F['CheY_P'], 24:32] = 0.5                            # and a switch to CW is unlikely
    flag_int[0], flag_int[1], flag_int[2] = target, have, mask.astype(np.uint32).view(np.int32)
    loc = np.stack([rng.uniform(0, BOUNDS[0], n), rng.uniform(0, BOUNDS[1], n)])
    reach = 0.5
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
    return motil, flag, flag_int, loc


class _Device:
    """The arrays of one colony's worth of agents on the device, ld >= n, padded with sentinels."""

    def __init__(self, dev, model, field, state, ld=None, counter=0):
        from lens_amd.lattice import Lattice
        motil, flag, flag_int, loc = state
        n = motil.shape[1]
        self.n, self.ld = n, ld or n
        self.model = model
        self.lat = Lattice(['MeAsp'], (NX, NY), BOUNDS, 10.0, 5.0, device=dev, initial={'MeAsp': field})
        pad = lambda a, fill: np.concatenate([a, np.full((a.shape[0], self.ld - n), fill, dtype=a.dtype)], axis=1)
        self.motil = torch.from_numpy(pad(motil, -7.0)).to(dev).contiguous()
        self.flag = torch.from_numpy(pad(flag, -7.0)).to(dev).contiguous()
        self.flag_int = torch.from_numpy(pad(flag_int, -7)).to(dev).contiguous()
        self.loc = torch.from_numpy(pad(loc, -7.0)).to(dev).contiguous()
        self.bins = torch.full((self.ld,), -7, dtype=torch.int32, device=dev)
        self.ix = torch.full((self.ld,), -7, dtype=torch.int32, device=dev)
        self.counter = torch.tensor([counter], dtype=torch.int64, device=dev)

    def step(self, dt, substeps, key=None):
        from lens_amd.motility import flagella_step
        flagella_step(self.model, self.lat, self.loc, self.motil, self.flag, self.flag_int, self.n, dt, self.counter,
                      key=key, bin_lin=self.bins, bin_ix=self.ix, substeps=substeps)
        torch.cuda.synchronize()

    def tensors(self):
        return self.motil, self.flag, self.flag_int, self.loc, self.bins, self.ix

    def host(self):
        n = self.n
        return [t[..., :n].cpu().numpy() for t in (self.motil, self.flag, self.flag_int, self.loc, self.bins)]

    def padding_untouched(self):
        n = self.n
        return all(bool((t[..., n:] == -7).all()) for t in self.tensors())


def _copy(state):
    return tuple(a.copy() for a in state)


def _margins_ok(margins):
    return all(v >= 1e-9 for v in margins.values())


def _compare(got, want, scale, where):
    """scale 1: the single-update bound of the module docstring."""
    (gm, gf, gi, gl, gb), (wm, wf, wi, wl, wb) = got, want
    worst = {}
    r = ref.R['chemoreceptor_activity']
    worst['chemoreceptor_activity'] = float(np.max(np.abs(gm[r] - wm[r]) / np.maximum(np.abs(wm[r]), 1e-300)))
    r = ref.R['n_methyl']
    worst['n_methyl'] = float(np.max(np.abs(gm[r] - wm[r]) / np.maximum(np.abs(wm[r]), 1e-300)))
    for name in ('CheY', 'CheY_P', 'cw_bias'):
        worst[name] = float(np.max(np.abs(gf[ref.F[name]] - wf[ref.F[name]])))
    for name in ('angle', 'torque'):
        worst[name] = float(np.max(np.abs(gm[ref.R[name]] - wm[ref.R[name]])))
    worst['location'] = float(max(np.max(np.abs(gl[0] - wl[0])) / BOUNDS[0], np.max(np.abs(gl[1] - wl[1])) / BOUNDS[1]))
    print(where, worst)
    assert np.array_equal(gi, wi), where                                               # target, have, mask
    assert np.array_equal(gf[ref.F['motile_state']], wf[ref.F['motile_state']]), where
    assert np.array_equal(gf[ref.F['PMF']], wf[ref.F['PMF']]), where
    for name in ('motor_state', 'thrust', 'CheY_P', 'ccw_motor_bias', 'ccw_to_cw'):   # the last three: untouched
        assert np.array_equal(gm[ref.R[name]], wm[ref.R[name]]), (where, name)
    assert np.array_equal(gb, wb), where
    for name, w in worst.items():
        if name != 'n_methyl':
            assert w <= scale * BOUND, (where, name, w)
    return worst


def test_one_update_from_random_states(dev):
    n = 1000
    rng = np.random.default_rng(SEED)
    model = _model()
    field = _field(rng)
    state = _states(rng, n)
    d = _Device(dev, model, field, state, counter=7)
    motil, flag, flag_int, loc = want = _copy(state)
    margins = {}
    bins = ref.step(model, motil, flag, flag_int, loc, field, BOUNDS, H, 1, 7, margins=margins)
    # the conditions, on the restatement alone
    assert set(margins) == {'switch', 'structural', 'edge'} and _margins_ok(margins), margins
    # the cases the states were drawn for did occur
    have0, target0 = state[2][1], state[2][0]
    for c in SPECIAL:
        assert (have0 == c).any() and (target0 == c).any()
    assert (target0 > have0).any() and (target0 < have0).any() and (target0 == have0).any()
    assert set(np.unique(flag[ref.F['motile_state']])) == {-1.0, 0.0, 1.0}
    assert (state[1][ref.F['CheY_P']] == 0.0).any() and (flag[ref.F['CheY_P']] == 0.0).any()
    assert np.array_equal(flag_int[1], np.clip(target0, 0, 32))
    assert ((flag_int[2].view(np.uint32).astype(np.uint64) >> flag_int[1].astype(np.uint64)) == 0).all()
    d.step(H, 1)
    got = d.host()
    _compare(got, (motil, flag, flag_int, loc, bins), 1, 'one update')
    assert np.array_equal(got[0][ref.R['n_methyl']], motil[ref.R['n_methyl']])          # bitwise
    assert int(d.counter[0]) == 8
    assert np.array_equal(d.ix[:n].cpu().numpy(), bins // NY)
    assert (got[3] >= 0).all() and (got[3][0] < BOUNDS[0]).all() and (got[3][1] < BOUNDS[1]).all()


def test_counts_outside_the_range_are_clamped(dev):
    """target and have beyond 0..32 (a device tensor handed to set_flagella is not read
    back) are used clamped; mask bits at and above have are ignored."""
    rng = np.random.default_rng(SEED + 5)
    model = _model(omega=0.0)                # frozen switches: the masks show the structure alone
    field = _field(rng)
    state = _states(rng, 8)
    state[2][0] = [40, -3, 32, 5, 40, 0, 33, 2 ** 31 - 1]
    state[2][1] = [32, 2, 40, -1, 0, 32, 32, 32]
    state[2][2] = -1                         # every bit set
    d = _Device(dev, model, field, state, counter=1)
    d.step(H, 1)
    got = d.host()[2]
    assert got[0].tolist() == state[2][0].tolist()                                      # target is only read
    assert got[1].tolist() == [32, 0, 32, 5, 32, 0, 32, 32]
    masks = got[2].view(np.uint32)
    assert masks[0] == masks[2] == masks[6] == masks[7] == 2 ** 32 - 1 and masks[1] == masks[5] == 0
    assert masks[3] < 32 and d.padding_untouched()


def test_launch_splitting(dev):
    """One launch of 30 updates, 30 launches of 1 and 3 launches of 10 agree on the
    device bit for bit (the device counter carries the inner-update index), and with
    the restatement within 30 x the bound.  n_methyl integrates P_on, so over a
    trajectory it gets the relative bound of P_on."""
    n = 192
    rng = np.random.default_rng(SEED + 1)
    model = _model()
    field = _field(rng)
    state = _states(rng, n)
    state[0][ref.R['n_methyl']] = rng.uniform(0.5, 7.5, n)
    a, b, c = (_Device(dev, model, field, state, counter=100) for _ in range(3))
    a.step(30 * HS, 30)
    for _ in range(30):
        b.step(HS, 1)
    for _ in range(3):
        c.step(10 * HS, 10)
    for x, y, z in zip(a.tensors(), b.tensors(), c.tensors()):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert int(a.counter[0]) == int(b.counter[0]) == int(c.counter[0]) == 130
    motil, flag, flag_int, loc = _copy(state)
    margins = {}
    for s in range(30):
        bins = ref.step(model, motil, flag, flag_int, loc, field, BOUNDS, HS, 1, 100 + s, margins=margins)
    assert _margins_ok(margins), margins
    worst = _compare(a.host(), (motil, flag, flag_int, loc, bins), 30, 'trajectory')
    assert worst['n_methyl'] <= 30 * BOUND


def test_keys_not_columns_pick_the_draws(dev):
    """Agents stored in another column order, with their keys, take the same walk."""
    n = 300
    rng = np.random.default_rng(SEED + 2)
    model = _model()
    field = _field(rng)
    state = _states(rng, n)
    perm = rng.permutation(n)
    a = _Device(dev, model, field, state, counter=5)
    b = _Device(dev, model, field, tuple(x[:, perm] for x in state), counter=5)
    key = torch.from_numpy(perm.astype(np.int64)).to(dev)
    for _ in range(3):
        a.step(3 * H, 3)
        b.step(3 * H, 3, key=key)
    p = torch.from_numpy(perm).to(dev)
    for x, y in zip(a.tensors(), b.tensors()):
        assert torch.equal(x[..., p], y)


@pytest.mark.parametrize('n,ld', [(0, 4), (1, 1), (63, 64), (64, 64), (65, 128), (257, 300)])
def test_edge_sizes_leave_the_padding_untouched(dev, n, ld):
    rng = np.random.default_rng(SEED + 3)
    model = _model()
    field = _field(rng)
    state = tuple(x[:, :n] for x in _states(rng, max(n, 1)))
    d = _Device(dev, model, field, state, ld=ld, counter=3)
    d.step(2 * H, 2)
    assert int(d.counter[0]) == 5                      # inner updates, counted for an empty colony too
    assert d.padding_untouched()
    if n:
        motil, flag, flag_int, loc = _copy(state)
        margins = {}
        bins = ref.step(model, motil, flag, flag_int, loc, field, BOUNDS, 2 * H, 2, 3, margins=margins)
        assert _margins_ok(margins), margins
        _compare(d.host(), (motil, flag, flag_int, loc, bins), 2, 'edge size')


@pytest.mark.parametrize('count,want', [(1, 0.15926368960196843), (5, 0.5800), (32, 0.9961)])
def test_stationary_tumble_fraction(dev, count, want):
    """Without CheY-P noise each flagellum is a two-state chain with p01 = CCW_to_CW h and
    p10 = CW_to_CCW h at CheY_P = YP_ss: CW with probability pi = p01 / (p01 + p10) once
    stationary, so a cell with n flagella tumbles with probability 1 - (1 - pi)^n.  1000
    updates are 35 relaxation times (1 / (p01 + p10) = 28 updates); agents are independent."""
    n = 65536
    pi = 0.15926368960196843
    q = 1.0 - (1.0 - pi) ** count
    assert abs(q - want) < 5e-5
    model = _model(sigma2_Y=0.0)
    rng = np.random.default_rng(SEED + 4)
    field = _field(rng)
    motil = np.zeros((9, n))
    motil[ref.R['n_methyl']], motil[ref.R['chemoreceptor_activity']] = model.n_methyl, model.chemoreceptor_activity
    motil[ref.R['angle']] = rng.uniform(0, 2 * np.pi, n)
    flag = np.zeros((5, n))
    flag[ref.F['CheY']], flag[ref.F['CheY_P']], flag[ref.F['PMF']] = 2.59, 2.59, 170.0
    flag_int = np.zeros((3, n), dtype=np.int32)
    flag_int[0], flag_int[1] = count, count
    loc = np.stack([rng.uniform(0, BOUNDS[0], n), rng.uniform(0, BOUNDS[1], n)])
    d = _Device(dev, model, field, (motil, flag, flag_int, loc), counter=0)
    d.step(1000 * H, 1000)
    assert bool((d.flag[ref.F['CheY_P']] == 2.59).all())
    tumbling = d.motil[ref.R['motor_state']]
    assert torch.equal(tumbling != 0, d.flag_int[2] != 0) and bool((d.flag_int[1] == count).all())
    fraction = float(tumbling.mean())
    sd = (q * (1.0 - q) / n) ** 0.5
    print('n_flagella', count, 'tumbling', fraction, 'expected', q, 'sd', (fraction - q) / sd)
    assert abs(fraction - q) <= 5.0 * sd


def test_bad_arguments_return_err_arg(dev):
    from lens_amd import native
    model = _model()
    rng = np.random.default_rng(SEED + 6)
    d = _Device(dev, model, _field(rng), _states(rng, 4), counter=9)
    before = [t.clone() for t in d.tensors()]
    p, f = model.vk_params(), model.flagella.vk_params()
    bad_tau = model.flagella.vk_params()
    bad_tau.tau = 0.0
    plane = d.lat.fields[0]

    def call(p=ctypes.byref(p), f=ctypes.byref(f), n=4, ld=4, dt=H, substeps=1, motil=d.motil, flag=d.flag,
             flag_int=d.flag_int, loc=d.loc, ligand=plane, nx=NX, ny=NY, bx=BOUNDS[0], by=BOUNDS[1],
             counter=d.counter, bins=d.bins):
        return native._lib.vk_flagella_step(
            p, f, n, ld, dt, substeps, native.ptr(motil), native.ptr(flag), native.ptr(flag_int), native.ptr(loc),
            None, native.ptr(ligand), nx, ny, bx, by, native.ptr(counter), native.ptr(bins), None,
            native.stream_handle())

    for kw in (dict(p=None), dict(f=None), dict(n=-1), dict(n=5), dict(dt=0.0), dict(dt=float('nan')),
               dict(substeps=0), dict(motil=None), dict(flag=None), dict(flag_int=None), dict(loc=None),
               dict(ligand=None), dict(nx=0), dict(ny=-1), dict(bx=0.0), dict(by=-1.0), dict(counter=None),
               dict(bins=None), dict(f=ctypes.byref(bad_tau)), dict(nx=65536, ny=65536)):
        assert call(**kw) == native.VK_ERR_ARG, kw
    torch.cuda.synchronize()
    assert int(d.counter[0]) == 9                      # nothing was launched
    for t, t0 in zip(d.tensors(), before):
        assert torch.equal(t, t0)
    assert call() == 0 and int(d.counter[0]) == 10
