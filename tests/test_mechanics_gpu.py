"""vk_contact_step against its NumPy restatement (tests/mechanics_ref.py, jitter
draws from oracle.colony.philox_uniform), at the ABI level, one relaxation
iteration at a time: every iteration is compared from the device's own state
before it, so errors do not compound.

Tolerance: 1e-12 absolute on x, y and theta.  The library is compiled with
-ffp-contract=off and the restatement performs the same + - x / sqrt in the same
order, all correctly rounded on both sides -- so the two differ only through
cos / sin of the axis angle (device library against libm: each within an ulp,
so a spine direction differs by an angle eps <~ 3e-16) and, with jitter, one
log / sqrt / cos / sin each, of magnitude <= a few, times a jitter <= 0.05.
Centres are <= 128 um (an ulp <= 2.9e-14) and every intermediate is <= a few um,
so a contact adds a few 1e-16 to a push, and a few dozen contacts stay far inside
the bound -- except where the geometry itself amplifies eps:
  * the closest-point solve s = (b f - c) / den turns eps into ds <= 2 eps |rho| /
    den (|rho| <= 4).  Where a closest point is clamped to a spine end it is not
    solved for, so this bites only when both are interior: the spines cross.  s
    then enters the turn directly, d(theta) = ds |push| 12 / L^2 <= (2 * 3e-16 * 4
    / den) * 0.25 * 12 = 7.5e-15 / den;
  * the normal v / d turns the difference of v -- eps times the lever arms, c and f
    of up to |rho| + h ~ 5 um on both spines, ~3e-15 in all -- into 3e-15 / d,
    times a push <= 0.25: 7.5e-16 / d.
With DEN_CROSS_MIN = 1e-2 and D_SMALL_MIN = 1e-3 both stay at or below 7.5e-13
in the worst case.  Measured on an MI355X: 5.5e-13 on y at n = 257 (a touching
pair 1.2e-3 apart, the second mechanism), <= 1.1e-14 in every other iteration
compared -- inside the bound, though the worst case not by 10x.  Both are
asserted on the restatement's values before every compared iteration: the drawn
states are conditioned for them (axis angles are swapped between agents until
they hold), and the seeds recorded here are ones for which the restatement's own
trajectory keeps them for the iterations compared.

Branch decisions can only be required to agree when the restatement's own are
not ties within rounding: no pair with |delta| < 1e-9, |den - 1e-12| < 1e-9 or
|d - 1e-9| < 1e-10 (the deliberate degenerate pairs excepted: they sit exactly
on their branch).  Asserted on the restatement's values before every compared
iteration; nothing is skipped.  The drawn states meet this for every pair (axis
angles are stratified modulo pi).  After an iteration the turned angles are the
device's, and among 500,000 pairs a few land within 1e-9 of parallel somewhere on
the plane: there the den condition is asserted for the pairs within reach of each
other (centres closer than (L_i + L_j) / 2) -- a pair farther apart cannot touch
whichever branch it takes, and contributes an exact zero.
"""

import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import mechanics_ref as ref

pytestmark = pytest.mark.gpu

SEED = 20261019
# offsets for which the restatement's own trajectory keeps the conditions above (found with the
# restatement alone: the first of 0, 10, 20, ... that does)
SEEDS = {'257': SEED + 210, '1000': SEED + 40, 'constant': SEED + 250, 'jitter': SEED + 60, 'order': SEED + 4}
BOUNDS = (41.5, 37.0)          # grid 10 x 9 at max_length 4: a swapped axis shows
NBINS = (17, 23)
W, MAX_LENGTH = 1.0, 4.0
TOL = 1e-12
DEN_CROSS_MIN, D_SMALL_MIN = 1e-2, 1e-3
GX, GY, EDGE_X, EDGE_Y = ref.grid(BOUNDS, MAX_LENGTH)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _model(**kw):
    from lens_amd.mechanics import ContactModel
    kw.setdefault('iterations', 1)
    return ContactModel(max_length=MAX_LENGTH, width=W, seed=SEED, **kw)


def _angles(rng, n):
    """Axis angles stratified modulo pi: no two agents within pi / (2 n) of parallel,
    so that den >= sin^2(pi / 2n) (2.5e-6 at n = 1,000) for EVERY pair."""
    k = rng.permutation(n)
    return np.pi * (k + rng.uniform(0.0, 0.5, n)) / n + np.pi * rng.integers(0, 2, n)


def _condition(rng, x, y, th, L):
    """Swap axis angles between agents until no pair of crossing spines has den <
    DEN_CROSS_MIN and no touching pair 1e-9 < d < D_SMALL_MIN (swaps keep the
    stratified set of angles)."""
    keys = np.arange(len(x))
    for _ in range(500):
        q = ref.pushes(x, y, th, L, keys, W, 0.5)[3]
        bad = (ref.crossing(q) & (q['den'] < DEN_CROSS_MIN)) | (q['contact'] & (q['d'] > 1e-9) & (q['d'] < D_SMALL_MIN))
        if not bad.any():
            return th
        for j in np.unique(np.nonzero(np.triu(bad))[1]):
            m = int(rng.integers(0, len(x)))
            th[j], th[m] = th[m], th[j]
    raise AssertionError('could not draw well-conditioned angles')


def _patch(rng, n, side, at):
    """n capsules, lengths w .. max_length, in a side x side patch."""
    x, y = at[0] + rng.uniform(0, side, n), at[1] + rng.uniform(0, side, n)
    L = rng.uniform(W, MAX_LENGTH, n)
    L[0], L[1] = W, MAX_LENGTH
    return x, y, _condition(rng, x, y, _angles(rng, n), L), L


def _thousand(rng):
    """1,000 agents on 41.5 x 37: on all four walls, in the four corner cells, cell
    (7, 7) empty, cell (4, 3) holding 100 (85 of them discs), lengths from w (a
    disc, half of the agents) to max_length.  The discs keep the count of
    capsule-capsule contacts, each of which has a 1e-3 chance of an ill-conditioned
    normal or closest point after an iteration, in the hundreds; n = 257 is all
    capsules."""
    n = 1000
    x, y = rng.uniform(0, BOUNDS[0], n), rng.uniform(0, BOUNDS[1], n)
    L = rng.uniform(W, MAX_LENGTH, n)
    below = (np.nextafter(BOUNDS[0], 0.0), np.nextafter(BOUNDS[1], 0.0))
    x[0:6], x[6:12] = 0.0, below[0]
    y[12:18], y[18:24] = 0.0, below[1]
    for k, (cx, cy) in enumerate(((0, 0), (0, GY - 1), (GX - 1, 0), (GX - 1, GY - 1))):      # corner cells
        a = slice(24 + 4 * k, 28 + 4 * k)
        x[a] = (cx + rng.uniform(0.05, 0.95, 4)) * EDGE_X
        y[a] = (cy + rng.uniform(0.05, 0.95, 4)) * EDGE_Y
    x[40], y[40] = 0.0, 0.0                                   # and the corners themselves
    x[41], y[41] = below[0], below[1]
    cell = ref.cells(x, y, BOUNDS, MAX_LENGTH)
    move = np.nonzero((cell == 7 * GY + 7) | ((cell == 4 * GY + 3) & (np.arange(n) >= 42)))[0]
    x[move] = rng.uniform(0.1, 3.9, len(move))                # out of the empty and the crowded cell
    crowd = slice(100, 200)
    x[crowd] = (4 + rng.uniform(0.02, 0.98, 100)) * EDGE_X
    y[crowd] = (3 + rng.uniform(0.02, 0.98, 100)) * EDGE_Y
    L[100:185] = W
    L[200:][rng.random(n - 200) < 0.55] = W
    L[50], L[51] = W, MAX_LENGTH
    return x, y, _condition(rng, x, y, _angles(rng, n), L), L


class _Device:
    """One colony's worth of capsules on the device, ld >= n, padding filled with -7."""

    def __init__(self, dev, model, x, y, th, L=None, ld=None, counter=0):
        from lens_amd.lattice import Lattice
        from lens_amd.mechanics import ContactBuffers
        n = len(x)
        self.n, self.ld, self.model = n, ld or max(n, 1), model
        self.lat = Lattice(['glc__D_e'], NBINS, BOUNDS, 10.0, 5.0, device=dev)
        pad = lambda a: np.concatenate([np.asarray(a, dtype=np.float64), np.full(self.ld - n, -7.0)])
        self.loc = torch.from_numpy(np.stack([pad(x), pad(y)])).to(dev).contiguous()
        self.angle = torch.from_numpy(pad(th)).to(dev)
        self.length = None if L is None else torch.from_numpy(pad(L)).to(dev)
        self.bins = torch.full((self.ld,), -7, dtype=torch.int32, device=dev)
        self.ix = torch.full((self.ld,), -7, dtype=torch.int32, device=dev)
        self.buf = ContactBuffers(self.ld, GX * GY, dev, counter=counter)

    def step(self, key=None, model=None):
        from lens_amd.mechanics import contact_step
        contact_step(model or self.model, self.lat, self.loc, self.angle, self.n, self.buf, length=self.length,
                     key=key, bin_lin=self.bins, bin_ix=self.ix)
        torch.cuda.synchronize()

    def host(self):
        n = self.n
        return self.loc[0, :n].cpu().numpy(), self.loc[1, :n].cpu().numpy(), self.angle[:n].cpu().numpy()

    def padding_untouched(self):
        n = self.n
        return (bool((self.loc[:, n:] == -7.0).all()) and bool((self.angle[n:] == -7.0).all()) and
                bool((self.bins[n:] == -7).all()) and bool((self.ix[n:] == -7).all()))


def _check_iterations(d, L, iterations, where, degenerate=False, keys=None, **kw):
    """``iterations`` launches of one iteration each, every one against the
    restatement from the device's state before it.  Returns the worst error."""
    worst = 0.0
    keys = np.arange(d.n) if keys is None else keys
    for it in range(iterations):
        x, y, th = d.host()
        s_global = int(d.buf.counter[0])
        info = {}
        want = ref.iterate(x, y, th, L, keys, BOUNDS, s_global, stiffness=d.model.stiffness, max_length=MAX_LENGTH,
                           width=W, max_push=d.model.max_push, max_turn=d.model.max_turn, jitter=d.model.jitter,
                           jitter_angle=d.model.jitter_angle, seed=d.model.seed, info=info)
        m = info['margins']
        print(where, 'iteration', it, 'margins', m, 'contacts', int(info['contact'].sum()) // 2)
        if not degenerate:
            # the drawn state: every pair.  A state the device produced: every pair
            # within reach (no other pair can touch, whichever branch it takes)
            den = m['den'] if it == 0 else m['den_near']
            assert m['delta'] >= 1e-9 and den >= 1e-9 and m['d'] >= 1e-10, (where, it, m)
            assert m['den_cross'] >= DEN_CROSS_MIN and m['d_small'] >= D_SMALL_MIN, (where, it, m)
        d.step()
        got = d.host()
        err = [float(np.abs(g - w).max()) for g, w in zip(got, want)]
        print(where, 'iteration', it, 'max |x|, |y|, |theta| error', err)
        assert max(err) <= TOL, (where, it, err)
        worst = max(worst, max(err))
        assert int(d.buf.counter[0]) == s_global + 1
        lin, ix = ref.bins(got[0], got[1], NBINS, BOUNDS)
        assert np.array_equal(d.bins[:d.n].cpu().numpy(), lin) and np.array_equal(d.ix[:d.n].cpu().numpy(), ix)
    assert int(d.buf.flags[0]) == 0
    return worst


def test_one_agent(dev):
    d = _Device(dev, _model(), [3.0], [36.5], [0.4], [2.5], ld=64)
    _check_iterations(d, np.array([2.5]), 2, 'n = 1')
    assert np.array_equal(np.stack(d.host()), [[3.0], [36.5], [0.4]])       # nothing to touch: bitwise still
    assert d.padding_untouched()


def test_coincident_centres_take_the_key_order_normal(dev):
    L = np.array([2.0, 3.0])
    d = _Device(dev, _model(), [5.0, 5.0], [7.0, 7.0], [0.2, 1.3], L)
    _check_iterations(d, L, 1, 'coincident', degenerate=True)
    x, y, th = d.host()
    assert x[0] == 5.25 and x[1] == 4.75 and y[0] == 7.0 and y[1] == 7.0    # exact: 0.5 * 0.5 * 1 along +-x
    # the keys decide, not the columns
    d = _Device(dev, _model(), [5.0, 5.0], [7.0, 7.0], [0.2, 1.3], L)
    d.step(key=torch.tensor([1, 0], dtype=torch.int64, device=dev))
    x, _, _ = d.host()
    assert x[0] == 4.75 and x[1] == 5.25


def test_crossing_spines_take_the_centre_line_normal(dev):
    L = np.array([3.0, 3.0])
    # perpendicular spines through each other: the closest points coincide (d = 0), the centres do not
    d = _Device(dev, _model(), [5.0, 5.25], [7.0, 7.0], [0.0, math.pi / 2], L)
    _check_iterations(d, L, 1, 'crossing', degenerate=True)
    x, y, _ = d.host()
    assert x[0] < 5.0 and x[1] > 5.25 and abs(y[0] - 7.0) <= TOL and abs(y[1] - 7.0) <= TOL


def test_257_agents(dev):
    rng = np.random.default_rng(SEEDS['257'])
    x, y, th, L = _patch(rng, 257, 14.0, (9.0, 11.0))
    d = _Device(dev, _model(), x, y, th, L, ld=300)
    _check_iterations(d, L, 3, 'n = 257')
    assert d.padding_untouched()


def test_1000_agents_on_the_10_by_9_grid(dev):
    rng = np.random.default_rng(SEEDS['1000'])
    x, y, th, L = _thousand(rng)
    cell = ref.cells(x, y, BOUNDS, MAX_LENGTH)
    count = np.bincount(cell, minlength=GX * GY)
    assert (GX, GY) == (10, 9) and count.max() >= 100 and count[4 * GY + 3] >= 100 and (count == 0).any()
    assert all(count[c] > 0 for c in (0, GY - 1, (GX - 1) * GY, GX * GY - 1))
    assert (x == 0).any() and (y == 0).any() and (x == np.nextafter(BOUNDS[0], 0)).any() and \
        (y == np.nextafter(BOUNDS[1], 0)).any()
    assert L.min() == W and L.max() == MAX_LENGTH
    d = _Device(dev, _model(), x, y, th, L)
    worst = _check_iterations(d, L, 2, 'n = 1000')
    print('n = 1000 worst error', worst)
    got = d.host()
    assert (got[0] >= 0).all() and (got[0] < BOUNDS[0]).all() and (got[1] >= 0).all() and (got[1] < BOUNDS[1]).all()
    # bin_lin / bin_ix are vk_bin_sites' of the final locations, bit for bit
    lin, ix = d.lat.bin_sites(d.loc, d.n)
    assert torch.equal(lin[:d.n], d.bins[:d.n]) and torch.equal(ix[:d.n], d.ix[:d.n])


def test_constant_length_and_several_iterations_per_launch(dev):
    """length NULL takes the model's constant; a launch of 4 iterations equals 4
    launches of one bit for bit (jitter on: the device counter carries the index)."""
    rng = np.random.default_rng(SEEDS['constant'])
    x, y, th, _ = _patch(rng, 200, 9.0, (1.0, 20.0))
    L = np.full(200, 2.0)
    th = _condition(rng, x, y, th, L)
    kw = dict(length=2.0, jitter=0.02, jitter_angle=0.05)
    a = _Device(dev, _model(**kw), x, y, th, counter=7)
    b = _Device(dev, _model(iterations=4, **kw), x, y, th, counter=7)
    _check_iterations(a, L, 4, 'constant length, jitter')          # two and more launches continue the counter
    b.step()
    assert int(a.buf.counter[0]) == int(b.buf.counter[0]) == 11
    assert torch.equal(a.loc, b.loc) and torch.equal(a.angle, b.angle)
    assert torch.equal(a.bins, b.bins) and torch.equal(a.ix, b.ix)


def test_jitter_equals_the_restatement_with_the_oracle_draws(dev):
    rng = np.random.default_rng(SEEDS['jitter'])
    x, y, th, L = _patch(rng, 257, 14.0, (20.0, 3.0))
    d = _Device(dev, _model(jitter=0.03, jitter_angle=0.05), x, y, th, L, counter=41)
    x0 = d.host()[0].copy()
    _check_iterations(d, L, 2, 'jitter')
    assert int(d.buf.counter[0]) == 43
    # the draws did move agents that touch nothing
    lone = _Device(dev, _model(jitter=0.03, jitter_angle=0.05), [30.0], [30.0], [0.0], [2.0], counter=41)
    lone.step()
    assert lone.host()[0][0] != 30.0 and lone.host()[2][0] != 0.0 and not np.array_equal(d.host()[0], x0)


def test_storage_order_does_not_matter(dev):
    """Permuted columns with the old columns as keys: equal bits, column for column."""
    rng = np.random.default_rng(SEEDS['order'])
    n = 300
    x, y, th, L = _patch(rng, n, 12.0, (25.0, 20.0))
    perm = rng.permutation(n)
    m = _model(iterations=4, jitter=0.01, jitter_angle=0.02)
    a = _Device(dev, m, x, y, th, L, counter=5)
    b = _Device(dev, m, x[perm], y[perm], th[perm], L[perm], counter=5)
    key = torch.from_numpy(perm.astype(np.int64)).to(dev)
    for _ in range(2):
        a.step()
        b.step(key=key)
    p = torch.from_numpy(perm).to(dev)
    assert torch.equal(a.loc[:, p], b.loc) and torch.equal(a.angle[p], b.angle)
    assert torch.equal(a.bins[p], b.bins) and torch.equal(a.ix[p], b.ix)
    assert not torch.equal(a.loc, torch.from_numpy(np.stack([x, y])).to(dev))


def test_too_long_flag(dev):
    edge = min(EDGE_X, EDGE_Y)
    x, y, th = [5.0, 20.0, 30.0], [5.0, 20.0, 30.0], [0.1, 0.2, 0.3]
    ok = _Device(dev, _model(), x, y, th, [2.0, edge, 3.0])
    ok.step()
    assert int(ok.buf.flags[0]) == 0
    ok.buf.check()
    bad = _Device(dev, _model(), x, y, th, [2.0, np.nextafter(edge, np.inf), 3.0])
    bad.step()
    assert int(bad.buf.flags[0]) == 1
    with pytest.raises(ValueError, match='longer than max_length'):
        bad.buf.check()
    const = _Device(dev, _model(length=4.5), x, y, th)         # the constant length is checked too
    const.step()
    assert int(const.buf.flags[0]) == 1


def test_bad_arguments_and_the_empty_colony(dev):
    from lens_amd import native
    lib = native.load()
    d = _Device(dev, _model(), [5.0, 6.0], [5.0, 6.0], [0.1, 0.2], [2.0, 2.0], ld=8)
    before = [t.clone() for t in (d.loc, d.angle, d.bins, d.buf.counter, d.buf.flags)]
    base = d.buf.scratch.data_ptr() + d.buf._off

    def call(p=None, n=2, ld=8, loc=d.loc, angle=d.angle, counter=d.buf.counter, flags=d.buf.flags, bins=d.bins,
             scratch=base, nbytes=d.buf._bytes, nx=NBINS[0], bx=BOUNDS[0]):
        p = p or d.model.vk_params(BOUNDS)
        return lib.vk_contact_step(ctypes.byref(p), n, ld, native.ptr(loc), native.ptr(angle), native.ptr(d.length),
                                   0, native.ptr(counter), native.ptr(flags), nx, NBINS[1], bx, BOUNDS[1],
                                   native.ptr(bins), native.ptr(d.ix), scratch, nbytes, native.stream_handle())

    def params(**kw):
        p = d.model.vk_params(BOUNDS)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    E = native.VK_ERR_ARG
    assert call(n=-1) == E and call(n=9) == E                       # n < 0, ld < n
    assert call(loc=None) == E and call(angle=None) == E and call(bins=None) == E
    assert call(counter=None) == E and call(flags=None) == E
    assert call(scratch=0) == E and call(scratch=base + 8) == E and call(nbytes=d.buf._bytes // 2) == E
    assert call(nx=0) == E and call(bx=0.0) == E and call(bx=float('nan')) == E
    assert call(p=params(iterations=0)) == E
    assert call(p=params(stiffness=0.0)) == E and call(p=params(stiffness=1.5)) == E
    assert call(p=params(width=0.0)) == E and call(p=params(max_length=0.5)) == E
    assert call(p=params(gx=0)) == E and call(p=params(gx=GX + 1)) == E and call(p=params(gy=GY + 1)) == E
    assert b'vk_contact_step' in lib.vk_last_error()
    torch.cuda.synchronize()
    for t, t0 in zip((d.loc, d.angle, d.bins, d.buf.counter, d.buf.flags), before):
        assert torch.equal(t, t0)                                   # nothing was launched
    # n == 0: VK_OK, arrays not needed
    assert call(n=0, ld=0, loc=None, angle=None, bins=None, scratch=0, nbytes=0) == native.VK_OK
    assert lib.vk_contact_scratch_bytes(0, 90) == 0 and lib.vk_contact_scratch_bytes(1000, 90) > 1000 * 60
    assert call() == native.VK_OK                                   # and the good call goes through
    torch.cuda.synchronize()
    assert int(d.buf.counter[0]) == 1
