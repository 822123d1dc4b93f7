"""The mother machine on the device against its NumPy restatement
(tests/mother_machine_ref.py): vk_population_plan bit for bit, the channel
projection and the outflow flag of vk_contact_step_channels at the ABI level, one
colony step against the same step driven by hand, and the whole scenario.

Channels at the ABI level: as tests/test_mechanics_gpu.py, one relaxation
iteration at a time from the device's own state, 1e-12 absolute on x, y, theta
(that file's bound and its reasoning).  The projection adds per agent one cos (of
an angle of a few rad: an ulp, 1e-16, times h <= 1.5 um on x), one sqrt
(correctly rounded on both sides) and one atan2 of magnitude <= pi (an ulp or
two: a few 1e-16 on theta), and both of its parts are continuous, so a tie of
|cos theta| against cmax moves the result by rounding only.  The one branch
that can tie is y against the channel height: |y - height| >= 1e-9 for the
moved centres is asserted on the restatement beside that file's conditions
(DEN_CROSS_MIN, D_SMALL_MIN, no tied branch) before every compared iteration;
nothing is skipped.  States are drawn inside channels, and the seed recorded
here is the first of SEED + 0, 10, 20, ... for which the restatement's own
trajectory keeps the conditions (found with the restatement alone).
"""

import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import mechanics_ref as ref
import mother_machine_ref as mm_ref
from lens_amd import configs, native

pytestmark = pytest.mark.gpu

SEED = 20261019
SEED_257 = SEED + 0            # see the module docstring
BOUNDS = (41.5, 37.0)          # test_mechanics_gpu.py's plane: grid 10 x 9 at max_length 4
NBINS = (17, 23)
W, MAX_LENGTH = 1.0, 4.0
TOL = 1e-12
DEN_CROSS_MIN, D_SMALL_MIN = 1e-2, 1e-3
HEIGHT_MIN = 1e-9
GX, GY, _, _ = ref.grid(BOUNDS, MAX_LENGTH)
CHANNELS = {'channel_height': 30.0, 'channel_space': 2.5, 'spacer_thickness': 0.1}     # 16 lines, the last at 37.5
CH_REF = {'height': 30.0, 'space': 2.5, 'spacer': 0.1}

# the scenario (tests/test_mother_machine_host.py prints the restatement's peak)
STEPS, JITTER, SC_SEED = 600, 0.005, 11
RESTATEMENT_PEAK = 42


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


# ---------------------------------------------------------------------------
# 1. the plan
# ---------------------------------------------------------------------------

PLAN_SIZES = (1, 1023, 1024, 1025, 4099, 262149)      # the last: one block past 256 scan blocks


def _plan(dev, divide, remove, n, fn='vk_population_plan'):
    lib = native.load()
    i32 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    d, r = i32(divide), i32(remove)
    src = torch.full((2 * n + 3,), -7, dtype=torch.int32, device=dev)
    kind = torch.full((2 * n + 3,), -7, dtype=torch.int32, device=dev)
    n_out = torch.full((1,), -7, dtype=torch.int64, device=dev)
    if fn == 'vk_population_plan':
        scratch = torch.empty(int(lib.vk_population_scratch_bytes(n)), dtype=torch.uint8, device=dev)
        rc = lib.vk_population_plan(native.ptr(d), native.ptr(r), n, native.ptr(src), native.ptr(kind),
                                    native.ptr(n_out), native.ptr(scratch), native.stream_handle())
    else:
        scratch = torch.empty(int(lib.vk_divide_scratch_bytes(n)), dtype=torch.uint8, device=dev)
        rc = lib.vk_divide_plan(native.ptr(d), n, native.ptr(src), native.ptr(kind), native.ptr(n_out),
                                native.ptr(scratch), native.stream_handle())
    assert rc == native.VK_OK
    torch.cuda.synchronize()
    return src.cpu().numpy(), kind.cpu().numpy(), int(n_out[0])


def _patterns(n):
    rng = np.random.default_rng(SEED + n)
    z, o = np.zeros(n, dtype=np.int32), np.ones(n, dtype=np.int32)
    both = (rng.random(n) < 0.5).astype(np.int32)
    both[0] = 1
    return {
        'no flags': (z, z), 'all removed': (z, o), 'all removed, all dividing': (o, o), 'all dividing': (o, z),
        'remove and divide on the same agents': (both, both),
        'random 0.3 each': ((rng.random(n) < 0.3).astype(np.int32), (rng.random(n) < 0.3).astype(np.int32)),
        'random, flag values other than 1': ((rng.random(n) < 0.3) * rng.integers(-3, 9, n),
                                             (rng.random(n) < 0.3) * rng.integers(-3, 9, n)),
        'divide NULL': (None, (rng.random(n) < 0.3).astype(np.int32)),
        'both NULL': (None, None),
    }


@pytest.mark.parametrize('n', PLAN_SIZES)
def test_plan_equals_the_restatement_bitwise(dev, n):
    for name, (divide, remove) in _patterns(n).items():
        src, kind, n_out = _plan(dev, divide, remove, n)
        want_src, want_kind, want_n = mm_ref.plan(divide, remove, n)
        assert n_out == want_n, (n, name)
        assert np.array_equal(src[:n_out], want_src) and np.array_equal(kind[:n_out], want_kind), (n, name)
        assert (src[n_out:] == -7).all() and (kind[n_out:] == -7).all(), (n, name)      # nothing written past n_out
        if name.startswith('all removed'):
            assert n_out == 0
        if name == 'all dividing':
            assert n_out == 2 * n


@pytest.mark.parametrize('n', PLAN_SIZES)
def test_plan_without_remove_equals_vk_divide_plan(dev, n):
    rng = np.random.default_rng(SEED - n)
    for divide in (np.zeros(n, dtype=np.int32), np.ones(n, dtype=np.int32), (rng.random(n) < 0.3).astype(np.int32)):
        a = _plan(dev, divide, None, n)
        b = _plan(dev, divide, None, n, fn='vk_divide_plan')
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_plan_bad_arguments(dev):
    lib = native.load()
    n = 8
    flags = torch.zeros(n, dtype=torch.int32, device=dev)
    src = torch.full((2 * n,), -7, dtype=torch.int32, device=dev)
    kind = torch.full((2 * n,), -7, dtype=torch.int32, device=dev)
    n_out = torch.full((1,), -7, dtype=torch.int64, device=dev)
    scratch = torch.empty(int(lib.vk_population_scratch_bytes(n)), dtype=torch.uint8, device=dev)

    def call(n=n, src=src, kind=kind, n_out=n_out, scratch=scratch):
        return lib.vk_population_plan(native.ptr(flags), native.ptr(flags), n, native.ptr(src), native.ptr(kind),
                                      native.ptr(n_out), native.ptr(scratch), native.stream_handle())

    E = native.VK_ERR_ARG
    assert call(n=-1) == E and call(n=0x40000000) == E
    assert call(src=None) == E and call(kind=None) == E and call(n_out=None) == E and call(scratch=None) == E
    assert b'vk_population_plan' in lib.vk_last_error()
    torch.cuda.synchronize()
    assert int(n_out[0]) == -7 and bool((src == -7).all()) and bool((kind == -7).all())     # nothing was launched
    assert lib.vk_population_scratch_bytes(-1) == 0 and lib.vk_population_scratch_bytes(0) >= 16
    assert lib.vk_population_scratch_bytes(1025) >= 2 * 3 * 8
    assert call(n=0, src=None, kind=None) == native.VK_OK               # n == 0: n_out := 0, arrays not needed
    torch.cuda.synchronize()
    assert int(n_out[0]) == 0
    assert call() == native.VK_OK
    torch.cuda.synchronize()
    assert int(n_out[0]) == n and src[:n].tolist() == list(range(n))


# ---------------------------------------------------------------------------
# 2. channels at the ABI level
# ---------------------------------------------------------------------------

def _model(channels=CHANNELS, **kw):
    from lens_amd.mechanics import ContactModel
    kw.setdefault('iterations', 1)
    return ContactModel(max_length=MAX_LENGTH, width=W, seed=SEED, channels=channels, **kw)


def _angles(rng, n):
    """Axis angles stratified modulo pi (test_mechanics_gpu.py): den >= sin^2(pi / 2n) for every pair."""
    k = rng.permutation(n)
    return np.pi * (k + rng.uniform(0.0, 0.5, n)) / n + np.pi * rng.integers(0, 2, n)


def _condition(rng, x, y, th, L):
    """Swap axis angles until no crossing pair has den < DEN_CROSS_MIN and no touching pair
    1e-9 < d < D_SMALL_MIN (test_mechanics_gpu.py)."""
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


def draw_257(seed):
    """257 capsules, lengths w .. max_length, inside the 16 channels (the last one runs to the
    plane's edge), y in [12, 35): a fifth of them above the channel height of 30."""
    rng = np.random.default_rng(seed)
    n, space, edge = 257, CH_REF['space'], W / 2 + CH_REF['spacer']
    c = rng.integers(0, 16, n)
    x = c * space + edge + rng.uniform(0.0, space - 2 * edge, n)
    y = rng.uniform(12.0, 35.0, n)
    L = rng.uniform(W, MAX_LENGTH, n)
    L[0], L[1] = W, MAX_LENGTH
    return x, y, _condition(rng, x, y, _angles(rng, n), L), L


def conditions(info, it):
    """test_mechanics_gpu.py's conditions on the restatement's margins, and the height's."""
    m = info['margins']
    den = m['den'] if it == 0 else m['den_near']
    return (m['delta'] >= 1e-9 and den >= 1e-9 and m['d'] >= 1e-10 and m['den_cross'] >= DEN_CROSS_MIN and
            m['d_small'] >= D_SMALL_MIN and info['height_margin'] >= HEIGHT_MIN)


class _Device:
    """One colony's worth of capsules on the device, ld >= n, padding filled with -7."""

    def __init__(self, dev, model, x, y, th, L, ld=None, counter=0):
        from lens_amd.lattice import Lattice
        from lens_amd.mechanics import ContactBuffers
        n = len(x)
        self.n, self.ld, self.model = n, ld or max(n, 1), model
        self.lat = Lattice(['glc__D_e'], NBINS, BOUNDS, 10.0, 5.0, device=dev)
        pad = lambda a: np.concatenate([np.asarray(a, dtype=np.float64), np.full(self.ld - n, -7.0)])
        self.loc = torch.from_numpy(np.stack([pad(x), pad(y)])).to(dev).contiguous()
        self.angle = torch.from_numpy(pad(th)).to(dev)
        self.length = torch.from_numpy(pad(L)).to(dev)
        self.bins = torch.full((self.ld,), -7, dtype=torch.int32, device=dev)
        self.ix = torch.full((self.ld,), -7, dtype=torch.int32, device=dev)
        self.outflow = torch.full((self.ld,), -7, dtype=torch.int32, device=dev)
        self.buf = ContactBuffers(self.ld, GX * GY, dev, counter=counter)

    def step(self, model=None):
        from lens_amd.mechanics import contact_step
        contact_step(model or self.model, self.lat, self.loc, self.angle, self.n, self.buf, length=self.length,
                     bin_lin=self.bins, bin_ix=self.ix, outflow=self.outflow)
        torch.cuda.synchronize()

    def host(self):
        n = self.n
        return self.loc[0, :n].cpu().numpy(), self.loc[1, :n].cpu().numpy(), self.angle[:n].cpu().numpy()

    def padding_untouched(self):
        n = self.n
        return (bool((self.loc[:, n:] == -7.0).all()) and bool((self.angle[n:] == -7.0).all()) and
                bool((self.bins[n:] == -7).all()) and bool((self.outflow[n:] == -7).all()))


def _check_iterations(d, L, iterations, where):
    """``iterations`` launches of one iteration each, every one against the restatement from
    the device's state before it; returns the outflow flags of every launch."""
    keys, flags = np.arange(d.n), []
    for it in range(iterations):
        x, y, th = d.host()
        s_global = int(d.buf.counter[0])
        info = {}
        want = mm_ref.iterate(x, y, th, L, keys, BOUNDS, s_global, CH_REF, info=info, stiffness=d.model.stiffness,
                              max_length=MAX_LENGTH, width=W, max_push=d.model.max_push, max_turn=d.model.max_turn,
                              jitter=d.model.jitter, jitter_angle=d.model.jitter_angle, seed=d.model.seed)
        print(where, 'iteration', it, 'margins', info['margins'], 'height margin', info['height_margin'],
              'contacts', int(info['contact'].sum()) // 2, 'above', int(want[3].sum()))
        assert conditions(info, it), (where, it, info['margins'], info['height_margin'])
        d.step()
        got = d.host()
        err = [float(np.abs(g - w).max()) for g, w in zip(got, want[:3])]
        print(where, 'iteration', it, 'max |x|, |y|, |theta| error', err)
        assert max(err) <= TOL, (where, it, err)
        out = d.outflow[:d.n].cpu().numpy()
        assert np.array_equal(out, want[3].astype(np.int32)), (where, it)
        flags.append(out)
        lin, ix = ref.bins(got[0], got[1], NBINS, BOUNDS)
        assert np.array_equal(d.bins[:d.n].cpu().numpy(), lin) and np.array_equal(d.ix[:d.n].cpu().numpy(), ix)
    assert int(d.buf.flags[0]) == 0
    return flags


def _single(dev, x, y, th, L, **kw):
    d = _Device(dev, _model(**kw), [x], [y], [th], [L], ld=8)
    flags = _check_iterations(d, np.array([L]), 2, 'single (%g, %g, %g, %g)' % (x, y, th, L))
    assert d.padding_untouched()
    return d.host(), flags


def test_a_long_tilted_cell_is_turned_and_clamped(dev):
    # channel 4 of [10, 12.5): lo = 10.6, hi = 11.9; h = 1.3: |cos| <= 0.5
    (x, y, th), flags = _single(dev, 11.8, 12.0, 0.2, 3.6)
    assert abs(abs(math.cos(th[0])) - 0.5) <= 1e-15 and 0.0 < th[0] < math.pi / 2 and abs(x[0] - 11.25) <= 1e-14
    assert y[0] == 12.0 and flags[0][0] == 0
    # the signs of cos and sin are kept: the mirrored cell turns the other way
    (x, y, th), _ = _single(dev, 10.7, 12.0, math.pi - 0.2, 3.6)
    assert abs(math.cos(th[0]) + 0.5) <= 1e-15 and math.sin(th[0]) > 0 and abs(x[0] - 11.25) <= 1e-14
    (x, y, th), _ = _single(dev, 11.0, 12.0, -0.2, 3.6)
    assert abs(math.cos(th[0]) - 0.5) <= 1e-15 and math.sin(th[0]) < 0


def test_a_cell_above_the_channels_is_untouched_and_flagged(dev):
    (x, y, th), flags = _single(dev, 12.4, 30.5, 0.2, 3.6)
    assert x[0] == 12.4 and y[0] == 30.5 and th[0] == 0.2 and flags[0][0] == 1 and flags[1][0] == 1
    # exactly at the height: not above
    (x, y, th), flags = _single_exact(dev, 12.4, 30.0)
    assert flags[0] == 0 and x[0] != 12.4


def _single_exact(dev, x, y):
    """y == height exactly (the one deliberate tie: y > height is false on both sides)."""
    d = _Device(dev, _model(), [x], [y], [0.2], [3.6], ld=8)
    d.step()
    return d.host(), d.outflow[:1].cpu().numpy()


def test_a_cell_right_of_the_last_line_takes_the_planes_edge(dev):
    # the last line stands at 37.5; the plane ends at 41.5
    (x, y, th), flags = _single(dev, 41.2, 5.0, 0.0, 3.0)
    assert th[0] == 0.0 and x[0] == np.nextafter(41.5, 0.0) - 1.0 and flags[0][0] == 0
    (x, y, th), _ = _single(dev, 37.6, 5.0, 0.1, 3.0)
    assert x[0] > 38.1 + 0.9 and th[0] == 0.1


def test_a_disc_keeps_its_angle(dev):
    (x, y, th), flags = _single(dev, 10.1, 5.0, 0.3, 1.0)
    assert th[0] == 0.3 and x[0] == 4 * 2.5 + (0.5 + 0.1) and flags[0][0] == 0      # lo of channel 4


def test_257_agents_in_channels(dev):
    x, y, th, L = draw_257(SEED_257)
    d = _Device(dev, _model(), x, y, th, L, ld=300)
    flags = _check_iterations(d, L, 3, 'n = 257')
    assert d.padding_untouched()
    assert 20 <= flags[0].sum() <= 100                       # both sides of the height are populated
    got = d.host()
    below = got[1] <= CH_REF['height']
    assert (mm_ref.channel_of(got[0], BOUNDS, 2.5)[below] == mm_ref.channel_of(x, BOUNDS, 2.5)[below]).all()


def test_the_outflow_flag_sticks_through_the_iterations_of_a_launch(dev):
    """A launch of 3 iterations equals 3 launches of one, bit for bit, and its flags are
    the OR of theirs (jitter on, so that centres cross the height both ways)."""
    x, y, th, L = draw_257(SEED_257)
    y = np.where(np.arange(257) % 2 == 0, 30.0 + (y - 25.5) * 0.004, y)      # half of them within 0.04 of the height
    kw = dict(jitter=0.03, jitter_angle=0.02)
    a = _Device(dev, _model(**kw), x, y, th, L, counter=3)
    b = _Device(dev, _model(iterations=3, **kw), x, y, th, L, counter=3)
    flags = []
    for _ in range(3):
        a.step()
        flags.append(a.outflow[:257].clone())
    b.step()
    assert torch.equal(a.loc, b.loc) and torch.equal(a.angle, b.angle) and torch.equal(a.bins, b.bins)
    assert torch.equal(b.outflow[:257], flags[0] | flags[1] | flags[2])
    assert not torch.equal(flags[0], flags[2]) and not torch.equal(b.outflow[:257], flags[2])


def _raw_call(d, fn, ch, outflow):
    lib = native.load()
    p = d.model.vk_params(BOUNDS)
    args = [ctypes.byref(p), d.n, d.ld, native.ptr(d.loc), native.ptr(d.angle), native.ptr(d.length), 0,
            native.ptr(d.buf.counter), native.ptr(d.buf.flags), NBINS[0], NBINS[1], BOUNDS[0], BOUNDS[1],
            native.ptr(d.bins), native.ptr(d.ix), d.buf.scratch.data_ptr() + d.buf._off, d.buf._bytes]
    if fn == 'vk_contact_step_channels':
        args += [ch, native.ptr(outflow)]
    return getattr(lib, fn)(*args, native.stream_handle())


def test_null_channels_equal_vk_contact_step_bitwise(dev):
    x, y, th, L = draw_257(SEED_257)
    m = _model(channels=None, iterations=3, jitter=0.01, jitter_angle=0.02)
    a = _Device(dev, m, x, y, th, L, ld=300)
    b = _Device(dev, m, x, y, th, L, ld=300)
    assert _raw_call(a, 'vk_contact_step', None, None) == native.VK_OK
    assert _raw_call(b, 'vk_contact_step_channels', None, b.outflow) == native.VK_OK
    torch.cuda.synchronize()
    assert torch.equal(a.loc, b.loc) and torch.equal(a.angle, b.angle) and torch.equal(a.bins, b.bins)
    assert torch.equal(a.ix, b.ix) and bool((b.outflow == -7).all())          # outflow is not written without channels
    assert not torch.equal(a.loc[0, :257], torch.from_numpy(x).to(dev))
    # and with channels the same state moves differently
    c = _Device(dev, _model(iterations=3, jitter=0.01, jitter_angle=0.02), x, y, th, L, ld=300)
    c.step()
    assert not torch.equal(a.loc, c.loc)


def test_channels_bad_arguments(dev):
    d = _Device(dev, _model(), [5.0, 6.0], [5.0, 6.0], [0.1, 0.2], [2.0, 2.0], ld=8)
    before = [t.clone() for t in (d.loc, d.angle, d.bins, d.outflow, d.buf.counter)]

    def call(**kw):
        ch = d.model.vk_channels(BOUNDS)
        for k, v in kw.items():
            setattr(ch, k, v)
        return _raw_call(d, 'vk_contact_step_channels', ctypes.byref(ch), d.outflow)

    E = native.VK_ERR_ARG
    assert call(height=0.0) == E and call(height=37.5) == E and call(height=float('nan')) == E
    assert call(space=1.1) == E and call(spacer=-0.1) == E and call(spacer=0.8) == E
    assert call(n_lines=0) == E and call(n_lines=15) == E and call(n_lines=17) == E
    assert b'vk_contact_step_channels' in native.load().vk_last_error()
    torch.cuda.synchronize()
    for t, t0 in zip((d.loc, d.angle, d.bins, d.outflow, d.buf.counter), before):
        assert torch.equal(t, t0)                                   # nothing was launched
    assert call() == native.VK_OK
    ch = d.model.vk_channels(BOUNDS)
    assert _raw_call(d, 'vk_contact_step_channels', ctypes.byref(ch), None) == native.VK_OK      # outflow is nullable
    torch.cuda.synchronize()
    assert int(d.buf.counter[0]) == 2 and d.outflow[:2].tolist() == [0, 0]


# ---------------------------------------------------------------------------
# 3. and 4. the colony
# ---------------------------------------------------------------------------

def _mm_colony(dev, mechanics=True, capacity=64):
    """The reference configuration: configs.mother_machine's three cells (CellModel 'growth',
    0.6 % per second, division at 2.6 fL) with glc_lct kinetics on the 10 x 10 lattice."""
    from lens_amd.cells import CellModel
    from lens_amd.colony import Colony
    from lens_amd.lattice import Lattice
    from lens_amd.mechanics import ContactModel
    mm = configs.mother_machine()
    cfg = configs.glc_lct_config()
    nb = mm['n_bins']
    start = {'glc__D_e': configs.gaussian_bump_field(nb), 'lcts_e': np.full(nb, 10.0)}
    lat = Lattice(['glc__D_e', 'lcts_e'], nb, mm['bounds'], 10.0, mm['diffusion'], device=dev, initial=start)
    model = ContactModel(jitter=JITTER, seed=SC_SEED, channels=mm['channels'])
    cells = CellModel(model='growth', growth_rate=mm['growth_rate'], division_volume=mm['division_volume'],
                      initial_mass=mm['mass'])
    col = Colony(cfg, 3, capacity=capacity, device=dev, integrator='dopri5', environment=lat, cells=cells,
                 mechanics=model if mechanics else None)
    col.set_agents(location=mm['location'])
    col.cell[native.VK_CELL_ANGLE, :3] = torch.from_numpy(mm['angle']).to(dev)
    col.gather_external()
    return col, model, mm


@pytest.fixture(scope='module')
def restatement():
    """The restatement's scenario, run once until its first cell leaves: that step's index."""
    sc = mm_ref.Scenario(configs.mother_machine(), jitter=JITTER, seed=SC_SEED)
    first = None
    for s in range(STEPS):
        sc.step()
        if sc.last_removed:
            first = s
            break
    assert first is not None and first > 50
    return first


def _same(a, b, where):
    assert a.n == b.n, where
    n = a.n
    for m in a.lattice.molecules:
        assert torch.equal(a.lattice.owned(m), b.lattice.owned(m)), (where, m)
    assert a.agent_array_names() == b.agent_array_names()
    for name in a.agent_array_names() + ['bin_lin', 'bin_ix']:
        assert torch.equal(getattr(a, name)[..., :n], getattr(b, name)[..., :n]), (where, name)


def test_one_colony_step_equals_the_step_driven_by_hand(dev, restatement):
    """Up to and including the step after the one in which the restatement's first cell
    leaves: step() of the colony with channels against a colony without mechanics driven by
    hand -- the contact launch with channels, the rest of the step, remove(outflow), division."""
    from lens_amd.mechanics import ContactBuffers, contact_step
    a, model, _ = _mm_colony(dev)
    b, _, _ = _mm_colony(dev, mechanics=False)
    grid = model.grid(b.lattice.bounds)
    buf = ContactBuffers(b.ld, grid[0] * grid[1], dev)
    outflow = torch.zeros(b.ld, dtype=torch.int32, device=dev)
    removed = []
    for step in range(restatement + 2):
        a.step(1.0)
        contact_step(model, b.lattice, b.location, b.cell[native.VK_CELL_ANGLE], b.n, buf,
                     length=b.cell[native.VK_CELL_LENGTH], outflow=outflow)
        b.refresh_bins()
        b.kinetics(1.0)
        b.gather_external()
        b.lattice.diffuse(1.0)
        b._step_exchange()
        removed.append(b.remove(outflow))
        b.grow_and_divide(1.0)
        b.time += 1.0
        b.step_index += 1
        assert b.ld == buf.ld                       # capacity 64 holds the colony: the buffers stay
        if step >= restatement:
            torch.cuda.synchronize()
            _same(a, b, step)
    print('removed per step', [(s, r) for s, r in enumerate(removed) if r], 'restatement', restatement)
    assert removed[restatement] >= 1 and sum(removed[:restatement]) == 0       # the device agrees on the step
    a.check_status()
    with pytest.raises(ValueError, match='channels'):
        a.capture(1.0, 1)


def test_without_cells_the_outflow_leaves_through_remove(dev):
    """A colony with channels and no cells: step() against a plain colony driven by hand -- the
    contact launch with channels on its arrays, the step, remove(outflow)."""
    from lens_amd.colony import Colony
    from lens_amd.lattice import Lattice
    from lens_amd.mechanics import ContactBuffers, ContactModel, contact_step
    from lens_amd.rate_law_compiler import compile_rate_laws
    n0, nx, bound = 300, 32, 64.0
    cfg = configs.glc_lct_config()
    t = compile_rate_laws(cfg['reactions'], cfg['kinetic_parameters'])
    model = ContactModel(jitter=0.02, jitter_angle=0.02, seed=SC_SEED,
                         channels={'channel_height': 40.0, 'channel_space': 4.0})
    rng = np.random.default_rng(SEED + 3)
    loc = np.stack([rng.integers(0, 16, n0) * 4.0 + rng.uniform(0.6, 3.4, n0), rng.uniform(25.0, 45.0, n0)])
    params, conc = configs.heterogeneous_colony(t, cfg, n0)

    def colony(mechanics):
        start = {'glc__D_e': configs.gaussian_bump_field((nx, nx)), 'lcts_e': np.full((nx, nx), 10.0)}
        lat = Lattice(['glc__D_e', 'lcts_e'], (nx, nx), (bound, bound), 10.0, 5.0, device=dev, initial=start)
        col = Colony(cfg, n0, device=dev, integrator='dopri5', environment=lat, table=t, mechanics=mechanics)
        col.set_agents(params=params, conc=conc, location=loc)
        col.gather_external()
        return col

    a, b = colony(model), colony(None)
    assert 'mech_angle' in a.agent_array_names() and a.outflow.shape[0] == a.ld
    angle = a.mech_angle.clone()
    grid = model.grid(b.lattice.bounds)
    buf = ContactBuffers(b.ld, grid[0] * grid[1], dev)
    outflow = torch.zeros(b.ld, dtype=torch.int32, device=dev)
    ns = [a.n]
    for step in range(3):
        a.step(1.0)
        contact_step(model, b.lattice, b.location, angle, b.n, buf, outflow=outflow)
        keep = outflow[:b.n] == 0
        b.refresh_bins()
        b.kinetics(1.0)
        b.gather_external()
        b.lattice.diffuse(1.0)
        b._step_exchange()
        angle[:int(keep.sum())] = angle[:b.n][keep]
        assert b.remove(outflow) == int((~keep).sum())
        b.time += 1.0
        b.step_index += 1
        torch.cuda.synchronize()
        assert a.n == b.n and torch.equal(a.mech_angle[:a.n], angle[:a.n]), step
        for m in a.lattice.molecules:
            assert torch.equal(a.lattice.owned(m), b.lattice.owned(m)), (step, m)
        for name in b.agent_array_names() + ['bin_lin', 'bin_ix']:
            assert torch.equal(getattr(a, name)[..., :a.n], getattr(b, name)[..., :a.n]), (step, name)
        ns.append(a.n)
    print('n per step', ns)
    assert 50 <= ns[0] - ns[1] <= 100 and ns[1] >= ns[2] >= ns[3] > 150       # a quarter starts above the channels
    assert not bool((a.location[1, :a.n] > 40.0).any())
    a.check_status()
    with pytest.raises(ValueError, match='channels'):
        a.capture(1.0, 1)


def test_the_scenario_on_the_device(dev):
    """The host scenario's four assertions (mother_machine_ref.check_scenario) after every one
    of the 600 steps of the device colony, plus check_status(); and the final population is at
    most twice the restatement's recorded peak, so a colony that never drains fails.
    Measured on an MI355X: peak 42, final 39, 24 removed -- the restatement's own figures."""
    a, model, mm = _mm_colony(dev)
    space, height = mm['channels']['channel_space'], mm['channels']['channel_height']
    root_channel = mm_ref.channel_of(mm['location'][0], mm['bounds'], space)
    removed = np.zeros(mm_ref.n_lines(mm['bounds'], space), dtype=np.int64)
    state = {'ids': set(a.agent_ids())}

    def step():
        a.step(1.0)
        a.check_status()
        n = a.n
        x, y = a.location[:, :n].cpu().numpy()
        ids = a.agent_ids()
        here = set(ids)
        # an agent of the last step that is gone and left no daughter was removed; ids are the
        # root's ('0', '1', '2') followed by the path bits, so the root is the first character
        for i in state['ids'] - here:
            if i + '0' not in here:
                removed[root_channel[int(i[0])]] += 1
        state.update(x=x, y=y, root=a.lin_root[:n].cpu().numpy(),
                     newborn=np.array([i not in state['ids'] for i in ids], dtype=bool), ids=here)

    pop = mm_ref.check_scenario(
        lambda: a.n, step,
        lambda: bool((mm_ref.channel_of(state['x'], mm['bounds'], space) == root_channel[state['root']]).all()),
        lambda: bool(((state['y'] > height) & ~state['newborn']).any()),
        lambda: removed, STEPS, sorted(set(root_channel.tolist())))
    print('device scenario: peak population', max(pop), 'final', pop[-1], 'removed', int(removed.sum()))
    assert pop[-1] <= 2 * RESTATEMENT_PEAK
