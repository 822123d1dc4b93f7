"""vk_motility_step_static and vk_flagella_step_static against the NumPy restatement
(tests/static_field_ref.py: the restated plane steps of motility_ref.py / flagella_ref.py, fed
the gradient at each agent's own position), at the ABI level.  The construction is that of
tests/test_motility_gpu.py and tests/test_flagella_gpu.py, whose states, device wrappers and
comparisons are used as they are.

Tolerances.  The plane tests hold every continuous row to 1e-12 (derived in their module
docstrings).  There the ligand is the same double on both sides; here it is computed.
  linear: dx, dy, the squares, the sum, sqrt, / 1000, base + slope d are correctly rounded
  operations in the same order on both sides: the ligand is bitwise equal, the bound stays
  1e-12.
  gaussian, exponential: one exp / pow of bitwise equal arguments, held to the OpenCL limits
  (3 and 16 ulp), NumPy's within 1: the ligand agrees to 1e-13 relative with a 25-fold margin
  (tests/test_static_field_gpu.py holds the kernels to that).  It enters the receptor's free
  energy through log((1 + L / K_off) / (1 + L / K_on)), whose sensitivity to a relative change
  of L is L d/dL log(...) = L / (K_off + L) - L / (K_on + L), of magnitude below 1.  That is
  multiplied by the receptor counts and summed: (n_Tar + n_Tsr) * 1e-13 = 18e-13 = 1.8e-12
  in F, hence (|dP / dF| = P (1 - P) <= P) relative in P_on, added to the existing 1e-12
  budget: 2.8e-12, rounded to 3e-12.
n_methyl is computed before the ligand is used: bitwise after one update.  Over k updates the
bounds are k times the single-update ones, as in the plane tests.

The discrete results (motor state, thrust, masks, bins) are required only where the
restatement's own decisions are not ties within rounding (switch >= 1e-9, edge >= 1e-9, for
flagella structural >= 1e-9); asserted on the restatement alone.  SEED is the recorded seed.

The field: bounds (34, 57.5) um with the centre inside the plane, so that the 1 / 1000 scaling
does not flatten it: exponential base 1e4 and scale 0.6 span 0.6 to 1, linear 0.1 to 0.7,
gaussian (deviation 0.03 mm) 0.2 to 1 -- the receptor's sensitive range (K_Tar_off 0.02,
K_Tar_on 0.5 mM).
"""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import flagella_ref as fref
import motility_ref as mref
import static_field_ref as sref
import test_flagella_gpu as fbase
import test_motility_gpu as base

pytestmark = pytest.mark.gpu

SEED = 20261020
NX, NY, BOUNDS, DT = base.NX, base.NY, base.BOUNDS, base.DT
CENTER = [0.4, 0.3]
GRADIENTS = {
    'linear': {'type': 'linear', 'molecules': {'MeAsp': {'center': CENTER, 'base': 0.1, 'slope': 10.0}}},
    'gaussian': {'type': 'gaussian', 'molecules': {'MeAsp': {'center': CENTER, 'deviation': 0.03}}},
    'exponential': {'type': 'exponential', 'molecules': {'MeAsp': {'center': CENTER, 'base': 1e4, 'scale': 0.6}}},
}
SCALE = {'linear': 1, 'gaussian': 3, 'exponential': 3}      # x 1e-12, the module docstring


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _static(kind):
    from lens_amd.static_field import StaticField
    return StaticField(['MeAsp'], BOUNDS, GRADIENTS[kind], n_bins=(NX, NY))


def _model(**kw):
    from lens_amd.motility import MotilityModel
    return MotilityModel(seed=SEED, **kw)


class _Coarse(base._Device):
    """The plane test's device arrays, stepped in a StaticField."""

    def __init__(self, dev, model, field, motil, loc, **kw):
        super().__init__(dev, model, np.zeros((NX, NY)), motil, loc, **kw)
        self.lat = field


class _Flagella(fbase._Device):
    def __init__(self, dev, model, field, state, **kw):
        super().__init__(dev, model, np.zeros((NX, NY)), state, **kw)
        self.lat = field


@pytest.mark.parametrize('kind', sorted(GRADIENTS))
def test_one_update_from_random_states(dev, kind):
    n = 4096
    rng = np.random.default_rng(SEED)
    model, field = _model(), _static(kind)
    motil, loc = base._states(rng, n, model)
    L = sref._ligand(field, 'MeAsp', loc)
    assert 0.05 < L.min() < L.max() < 1.2 and L.max() - L.min() > 0.3, (L.min(), L.max())
    d = _Coarse(dev, model, field, motil, loc, counter=7)
    margins = {}
    bins = sref.motility_step(model, field, motil, loc, DT, 1, 7, margins=margins)
    assert margins['switch'] >= 1e-9 and margins['edge'] >= 1e-9, margins
    nm = motil[mref.R['n_methyl']]
    assert (nm == 0.0).any() and (nm == 8.0).any()
    assert set(np.unique(motil[mref.R['motor_state']])) == {0.0, 1.0}
    d.step(DT, 1)
    got = d.host()
    base._compare(got, (motil, loc, bins), SCALE[kind], 'one update, ' + kind)
    assert np.array_equal(got[0][mref.R['n_methyl']], nm)                # bitwise
    assert int(d.counter[0]) == 8
    assert np.array_equal(d.ix[:n].cpu().numpy(), bins // NY)
    assert (got[1] >= 0).all() and (got[1][0] < BOUNDS[0]).all() and (got[1][1] < BOUNDS[1]).all()


@pytest.mark.parametrize('kind', ['exponential', 'linear'])
def test_trajectory_and_substeps(dev, kind):
    """20 calls of 0.1 s equal 2 calls of 1 s with 10 substeps bit for bit: every inner update
    senses the field where the one before it left the agent, whichever launch it is in."""
    n = 512
    rng = np.random.default_rng(SEED + 1)
    model, field = _model(), _static(kind)
    motil, loc = base._states(rng, n, model)
    motil[mref.R['n_methyl']] = rng.uniform(0.5, 7.5, n)
    a = _Coarse(dev, model, field, motil, loc, counter=100)
    b = _Coarse(dev, model, field, motil, loc, counter=100)
    for _ in range(20):
        a.step(DT, 1)
    for _ in range(2):
        b.step(1.0, 10)
    assert torch.equal(a.motil, b.motil) and torch.equal(a.loc, b.loc) and torch.equal(a.bins, b.bins)
    assert int(a.counter[0]) == int(b.counter[0]) == 120
    margins = {}
    for s in range(20):
        bins = sref.motility_step(model, field, motil, loc, DT, 1, 100 + s, margins=margins)
    assert margins['switch'] >= 1e-9 and margins['edge'] >= 1e-9, margins
    worst = base._compare(a.host(), (motil, loc, bins), 20 * SCALE[kind], 'trajectory, ' + kind)
    assert worst['n_methyl'] <= 20 * SCALE[kind] * 1e-12


def test_position_not_bin(dev):
    """Two agents in one bin at different positions sense different ligand."""
    model, field = _model(), _static('exponential')
    motil = np.zeros((9, 2))
    motil[mref.R['n_methyl']], motil[mref.R['chemoreceptor_activity']] = 3.0, 1.0 / 3.0
    loc = np.array([[20.1, 21.9], [30.2, 32.3]])          # bins of 2.0 x 2.5 um: both in (10, 12)
    assert len(set((mref.bin_axis(loc[0], NX, BOUNDS[0]) * NY + mref.bin_axis(loc[1], NY, BOUNDS[1])).tolist())) == 1
    d = _Coarse(dev, model, field, motil, loc, counter=0)
    sref.motility_step(model, field, motil, loc, DT, 1, 0)
    d.step(DT, 1)
    got = d.host()[0][mref.R['chemoreceptor_activity']]
    want = motil[mref.R['chemoreceptor_activity']]
    assert abs(want[0] - want[1]) > 1e-3 * want[0]
    assert np.all(np.abs(got - want) <= 3e-12 * want)


def test_keys_not_columns_pick_the_draws(dev):
    n = 300
    rng = np.random.default_rng(SEED + 2)
    model, field = _model(substeps=3), _static('exponential')
    motil, loc = base._states(rng, n, model)
    perm = rng.permutation(n)
    a = _Coarse(dev, model, field, motil, loc, counter=5)
    b = _Coarse(dev, model, field, motil[:, perm], loc[:, perm], counter=5)
    key = torch.from_numpy(perm.astype(np.int64)).to(dev)
    for _ in range(3):
        a.step(0.3, None)
        b.step(0.3, None, key=key)
    p = torch.from_numpy(perm).to(dev)
    assert torch.equal(a.motil[:, p], b.motil) and torch.equal(a.loc[:, p], b.loc) and torch.equal(a.bins[p], b.bins)


@pytest.mark.parametrize('n,ld', [(1, 1), (1, 64), (63, 70), (65, 128)])
def test_edge_sizes_leave_the_padding_untouched(dev, n, ld):
    rng = np.random.default_rng(SEED + 3)
    model, field = _model(), _static('exponential')
    motil, loc = base._states(rng, n, model)
    d = _Coarse(dev, model, field, motil, loc, ld=ld, counter=3)
    d.step(DT, 2)
    assert int(d.counter[0]) == 5
    assert bool((d.motil[:, n:] == -7.0).all()) and bool((d.loc[:, n:] == -7.0).all())
    assert bool((d.bins[n:] == -7).all()) and bool((d.ix[n:] == -7).all())
    margins = {}
    bins = sref.motility_step(model, field, motil, loc, DT, 2, 3, margins=margins)
    assert margins['switch'] >= 1e-9 and margins['edge'] >= 1e-9, margins
    base._compare(d.host(), (motil, loc, bins), 2 * SCALE['exponential'], 'n = %d' % n)


def test_a_bad_spec_is_refused(dev):
    """The launch checks the spec it is handed: nothing runs with a zero deviation."""
    import ctypes
    from lens_amd import native
    rng = np.random.default_rng(SEED + 4)
    model, field = _model(), _static('gaussian')
    motil, loc = base._states(rng, 8, model)
    d = _Coarse(dev, model, field, motil, loc)
    bad = native.VkGradientSpec(native.VK_GRADIENT_GAUSSIAN, 1.0, 1.0, 0.0, 0.0)
    p = model.vk_params()
    rc = native._lib.vk_motility_step_static(
        ctypes.byref(p), 8, 8, 0.1, 1, native.ptr(d.motil), native.ptr(d.loc), 0, ctypes.byref(bad), NX, NY, BOUNDS[0],
        BOUNDS[1], native.ptr(d.counter), native.ptr(d.bins), 0, native.stream_handle())
    assert rc == native.VK_ERR_ARG and int(d.counter[0]) == 0
    assert np.array_equal(d.host()[0], motil)


# -- the multi-flagellar motor ------------------------------------------------------------

def _flagella_model(k):
    from lens_amd.motility import FlagellaModel, MotilityModel
    return MotilityModel(seed=SEED, initial_ligand=1e-2, flagella=FlagellaModel(k))


def _flagella_states(rng, n, k):
    """The plane test's random states with every agent at k flagella (have = target = k)."""
    motil, flag, flag_int, loc = fbase._states(rng, n)
    flag_int[0], flag_int[1] = k, k
    mask = flag_int[2].view(np.uint32).astype(np.uint64) & ((np.uint64(1) << np.uint64(k)) - np.uint64(1))
    flag_int[2] = mask.astype(np.uint32).view(np.int32)
    return motil, flag, flag_int, loc


@pytest.mark.parametrize('k', [0, 5, 32])
def test_flagella_one_update(dev, k):
    n = 512
    rng = np.random.default_rng(SEED + 10 + k)
    model, field = _flagella_model(k), _static('exponential')
    state = _flagella_states(rng, n, k)
    d = _Flagella(dev, model, field, state, counter=7)
    motil, flag, flag_int, loc = fbase._copy(state)
    margins = {}
    bins = sref.flagella_step(model, field, motil, flag, flag_int, loc, fbase.H, 1, 7, margins=margins)
    assert 'edge' in margins and fbase._margins_ok(margins), margins
    d.step(fbase.H, 1)
    got = d.host()
    fbase._compare(got, (motil, flag, flag_int, loc, bins), SCALE['exponential'], 'flagella one update, k = %d' % k)
    assert np.array_equal(got[0][fref.R['n_methyl']], motil[fref.R['n_methyl']])        # bitwise
    assert int(d.counter[0]) == 8 and d.padding_untouched()


@pytest.mark.parametrize('k', [0, 5, 32])
def test_flagella_trajectory_and_substeps(dev, k):
    n = 512
    hs = fbase.HS
    rng = np.random.default_rng(SEED + 20 + k)
    model, field = _flagella_model(k), _static('exponential')
    state = _flagella_states(rng, n, k)
    state[0][fref.R['n_methyl']] = rng.uniform(0.5, 7.5, n)
    a = _Flagella(dev, model, field, state, counter=100)
    b = _Flagella(dev, model, field, state, counter=100)
    for _ in range(20):
        a.step(hs, 1)
    for _ in range(2):
        b.step(10 * hs, 10)
    assert all(torch.equal(x, y) for x, y in zip(a.tensors(), b.tensors()))
    assert int(a.counter[0]) == int(b.counter[0]) == 120
    motil, flag, flag_int, loc = fbase._copy(state)
    margins = {}
    for s in range(20):
        bins = sref.flagella_step(model, field, motil, flag, flag_int, loc, hs, 1, 100 + s, margins=margins)
    assert fbase._margins_ok(margins), margins
    worst = fbase._compare(a.host(), (motil, flag, flag_int, loc, bins), 20 * SCALE['exponential'],
                           'flagella trajectory, k = %d' % k)
    assert worst['n_methyl'] <= 20 * SCALE['exponential'] * 1e-12
