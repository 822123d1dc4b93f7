"""Colony(stochastic=StochasticModel(...)): the per-agent counts (``ssa``) and keys
(``ssa_key``) against a restated loop (tests/ssa_ref.py: the step, then divide_split over
the division the colony made), and everything else against the same colony built without
``stochastic=``, bit for bit.

The whole-colony case: 24 agents on 16 x 16 bins, GrowthProtein at rate 0.05 (a division
every 14 s), the reference's complexation network (tests/golden/flagella_complexation.json)
from monomer counts drawn in 0..300 per agent, 30 steps of 1 s.  The seed was chosen on the
CPU so that no agent's time margin falls below 1e-9 (asserted on the restatement alone)."""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import ssa_ref as sref

pytestmark = pytest.mark.gpu

N, BINS, BOUNDS, STEPS, CAP = 24, (16, 16), (32.0, 32.0), 30, 128
SEED = 20261020


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lens_amd import native
    native.load()
    return torch.device('cuda', 0)


def _model(seed=SEED, initial=0):
    return sref.fixture_model(initial, seed=seed)


def _start_counts(model, n):
    return np.random.default_rng(SEED + 5).integers(0, 301, (model.n_species, n)).astype(np.int32)


def _lattice(dev, molecules=('glc__D_e', 'lcts_e')):
    from lens_amd import configs
    from lens_amd.lattice import Lattice
    start = {'glc__D_e': configs.gaussian_bump_field(BINS), 'lcts_e': np.full(BINS, 10.0)}
    if 'MeAsp' in molecules:
        x = np.linspace(0.0, 1.0, BINS[0])
        start['MeAsp'] = 0.2 * x[:, None] + 0.05 * x[None, :] ** 2
    return Lattice(list(molecules), BINS, BOUNDS, 10.0, 5.0, device=dev, initial=start)


def _colony(dev, stochastic, capacity=CAP, cells=True, environment='lattice', n=N, **extra):
    from lens_amd import configs
    from lens_amd.cells import CellModel
    from lens_amd.colony import Colony
    env = _lattice(dev) if environment == 'lattice' else environment
    cm = CellModel(rng='philox', growth_rate=0.05, seed=SEED + 1) if cells else None
    col = Colony(configs.glc_lct_config(), n, capacity=capacity, device=dev, integrator='dopri5', environment=env,
                 cells=cm, agent_ids=['c%d.' % i for i in range(n)] if cells else None, stochastic=stochastic, **extra)
    if env not in ('held', 'nonspatial'):
        loc = np.random.default_rng(SEED).uniform(0.0, BOUNDS[0], (2, n))
        col.set_agents(location=loc)
        col.gather_external()
    if stochastic is not None:
        col.ssa[:, :n] = torch.from_numpy(_start_counts(stochastic, n)).to(dev)
    return col


def _same(a, b, names, where):
    assert a.n == b.n, where
    for name in names:
        ta, tb = getattr(a, name), getattr(b, name)
        assert torch.equal(ta[..., :a.n], tb[..., :b.n]), (where, name)


def _plan(before, after):
    """(src, kind, n_keep) of the division that took the ids ``before`` to ``after``."""
    index = {v: k for k, v in enumerate(before)}
    src, kind = [], []
    for v in after:
        if v in index:
            src.append(index[v])
            kind.append(-1)
        else:
            src.append(index[v[:-1]])
            kind.append(int(v[-1]))
    n_keep = kind.count(-1)
    assert all(k == -1 for k in kind[:n_keep]) and kind[n_keep:] == [0, 1] * ((len(kind) - n_keep) // 2)
    return src, kind, n_keep


@pytest.fixture(scope='module')
def trajectory(dev):
    """The colony with stochastic=, its twin without, and the restated ssa / ssa_key, compared
    at every step."""
    model = _model()
    a, b = _colony(dev, model), _colony(dev, None)
    x = _start_counts(model, N)
    keys = np.arange(N, dtype=np.int64)
    key_base, status = N, np.zeros(N, dtype=np.int32)
    plain = b.agent_array_names()
    assert a.agent_array_names() == plain + ['ssa', 'ssa_key']
    divisions, fired, left_out = [], [], 0
    for step in range(STEPS):
        ids = b.agent_ids()
        a.step(1.0)
        b.step(1.0)
        torch.cuda.synchronize()
        events, status, margin = sref.step(model, x, keys, 1.0, model.seed, step, status=status)
        left_out += int((margin < sref.MARGIN).sum())
        assert left_out == 0, step                          # nobody is left out with this seed
        assert np.array_equal(a.ssa_events[:len(events)].cpu().numpy(), events) or a.n != len(events), step
        after = b.agent_ids()
        if after != ids:
            src, kind, n_keep = _plan(ids, after)
            x, keys = sref.divide_counts(x, keys, src, kind, n_keep, model.seed, step, key_base)
            key_base += len(src) - n_keep
            status = np.zeros(len(src), dtype=np.int32)
            divisions.append(step)
        fired.append(int(events.sum()))
        _same(a, b, plain + ['bin_lin', 'bin_ix'], step)    # every pre-existing array, bit for bit
        assert a.agent_ids() == after, step
        assert np.array_equal(a.ssa[:, :a.n].cpu().numpy(), x), step
        assert np.array_equal(a.ssa_key[:a.n].cpu().numpy(), keys), step
    a.check_status()
    b.check_status()
    return a, b, x, keys, divisions, fired, key_base


def test_colony_equals_the_restated_loop(trajectory):
    a, b, x, keys, divisions, fired, key_base = trajectory
    assert len(divisions) >= 1 and a.n >= 2 * N
    assert fired[0] > 50 * N and sum(1 for f in fired if f) >= 3        # a burst, then the slow tail
    assert a._ssa_key_base == key_base and len(set(keys.tolist())) == a.n
    assert int(a._ssa.step_counter.item()) == STEPS
    snap = a.snapshot()
    assert np.array_equal(snap['stochastic']['flagella'], x[a.stochastic.index('flagella')])
    assert np.array_equal(snap['ssa_key'], keys)
    assert a.ssa.dtype == torch.int32 and a.ssa_key.dtype == torch.int64 and a.ssa_events.shape == (a.ld,)


def test_capacity_scratch_is_complete(trajectory):
    from lens_amd.colony import CAPACITY_SCRATCH
    a = trajectory[0]
    sized = {name for name, t in vars(a).items() if torch.is_tensor(t) and t.dim() and t.shape[-1] == a.ld}
    assert sized - set(a.agent_array_names()) - set(CAPACITY_SCRATCH) == set()
    assert {'ssa', 'ssa_key', 'ssa_events', '_ssa_status'} <= sized


def test_capacity_growth_keeps_counts_with_their_agents(dev, trajectory):
    roomy = trajectory[0]
    tight = _colony(dev, _model(), capacity=N)
    for step in range(STEPS):
        tight.step(1.0)
    torch.cuda.synchronize()
    assert tight.ld > N and tight.ld != roomy.ld
    _same(tight, roomy, tight.agent_array_names(), 'capacity growth')
    for name in tight.agent_array_names() + ['ssa_events', '_ssa_status']:
        assert getattr(tight, name).shape[-1] == tight.ld, name
    assert tight._ssa_key_base == roomy._ssa_key_base


def test_remove_keeps_counts_and_keys(dev):
    a = _colony(dev, _model(), cells=False)
    a.step(1.0)
    n = a.n
    mask = torch.zeros(n, dtype=torch.int32, device=dev)
    mask[::3] = 1
    keep = torch.nonzero(mask == 0).flatten()
    want_x, want_k = a.ssa[:, keep].clone(), a.ssa_key[keep].clone()
    assert a.remove(mask) == (n + 2) // 3 and a.n == len(keep)
    assert torch.equal(a.ssa[:, :a.n], want_x) and torch.equal(a.ssa_key[:a.n], want_k)
    assert a.ssa.shape[-1] == a.ld and a.ssa_key.dtype == torch.int64
    # the survivors draw by their own keys: the next step equals the restatement's
    model = a.stochastic
    x, keys = want_x.cpu().numpy().copy(), want_k.cpu().numpy()
    a.step(1.0)
    events, status, margin = sref.step(model, x, keys, 1.0, model.seed, 1)
    assert (margin >= sref.MARGIN).all()
    assert np.array_equal(a.ssa[:, :a.n].cpu().numpy(), x)
    assert np.array_equal(a.ssa_events[:a.n].cpu().numpy(), events)
    a.check_status()


@pytest.mark.parametrize('environment', ['held', 'nonspatial', 'lattice'])
def test_pre_existing_arrays_are_untouched(dev, environment):
    a = _colony(dev, _model(), cells=False, environment=environment)
    b = _colony(dev, None, cells=False, environment=environment)
    for step in range(3):
        a.step(1.0)
        b.step(1.0)
    torch.cuda.synchronize()
    names = b.agent_array_names()
    assert a.agent_array_names() == names + ['ssa', 'ssa_key']
    _same(a, b, names, environment)
    if environment == 'lattice':
        assert torch.equal(a.lattice.fields, b.lattice.fields)
    assert int(a.ssa_events[:a.n].sum()) >= 0 and int(a._ssa.step_counter.item()) == 3
    a.check_status()


def test_graph_replay_equals_eager_steps(dev):
    a = _colony(dev, _model(), cells=False)
    b = _colony(dev, _model(), cells=False)
    replay = b.capture(1.0, 2)
    seen = []
    for k in range(3):
        a.step(1.0)
        a.step(1.0)
        replay()
        torch.cuda.synchronize()
        _same(a, b, a.agent_array_names() + ['ssa_events', '_ssa_status'], k)
        seen.append(a.ssa[:, :a.n].clone())
    assert int(b._ssa.step_counter.item()) == 6 == int(a._ssa.step_counter.item())
    assert not torch.equal(seen[0], seen[1])             # the later replays fired events of their own
    b.check_status()


def test_status_bits_reach_check_status(dev):
    a = _colony(dev, sref.fixture_model(seed=1, max_events=10), cells=False)
    a.ssa.zero_()                                        # only agent 3 has anything to fire
    a.ssa[:, 3] = 1000
    a.step(1.0)
    assert a.ssa_events[:a.n].tolist() == [10 if k == 3 else 0 for k in range(a.n)]
    with pytest.raises(FloatingPointError, match='agent 3: stochastic step status 1'):
        a.check_status()
    mask = torch.zeros(a.n, dtype=torch.int32, device=dev)
    mask[0] = 1
    with pytest.raises(FloatingPointError, match='agent 3'):
        a.remove(mask)                                   # read before the columns move


def _motile(dev, stochastic, flagella, cells=False):
    from lens_amd import configs
    from lens_amd.cells import CellModel
    from lens_amd.colony import Colony
    from lens_amd.motility import MotilityModel
    model = MotilityModel(ligand_id='MeAsp', initial_ligand=1e-2, substeps=10, seed=SEED, flagella=flagella,
                          division='merged' if cells else None)
    lat = _lattice(dev, ('glc__D_e', 'lcts_e', 'MeAsp'))
    cm = CellModel(rng='philox', growth_rate=0.05, seed=SEED + 1) if cells else None
    col = Colony(configs.glc_lct_config(), N, capacity=CAP, device=dev, integrator='dopri5', environment=lat,
                 motility=model, stochastic=stochastic, cells=cm)
    col.set_agents(location=np.random.default_rng(SEED).uniform(0.0, BOUNDS[0], (2, N)))
    col.gather_external()
    return col


def test_flagella_from_the_complex(dev):
    """The motor's target is the count the stochastic step left; the motor reads it in the
    next step (have := target inside the motor's update), so ``have`` is one step behind."""
    from lens_amd import native
    from lens_amd.motility import FlagellaModel
    T, H = native.VK_FLAGI_TARGET, native.VK_FLAGI_HAVE
    model = sref.fixture_model(seed=SEED)
    row = model.index('flagella')
    model.initial[row] = 2                               # every agent starts with two assembled
    col = _motile(dev, model, FlagellaModel(0, complexes='flagella'))
    n = col.n
    assert col.flag_int[T, :n].tolist() == [2] * n and col.flag_int[H, :n].tolist() == [0] * n      # once at t = 0
    # monomers for 0..5 more flagella per agent, all assembled within the first step
    extra = torch.arange(n, dtype=torch.int32, device=dev) % 6
    for name in sref.load_fixture()['monomer_ids']:
        col.ssa[model.index(name), :n] = 1000
    # a hook takes 120 flgE; the 60 to spare keep the last hook fast (C(120, 120) = 1 would
    # leave it at 1e-4 per second) and cannot react themselves
    col.ssa[model.index('flgE'), :n] = 120 * extra + 60
    previous = col.flag_int[T, :n].clone()
    counts = []
    for step in range(3):
        col.step(1.0)
        torch.cuda.synchronize()
        assert torch.equal(col.flag_int[H, :n], previous), step          # what the motor read
        assert torch.equal(col.flag_int[T, :n], col.ssa[row, :n]), step  # what the next step's motor reads
        previous = col.flag_int[T, :n].clone()
        counts.append(previous.tolist())
    assert counts[0] == (2 + extra).tolist() and counts[2] == counts[0]
    col.check_status()
    with pytest.raises(ValueError, match='complexes'):
        col.set_flagella(3)
    # a 33rd flagellum: the kernel clamps, the colony raises where it reads anyway
    col.ssa[row, 5] = 33
    col.step(1.0)
    assert int(col.flag_int[T, 5]) == 32
    with pytest.raises(FloatingPointError, match='flagella'):
        col.check_status()


def test_flagella_from_the_complex_through_a_division(dev):
    """Daughters' motors read their own share of the complex."""
    from lens_amd import native
    from lens_amd.motility import FlagellaModel
    model = sref.fixture_model(seed=SEED)
    row = model.index('flagella')
    model.initial[row] = 9
    col = _motile(dev, model, FlagellaModel(0, complexes='flagella'), cells=True)
    for step in range(16):
        col.step(1.0)
    torch.cuda.synchronize()
    assert col.n == 2 * N
    t = col.flag_int[native.VK_FLAGI_TARGET, :col.n]
    assert torch.equal(t, col.ssa[row, :col.n]) and sorted(set(t.tolist())) == [4, 5]
    d = col.ssa[row, :2 * N].reshape(N, 2)               # every agent divided: the daughters in mother order
    assert d.sum(dim=1).tolist() == [9] * N
    col.check_status()


def test_rejected_combinations(dev, monkeypatch):
    """Every refusal comes before a buffer is allocated: torch.zeros / torch.from_numpy are
    never reached."""
    from lens_amd import configs
    from lens_amd.colony import Colony
    from lens_amd.distributed import AgentRouter
    from lens_amd.lattice import Lattice
    from lens_amd.motility import FlagellaModel, MotilityModel
    from lens_amd.response import ANTIBIOTICS_DEFAULTS, CellResponse
    model = _model()
    cfg = configs.glc_lct_config()
    band = Lattice(['glc__D_e', 'lcts_e'], BINS, BOUNDS, 10.0, 5.0, device=dev, row_band=(0, 8), halo=1)
    whole = _lattice(dev, ('glc__D_e', 'lcts_e', 'MeAsp'))
    motile = lambda fm: MotilityModel(ligand_id='MeAsp', initial_ligand=1e-2, seed=1, flagella=fm)
    response = CellResponse(expression=ANTIBIOTICS_DEFAULTS['ode_expression'])

    def refuse(*args, **kw):
        raise AssertionError('a buffer was allocated before the refusal')

    cases = [dict(environment='held', stochastic='not a model'),
             dict(environment=whole, motility=motile(FlagellaModel(0, complexes='flagella'))),      # no stochastic=
             dict(environment=whole, motility=motile(FlagellaModel(0, complexes='no such')), stochastic=model),
             dict(environment=band, stochastic=model),
             dict(environment='nonspatial', stochastic=model, response=response)]
    for kw in cases:
        with monkeypatch.context() as mp:
            mp.setattr(torch, 'zeros', refuse)
            mp.setattr(torch, 'full', refuse)
            with pytest.raises(ValueError):
                Colony(cfg, 4, device=dev, **kw)
    with pytest.raises(ValueError, match='not both'):
        FlagellaModel(0, expression=configs.flagella_expression(), complexes='flagella')
    with pytest.raises(ValueError):
        FlagellaModel(0, complexes=3)
    col = _colony(dev, model, cells=True)
    with pytest.raises(ValueError, match='stochastic'):
        AgentRouter(col, 0, 1, agent_offset=0)
    with pytest.raises(ValueError, match='stochastic'):
        _colony(dev, model, cells=False, environment='held').step_many(1.0, 2)
    with pytest.raises(ValueError, match='stochastic'):
        _colony(dev, model, cells=False).run(1.0)
