"""Colony(stochastic=..., translation=TranslationModel(...)): the ribosome lists, the monomer
pools and the ``ssa`` counts against a restated loop (tests/translation_ref.py: the
translation step; tests/ssa_ref.py: the network's step after it, on the counts translation
left; then both dividers over the division the colony made), and everything else against the
same colony built without ``translation=``, bit for bit.

The whole-colony case: 24 agents on 16 x 16 bins, GrowthProtein at rate 0.05 (a division every
14 s), the small model of tests/translation_ref.py (3 templates on 2 operons, 4 monomers,
rate 4, occlusion 2) over the table {o1, o2, pX, pY, pW, pZ, Ribosome, C1} with pX + pZ -> C1,
30 steps of 1 s.  That no agent's margin falls below 1e-9 is asserted on the restatement."""

import copy

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import ssa_ref as sref
import translation_ref as tref
from test_ssa_colony_gpu import BINS, BOUNDS, CAP, N, STEPS, _lattice, _plan, _same

pytestmark = pytest.mark.gpu

SEED = 20261021
X = tref.SPECIES.index
TL_NAMES = ['ribosome_slots', 'ribosome_count', 'tl_molecules']


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lens_amd import native
    native.load()
    return torch.device('cuda', 0)


def _models(rate=0.05, **kw):
    return tref.small_stochastic(seed=SEED + 2, rate=rate), tref.small_model(max_ribosomes=16, seed=SEED + 3, **kw)


def _start(n, transcripts=True):
    """(ssa counts [8, n], molecules [6, n]): 0..3 transcripts per operon, 3..6 free ribosomes,
    pools that run short of Val for some agents."""
    rng = np.random.default_rng(SEED + 5)
    x = np.zeros((len(tref.SPECIES), n), dtype=np.int32)
    x[X('o1')], x[X('o2')] = rng.integers(0, 4, n), rng.integers(0, 4, n)
    if not transcripts:
        x[X('o1')], x[X('o2')] = 0, 0
    x[X('Ribosome')] = rng.integers(3, 7, n)
    x[X('pX')], x[X('pZ')] = rng.integers(0, 3, n), rng.integers(0, 3, n)
    mol = rng.integers(40, 400, (6, n)).astype(np.int32)
    mol[3] = rng.integers(0, 60, n)
    mol[4], mol[5] = 5000, 0
    return x, mol


def _colony(dev, sm, tm, capacity=CAP, cells=True, environment='lattice', n=N, transcripts=True, motility=None):
    from lens_amd import configs
    from lens_amd.cells import CellModel
    from lens_amd.colony import Colony
    molecules = ('glc__D_e', 'lcts_e', 'MeAsp') if motility is not None else ('glc__D_e', 'lcts_e')
    env = _lattice(dev, molecules) if environment == 'lattice' else environment
    cm = CellModel(rng='philox', growth_rate=0.05, seed=SEED + 1) if cells else None
    extra = {} if tm is None else {'translation': tm}
    col = Colony(configs.glc_lct_config(), n, capacity=capacity, device=dev, integrator='dopri5', environment=env,
                 cells=cm, agent_ids=['c%d.' % i for i in range(n)] if cells else None, stochastic=sm,
                 motility=motility, **extra)
    if env not in ('held', 'nonspatial'):
        col.set_agents(location=np.random.default_rng(SEED).uniform(0.0, BOUNDS[0], (2, n)))
        col.gather_external()
    x, mol = _start(n, transcripts)
    col.ssa[:, :n] = torch.from_numpy(x).to(dev)
    if tm is not None:
        col.set_translation_molecules(**{name: mol[row] for row, name in enumerate(tm.molecule_ids)})
    return col


@pytest.fixture(scope='module')
def trajectory(dev):
    """The colony and the restated loop, compared at every step."""
    from lens_amd import native
    sm, tm = _models()
    a = _colony(dev, sm, tm)
    rows = tm.bind(sm)
    x, mol = _start(N)
    lists = [[] for _ in range(N)]
    keys = np.arange(N, dtype=np.int64)
    key_base = N
    status, tl_status = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    assert a.agent_array_names()[-5:] == ['ssa', 'ssa_key'] + TL_NAMES
    assert a.ribosomes() == lists
    divisions, bound, longest = [], [], 0
    for step in range(STEPS):
        ids = a.agent_ids()
        a.step(1.0)
        torch.cuda.synchronize()
        tl_events, tl_status, margin_t, margin_q = tref.step(tm, rows, lists, mol, x, keys, 1.0, tm.seed, step,
                                                             status=tl_status)
        events, status, margin = sref.step(sm, x, keys, 1.0, sm.seed, step, status=status)
        assert margin_t.min() >= tref.MARGIN and margin_q.min() >= tref.MARGIN and (margin >= sref.MARGIN).all(), step
        assert not tl_status.any() and not status.any(), step
        longest = max(longest, max(len(l) for l in lists))
        after = a.agent_ids()
        if after != ids:
            src, kind, n_keep = _plan(ids, after)
            lists = tref.divide_ribosomes(lists, keys, src, kind, tm.seed, step)
            mol, _ = sref.divide_counts(mol, keys, src, kind, n_keep, tm.seed ^ native.VK_TL_DIVIDE_DOMAIN, step,
                                        key_base)
            x, keys = sref.divide_counts(x, keys, src, kind, n_keep, sm.seed, step, key_base)
            key_base += len(src) - n_keep
            status, tl_status = np.zeros(len(src), dtype=np.int32), np.zeros(len(src), dtype=np.int32)
            divisions.append(step)
        else:
            assert np.array_equal(a.tl_events[:a.n].cpu().numpy(), tl_events), step
        bound.append(int(tl_events.sum()))
        assert a.ribosomes() == [[tuple(r) for r in l] for l in lists], step
        assert np.array_equal(a.tl_molecules[:, :a.n].cpu().numpy(), mol), step
        assert np.array_equal(a.ssa[:, :a.n].cpu().numpy(), x), step
        assert np.array_equal(a.ssa_key[:a.n].cpu().numpy(), keys), step
    a.check_status()
    return a, lists, mol, x, keys, divisions, bound, longest


def test_colony_equals_the_restated_loop(trajectory):
    a, lists, mol, x, keys, divisions, bound, longest = trajectory
    assert len(divisions) >= 1 and a.n >= 2 * N
    assert sum(bound) > 5 * N and 2 <= longest <= 16
    assert x[X('pX')].sum() + x[X('pY')].sum() + x[X('pZ')].sum() + x[X('C1')].sum() > N      # proteins were made
    assert int(a._ssa.step_counter.item()) == STEPS            # one step word for both launches
    snap = a.snapshot()
    assert np.array_equal(snap['translation_molecules']['ATP'], mol[4])
    assert np.array_equal(snap['ribosome_count'], [len(l) for l in lists])
    assert a.ribosome_slots.dtype == torch.int32 and a.ribosome_slots.shape == (16, a.ld)


def test_capacity_scratch_is_complete(trajectory):
    from lens_amd.colony import CAPACITY_SCRATCH
    a = trajectory[0]
    sized = {name for name, t in vars(a).items() if torch.is_tensor(t) and t.dim() and t.shape[-1] == a.ld}
    assert sized - set(a.agent_array_names()) - set(CAPACITY_SCRATCH) == set()
    assert set(TL_NAMES) | {'tl_events', '_tl_status'} <= sized


def test_capacity_growth_keeps_lists_with_their_agents(dev, trajectory):
    roomy = trajectory[0]
    tight = _colony(dev, *_models(), capacity=N)
    for step in range(STEPS):
        tight.step(1.0)
    torch.cuda.synchronize()
    assert tight.ld > N and tight.ld != roomy.ld
    assert tight.ribosomes() == roomy.ribosomes()
    _same(tight, roomy, [name for name in tight.agent_array_names() if name != 'ribosome_slots'], 'capacity growth')
    for name in tight.agent_array_names() + ['tl_events', '_tl_status']:
        assert getattr(tight, name).shape[-1] == tight.ld, name


def test_all_transcripts_at_zero_changes_nothing(dev):
    """Nothing binds and nothing elongates: every pre-existing array, ssa included, is the one
    of the colony without translation=, through a division too."""
    sm, tm = _models()
    a, b = _colony(dev, sm, tm, transcripts=False), _colony(dev, tref.small_stochastic(seed=SEED + 2), None,
                                                            transcripts=False)
    names = b.agent_array_names()
    assert a.agent_array_names() == names + TL_NAMES
    for step in range(16):
        a.step(1.0)
        b.step(1.0)
        torch.cuda.synchronize()
        _same(a, b, names + ['bin_lin', 'bin_ix', 'ssa_events'], step)
    assert a.n == 2 * N and torch.equal(a.lattice.fields, b.lattice.fields)
    assert int(a.tl_events[:a.n].sum()) == 0 and int(a.ribosome_count[:a.n].sum()) == 0
    a.check_status()


def test_remove_keeps_lists_and_pools(dev):
    sm, tm = _models()
    a = _colony(dev, sm, tm, cells=False)
    for _ in range(2):
        a.step(1.0)
    n = a.n
    mask = torch.zeros(n, dtype=torch.int32, device=dev)
    mask[::3] = 1
    keep = torch.nonzero(mask == 0).flatten().tolist()
    lists, mol, x, keys = a.ribosomes(), a.tl_molecules[:, keep].clone(), a.ssa[:, keep].clone(), a.ssa_key[keep].clone()
    assert sum(map(len, lists)) > 0
    assert a.remove(mask) == (n + 2) // 3 and a.n == len(keep)
    assert a.ribosomes() == [lists[k] for k in keep] and torch.equal(a.tl_molecules[:, :a.n], mol)
    assert torch.equal(a.ssa[:, :a.n], x) and torch.equal(a.ssa_key[:a.n], keys)
    # the survivors go on by their own keys: the next step equals the restatement's
    want = [[list(r) for r in lists[k]] for k in keep]
    mol, x, keys = mol.cpu().numpy().copy(), x.cpu().numpy().copy(), keys.cpu().numpy()
    a.step(1.0)
    tl_events, _, margin_t, margin_q = tref.step(tm, tm.bind(sm), want, mol, x, keys, 1.0, tm.seed, 2)
    events, _, margin = sref.step(sm, x, keys, 1.0, sm.seed, 2)
    assert margin_t.min() >= tref.MARGIN and margin_q.min() >= tref.MARGIN and (margin >= sref.MARGIN).all()
    assert a.ribosomes() == [[tuple(r) for r in l] for l in want]
    assert np.array_equal(a.ssa[:, :a.n].cpu().numpy(), x) and np.array_equal(a.tl_molecules[:, :a.n].cpu().numpy(), mol)
    assert np.array_equal(a.tl_events[:a.n].cpu().numpy(), tl_events)
    a.check_status()


def test_graph_replay_equals_eager_steps(dev):
    a = _colony(dev, *_models(), cells=False)
    b = _colony(dev, *_models(), cells=False)
    replay = b.capture(1.0, 2)
    seen = []
    for k in range(3):
        a.step(1.0)
        a.step(1.0)
        replay()
        torch.cuda.synchronize()
        assert a.ribosomes() == b.ribosomes(), k
        _same(a, b, [name for name in a.agent_array_names() if name != 'ribosome_slots'] +
              ['ssa_events', '_ssa_status', 'tl_events', '_tl_status'], k)
        seen.append(a.ribosomes())
    assert int(b._ssa.step_counter.item()) == 6 == int(a._ssa.step_counter.item())
    assert seen[0] != seen[1] and sum(map(len, seen[2])) > 0
    b.check_status()


def test_status_bits_reach_check_status(dev):
    sm, tm = tref.small_stochastic(), tref.small_model(max_ribosomes=2, affinities=(50.0, 50.0, 50.0))
    a = _colony(dev, sm, tm, cells=False)
    a.ssa.zero_()                                        # only agent 3 has anything to bind
    a.ssa[X('o1'), 3], a.ssa[X('Ribosome'), 3] = 5, 5
    a.step(1.0)
    assert a.tl_events[:a.n].tolist() == [2 if k == 3 else 0 for k in range(a.n)]
    with pytest.raises(FloatingPointError, match='agent 3: translation step status 1'):
        a.check_status()


def test_accessors(dev):
    sm, tm = _models()
    a = _colony(dev, sm, tm, cells=False)
    lists = [[(k % 3, 0, True), (1, 11, False)][:k % 3] for k in range(a.n)]
    a.set_ribosomes(lists)
    assert a.ribosomes() == lists
    with pytest.raises(ValueError):
        a.set_ribosomes(lists[:-1])
    with pytest.raises(ValueError):
        a.set_ribosomes([[(0, 3, True)]] * a.n)
    a.set_translation_molecules(Ala=7, ATP=np.arange(a.n))
    assert a.tl_molecules[0, :a.n].tolist() == [7] * a.n and a.tl_molecules[4, :a.n].tolist() == list(range(a.n))
    with pytest.raises(ValueError):
        a.set_translation_molecules(Unobtainium=1)
    b = _colony(dev, sm, None, cells=False)
    for call in (b.ribosomes, lambda: b.set_ribosomes([]), lambda: b.set_translation_molecules(Ala=1)):
        with pytest.raises(ValueError, match='translation'):
            call()


def test_pipeline_transcript_to_motor(dev):
    """A held transcript yields a product, a complexation reaction consumes it, and the flagella
    target follows; the motor reads it one step behind."""
    from lens_amd import native
    from lens_amd.motility import FlagellaModel, MotilityModel
    T, H = native.VK_FLAGI_TARGET, native.VK_FLAGI_HAVE
    sm, tm = _models(rate=50.0, affinities=(2.0, 0.0, 2.0))
    motility = MotilityModel(ligand_id='MeAsp', initial_ligand=1e-2, substeps=10, seed=SEED,
                             flagella=FlagellaModel(0, complexes='C1'))
    col = _colony(dev, sm, tm, cells=False, motility=motility)
    n = col.n
    col.ssa.zero_()
    col.ssa[X('o1'), :n], col.ssa[X('o2'), :n], col.ssa[X('Ribosome'), :n] = 2, 2, 3
    col.set_translation_molecules(Ala=500, Gly=500, Ser=500, Val=500)
    previous = col.flag_int[T, :n].clone()
    assert previous.tolist() == [0] * n
    made = []
    for step in range(6):
        col.step(1.0)
        torch.cuda.synchronize()
        assert torch.equal(col.flag_int[H, :n], previous), step                     # what the motor read
        assert torch.equal(col.flag_int[T, :n], col.ssa[X('C1'), :n]), step         # what the next step's reads
        assert col.ssa[X('o1'), :n].tolist() == [2] * n                             # the transcripts are held
        previous = col.flag_int[T, :n].clone()
        made.append(int(previous.sum()))
    assert made[0] == 0 and made[-1] >= n and made == sorted(made)    # pZ takes 5 residues at 4 per second
    # every protein made is a monomer still or sits in a complex; every ribosome is free or on a transcript
    x = col.ssa[:, :n].cpu().numpy()
    assert (x[X('pX')] + x[X('C1')]).sum() > 0 and np.all(x[X('pY')] == 0)
    assert np.array_equal(x[X('Ribosome')] + col.ribosome_count[:n].cpu().numpy(), np.full(n, 3))
    col.check_status()


def test_rejected_combinations(dev, monkeypatch):
    """Every refusal comes before a buffer is allocated."""
    from lens_amd import configs
    from lens_amd.colony import Colony
    from lens_amd.distributed import AgentRouter
    from lens_amd.lattice import Lattice
    from lens_amd.response import ANTIBIOTICS_DEFAULTS, CellResponse
    from lens_amd.stochastic import StochasticModel
    sm, tm = _models()
    cfg = configs.glc_lct_config()
    band = Lattice(['glc__D_e', 'lcts_e'], BINS, BOUNDS, 10.0, 5.0, device=dev, row_band=(0, 8), halo=1)
    response = CellResponse(expression=ANTIBIOTICS_DEFAULTS['ode_expression'])

    def refuse(*args, **kw):
        raise AssertionError('a buffer was allocated before the refusal')

    cases = [dict(environment='held', translation=tm),                                   # no stochastic=
             dict(environment='held', stochastic=sm, translation='not a model'),
             dict(environment='held', translation=tm,
                  stochastic=StochasticModel(['C1', 'Ribosome'], {'r': {'C1': 1}}, {'r': 1.0})),
             dict(environment=band, stochastic=sm, translation=tm),
             dict(environment='nonspatial', stochastic=sm, translation=tm, response=response)]
    for kw in cases:
        with monkeypatch.context() as mp:
            mp.setattr(torch, 'zeros', refuse)
            mp.setattr(torch, 'full', refuse)
            with pytest.raises(ValueError):
                Colony(cfg, 4, device=dev, **kw)
    col = _colony(dev, sm, tm, cells=True)
    with pytest.raises(ValueError, match='stochastic'):
        AgentRouter(col, 0, 1, agent_offset=0)
    with pytest.raises(ValueError, match='stochastic'):
        _colony(dev, sm, tm, cells=False, environment='held').step_many(1.0, 2)
    with pytest.raises(ValueError, match='stochastic'):
        _colony(dev, sm, tm, cells=False).run(1.0)
