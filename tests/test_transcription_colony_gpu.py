"""Colony(stochastic=..., transcription=TranscriptionModel(...)): the RNAP lists, the nucleotide
pools and the ``ssa`` counts against a restated loop (tests/transcription_ref.py: the
transcription step with the mmol_to_counts the previous step left; tests/ssa_ref.py: the
network's step after it, on the counts transcription left; then the dividers over the division
the colony made), and everything else against the same colony built without ``transcription=``,
bit for bit.

The whole-colony case: 24 agents on 16 x 16 bins, GrowthProtein at rate 0.05 (a division every
14 s), the toy chromosome over the table {oA, oAZ, oB, oBY, tfA, tfB, RNA Polymerase, X} with
oA -> X, 30 steps of 1 s.  The factor counts start at 0.2 .. 0.7 mM, so growth (mmol_to_counts
rises) and division (the counts split) carry agents across both thresholds.  That no agent's
margin falls below 1e-9 is asserted on the restatement."""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import ssa_ref as sref
import transcription_ref as xref
from test_ssa_colony_gpu import BINS, BOUNDS, CAP, N, STEPS, _lattice, _plan, _same

pytestmark = pytest.mark.gpu

SEED = 20261021
X = xref.SPECIES.index
TX_NAMES = ['rnap_slots', 'rnap_count', 'tx_molecules']


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lens_amd import native
    native.load()
    return torch.device('cuda', 0)


def _models(rate=0.05, **kw):
    kw.setdefault('max_rnaps', 16)
    return xref.toy_stochastic(seed=SEED + 2, rate=rate), xref.toy_model(seed=SEED + 3, **kw)


def _start(n, m2c):
    """(ssa counts [8, n], molecules [5, n]): factors at 0.2 .. 0.7 mM, 1..4 free RNAPs, pools that
    run short of UTP for some agents."""
    rng = np.random.default_rng(SEED + 5)
    x = np.zeros((len(xref.SPECIES), n), dtype=np.int32)
    x[X('tfA')] = np.rint(rng.uniform(0.2, 0.7, n) * m2c)
    x[X('tfB')] = np.rint(rng.uniform(0.2, 0.7, n) * m2c)
    x[X('RNA Polymerase')] = rng.integers(1, 5, n)
    x[X('oA')] = rng.integers(0, 3, n)
    mol = rng.integers(40, 400, (5, n)).astype(np.int32)
    mol[2] = rng.integers(0, 40, n)
    mol[4] = 0
    return x, mol


def _colony(dev, sm, tm, capacity=CAP, cells=True, environment='lattice', n=N, translation=None, start=True):
    from lens_amd import configs
    from lens_amd.cells import CellModel
    from lens_amd.colony import Colony
    env = _lattice(dev) if environment == 'lattice' else environment
    cm = CellModel(rng='philox', growth_rate=0.05, seed=SEED + 1) if cells else None
    extra = {} if tm is None else {'transcription': tm}
    if translation is not None:
        extra['translation'] = translation
    col = Colony(configs.glc_lct_config(), n, capacity=capacity, device=dev, integrator='dopri5', environment=env,
                 cells=cm, agent_ids=['c%d.' % i for i in range(n)] if cells else None, stochastic=sm, **extra)
    if env not in ('held', 'nonspatial'):
        col.set_agents(location=np.random.default_rng(SEED).uniform(0.0, BOUNDS[0], (2, n)))
        col.gather_external()
    if start:
        x, mol = _start(n, col.m2c[:n].cpu().numpy())
        col.ssa[:, :n] = torch.from_numpy(x).to(dev)
        if tm is not None:
            col.set_transcription_molecules(**{name: mol[row] for row, name in enumerate(tm.molecule_ids)})
    return col


@pytest.fixture(scope='module')
def trajectory(dev):
    """The colony and the restated loop, compared at every step."""
    from lens_amd import native
    sm, tm = _models()
    a = _colony(dev, sm, tm)
    rows = tm.bind(sm)
    x, mol = _start(N, a.m2c[:N].cpu().numpy())
    lists = [[] for _ in range(N)]
    keys = np.arange(N, dtype=np.int64)
    key_base = N
    status, tx_status = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    assert a.agent_array_names()[-5:] == ['ssa', 'ssa_key'] + TX_NAMES
    assert a.rnaps() == lists
    divisions, bound, longest, states = [], [], 0, set()
    for step in range(STEPS):
        ids = a.agent_ids()
        m2c = a.m2c[:a.n].cpu().numpy().copy()           # what the previous step left: the launch's input
        for k in range(a.n):
            states.add((x[X('tfA'), k] / m2c[k] >= 0.3, x[X('tfB'), k] / m2c[k] >= 0.5))
        a.step(1.0)
        torch.cuda.synchronize()
        tx_events, tx_status, margins = xref.step(tm, rows, lists, mol, x, m2c, keys, 1.0, tm.seed, step,
                                                  status=tx_status)
        events, status, margin = sref.step(sm, x, keys, 1.0, sm.seed, step, status=status)
        assert margins.min() >= xref.MARGIN and (margin >= sref.MARGIN).all(), step
        assert not status.any() and not tx_status.any(), step
        longest = max(longest, max(len(l) for l in lists))
        after = a.agent_ids()
        if after != ids:
            src, kind, n_keep = _plan(ids, after)
            lists = xref.divide_rnaps(lists, keys, src, kind, tm.seed, step)
            mol, _ = sref.divide_counts(mol, keys, src, kind, n_keep, tm.seed ^ native.VK_TX_DIVIDE_DOMAIN, step,
                                        key_base)
            x, keys = sref.divide_counts(x, keys, src, kind, n_keep, sm.seed, step, key_base)
            key_base += len(src) - n_keep
            status, tx_status = np.zeros(len(src), dtype=np.int32), np.zeros(len(src), dtype=np.int32)
            divisions.append(step)
        else:
            assert np.array_equal(a.tx_events[:a.n].cpu().numpy(), tx_events), step
        bound.append(int(tx_events.sum()))
        assert a.rnaps() == [[tuple(r) for r in l] for l in lists], step
        assert np.array_equal(a.tx_molecules[:, :a.n].cpu().numpy(), mol), step
        assert np.array_equal(a.ssa[:, :a.n].cpu().numpy(), x), step
        assert np.array_equal(a.ssa_key[:a.n].cpu().numpy(), keys), step
    a.check_status()
    return a, lists, mol, x, keys, divisions, bound, longest, states


def test_colony_equals_the_restated_loop(trajectory):
    a, lists, mol, x, keys, divisions, bound, longest, states = trajectory
    assert len(divisions) >= 1 and a.n >= 2 * N
    assert sum(bound) > 2 * N and 2 <= longest <= 16
    assert len(states) == 4                                    # every combination of bound / unbound sites was met
    assert min(x[X(s)].sum() for s in ('oAZ', 'oB', 'oBY')) > 0 and x[X('X')].sum() > 0       # transcripts, and oA decays
    assert int(a._ssa.step_counter.item()) == STEPS            # one step word for both launches
    snap = a.snapshot()
    assert np.array_equal(snap['transcription_molecules']['ADP'], mol[4])
    assert np.array_equal(snap['rnap_count'], [len(l) for l in lists])
    assert snap['transcription_events'].shape == (a.n,)
    assert a.rnap_slots.dtype == torch.int32 and a.rnap_slots.shape == (16, a.ld)


def test_capacity_scratch_is_complete(trajectory):
    from lens_amd.colony import CAPACITY_SCRATCH
    a = trajectory[0]
    sized = {name for name, t in vars(a).items() if torch.is_tensor(t) and t.dim() and t.shape[-1] == a.ld}
    assert sized - set(a.agent_array_names()) - set(CAPACITY_SCRATCH) == set()
    assert set(TX_NAMES) | {'tx_events', '_tx_status'} <= sized


def test_capacity_growth_keeps_lists_with_their_agents(dev, trajectory):
    roomy = trajectory[0]
    tight = _colony(dev, *_models(), capacity=N)
    for step in range(STEPS):
        tight.step(1.0)
    torch.cuda.synchronize()
    assert tight.ld > N and tight.ld != roomy.ld
    assert tight.rnaps() == roomy.rnaps()
    _same(tight, roomy, [name for name in tight.agent_array_names() if name != 'rnap_slots'], 'capacity growth')
    for name in tight.agent_array_names() + ['tx_events', '_tx_status']:
        assert getattr(tight, name).shape[-1] == tight.ld, name


def test_no_affinity_changes_nothing(dev):
    """Every affinity 0 and empty lists: nothing binds and nothing elongates, and every pre-existing
    array, ssa included, is the one of the colony without transcription=, through a division too."""
    sm, tm = _models(affinity=0.0)
    a, b = _colony(dev, sm, tm), _colony(dev, xref.toy_stochastic(seed=SEED + 2), None)
    names = b.agent_array_names()
    assert a.agent_array_names() == names + TX_NAMES
    for step in range(16):
        a.step(1.0)
        b.step(1.0)
        torch.cuda.synchronize()
        _same(a, b, names + ['bin_lin', 'bin_ix', 'ssa_events', '_ssa_status'], step)
    assert a.n == 2 * N and torch.equal(a.lattice.fields, b.lattice.fields)
    assert int(a.tx_events[:a.n].sum()) == 0 and int(a.rnap_count[:a.n].sum()) == 0
    assert int(a.tx_molecules[4, :a.n].sum()) == 0
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
    lists, mol, x, keys = a.rnaps(), a.tx_molecules[:, keep].clone(), a.ssa[:, keep].clone(), a.ssa_key[keep].clone()
    assert sum(map(len, lists)) > 0
    assert a.remove(mask) == (n + 2) // 3 and a.n == len(keep)
    assert a.rnaps() == [lists[k] for k in keep] and torch.equal(a.tx_molecules[:, :a.n], mol)
    assert torch.equal(a.ssa[:, :a.n], x) and torch.equal(a.ssa_key[:a.n], keys)
    # the survivors go on by their own keys: the next step equals the restatement's
    want = [[list(r) for r in lists[k]] for k in keep]
    mol, x, keys = mol.cpu().numpy().copy(), x.cpu().numpy().copy(), keys.cpu().numpy()
    m2c = a.m2c[:a.n].cpu().numpy().copy()
    a.step(1.0)
    tx_events, _, margins = xref.step(tm, tm.bind(sm), want, mol, x, m2c, keys, 1.0, tm.seed, 2)
    events, _, margin = sref.step(sm, x, keys, 1.0, sm.seed, 2)
    assert margins.min() >= xref.MARGIN and (margin >= sref.MARGIN).all()
    assert a.rnaps() == [[tuple(r) for r in l] for l in want]
    assert np.array_equal(a.ssa[:, :a.n].cpu().numpy(), x) and np.array_equal(a.tx_molecules[:, :a.n].cpu().numpy(), mol)
    assert np.array_equal(a.tx_events[:a.n].cpu().numpy(), tx_events)


def test_graph_replay_equals_eager_steps(dev):
    """capture() works without cells: the replayed steps are the plain ones."""
    a = _colony(dev, *_models(), cells=False)
    b = _colony(dev, *_models(), cells=False)
    replay = b.capture(1.0, 2)
    seen = []
    for k in range(3):
        a.step(1.0)
        a.step(1.0)
        replay()
        torch.cuda.synchronize()
        assert a.rnaps() == b.rnaps(), k
        _same(a, b, [name for name in a.agent_array_names() if name != 'rnap_slots'] +
              ['ssa_events', '_ssa_status', 'tx_events', '_tx_status'], k)
        seen.append(a.rnaps())
    assert int(b._ssa.step_counter.item()) == 6 == int(a._ssa.step_counter.item())
    assert seen[0] != seen[1] and sum(map(len, seen[2])) > 0


def test_status_bits_reach_check_status(dev):
    sm, tm = xref.toy_stochastic(), xref.toy_model(max_rnaps=1, affinity=500.0, polymerase_occlusion=0)
    a = _colony(dev, sm, tm, cells=False)
    a.ssa.zero_()                                        # only agent 3 has a free RNAP
    a.tx_molecules.zero_()                               # and nobody a nucleotide: the one bound stays
    a.ssa[X('RNA Polymerase'), 3] = 5
    a.step(1.0)
    assert a.tx_events[:a.n].tolist() == [1 if k == 3 else 0 for k in range(a.n)]
    with pytest.raises(FloatingPointError, match='agent 3: transcription step status 1'):
        a.check_status()


def test_accessors(dev):
    sm, tm = _models()
    a = _colony(dev, sm, tm, cells=False)
    lists = [[(k % 2, 0, 0, True), (1, 1, 8, False)][:k % 3] for k in range(a.n)]
    a.set_rnaps(lists)
    assert a.rnaps() == lists
    with pytest.raises(ValueError):
        a.set_rnaps(lists[:-1])
    with pytest.raises(ValueError):
        a.set_rnaps([[(0, 0, 3, True)]] * a.n)
    a.set_transcription_molecules(GTP=7, ATP=np.arange(a.n))
    assert a.tx_molecules[1, :a.n].tolist() == [7] * a.n and a.tx_molecules[0, :a.n].tolist() == list(range(a.n))
    with pytest.raises(ValueError):
        a.set_transcription_molecules(Unobtainium=1)
    b = _colony(dev, sm, None, cells=False)
    for call in (b.rnaps, lambda: b.set_rnaps([]), lambda: b.set_transcription_molecules(GTP=1)):
        with pytest.raises(ValueError, match='transcription'):
            call()


def test_pipeline_factor_to_transcript_to_product(dev):
    """The flagella fixture's fliC operon with translation=: fliA above fliCp's threshold (5e-6 mM,
    3.7 counts at this mass) opens the promoter, RNAPs transcribe its 1496 bases (30 s at 50 per
    second), ribosomes translate the transcript.  With fliA below the threshold no RNAP ever binds
    and no transcript appears."""
    import json
    import os
    from lens_amd import configs
    from lens_amd.stochastic import StochasticModel
    tx = configs.flagella_transcription(xref.flagella_data(), operons=['fliC'], max_rnaps=32)
    with open(os.path.join(xref.GOLDEN, 'flagella_translation.json')) as f:
        tl = configs.flagella_translation(json.load(f), operons=['fliC'], sequences={'fliC': 'MAQVINTNSLSLLTQNNLNK'},
                                          max_ribosomes=32)
    species = ['fliC_RNA', 'fliC', 'fliA', 'RNA Polymerase', 'Ribosome', 'spent']
    sm = StochasticModel(species, {'decay': {'fliC': -1, 'spent': 1}}, {'decay': 1e-4}, seed=SEED)
    assert tx.promoter_order == ['fliCp'] and tx.length(0) == 1496 and tx.species() == ['fliC_RNA', 'fliA',
                                                                                         'RNA Polymerase']
    n = 8
    col = _colony(dev, sm, tx, cells=False, environment='held', n=n, capacity=n, translation=tl, start=False)
    assert col.agent_array_names()[-8:-3] == ['ssa', 'ssa_key', 'ribosome_slots', 'ribosome_count', 'tl_molecules']
    threshold = 5e-06 * float(col.m2c[0])
    assert 3 < threshold < 4
    fliA = np.array([10, 1, 4, 3, 0, 50, 2, 7])
    on = fliA >= threshold
    col.ssa[species.index('fliA'), :n] = torch.from_numpy(fliA.astype(np.int32)).to(dev)
    col.ssa[species.index('RNA Polymerase'), :n] = 4
    col.ssa[species.index('Ribosome'), :n] = 4
    col.set_transcription_molecules(ATP=10 ** 6, GTP=10 ** 6, UTP=10 ** 6, CTP=10 ** 6)
    col.set_translation_molecules(ATP=10 ** 6, **{name: 10 ** 5 for name in tl.monomer_ids})
    first = None
    for step in range(6):
        col.step(10.0)                                   # the reference's compartment step: 500 sub-intervals
        torch.cuda.synchronize()
        if step == 1:
            first = col.ssa[species.index('fliC_RNA'), :n].cpu().numpy().copy()
    col.check_status()
    x = col.ssa[:, :n].cpu().numpy()
    rna, protein = x[species.index('fliC_RNA')], x[species.index('fliC')] + x[species.index('spent')]
    assert np.all(first == 0)                                     # 20 s are too short for 1496 bases
    assert np.all(rna[on] > 0) and np.all(protein[on] > 0)
    assert np.all(rna[~on] == 0) and np.all(protein[~on] == 0)
    assert np.all(col.rnap_count[:n].cpu().numpy()[~on] == 0) and np.all(x[species.index('RNA Polymerase')][~on] == 4)
    assert np.array_equal(x[species.index('RNA Polymerase')] + col.rnap_count[:n].cpu().numpy(), np.full(n, 4))
    # the books: ATP pays one per base whatever the base, ADP gains as many
    mol = col.tx_molecules[:, :n].cpu().numpy().astype(np.int64)
    assert np.array_equal(mol[4], 10 ** 6 - mol[0]) and np.all(mol[4][on] > 1496) and np.all(mol[4][~on] == 0)


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

    cases = [dict(environment='held', transcription=tm),                                 # no stochastic=
             dict(environment='held', stochastic=sm, transcription='not a model'),
             dict(environment='held', transcription=tm,
                  stochastic=StochasticModel(['X', 'RNA Polymerase'], {'r': {'X': 1}}, {'r': 1.0})),
             dict(environment=band, stochastic=sm, transcription=tm),
             dict(environment='nonspatial', stochastic=sm, transcription=tm, response=response)]
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
