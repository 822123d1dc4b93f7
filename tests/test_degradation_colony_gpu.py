"""Colony(stochastic=..., transcription=..., degradation=DegradationModel(...)): the carries, the
``ssa`` counts with a passive row and the pools against a restated loop (tests/transcription_ref.py
-> tests/degradation_ref.py -> tests/ssa_ref.py -> the dividers over the division the colony
made), everything else against the same colony built without ``degradation=``, and the whole
flagella chromosome in one colony.

The toy colony is test_transcription_colony_gpu.py's: 24 agents on 16 x 16 bins, GrowthProtein at
rate 0.05 (a division every 14 s), the toy chromosome over the table {oA, oAZ, oB, oBY, tfA, tfB,
RNA Polymerase, X} with oA -> X, and one passive row, the endoRNAse; 30 steps of 1 s."""

import json
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import degradation_ref as dref
import ssa_ref as sref
import transcription_ref as xref
from test_ssa_colony_gpu import BOUNDS, CAP, N, STEPS, _lattice, _plan, _same
from test_transcription_colony_gpu import SEED, X, _start

pytestmark = pytest.mark.gpu

E_ROW = len(xref.SPECIES)                  # the passive row
KM = 1e-23


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lens_amd import native
    native.load()
    return torch.device('cuda', 0)


def _models(kcat=0.1):
    from lens_amd.degradation import DegradationModel
    from lens_amd.stochastic import StochasticModel
    sm = StochasticModel(xref.SPECIES, {'decay': {'oA': -1, 'X': 1}}, {'decay': 0.05}, seed=SEED + 2,
                         passive=['endoRNAse'])
    tm = xref.toy_model(seed=SEED + 3, max_rnaps=16)
    dm = DegradationModel.from_transcription(tm, {'endoRNAse': kcat}, {'transcripts': {'endoRNAse': {
        o: KM for o in ('oA', 'oAZ', 'oB', 'oBY')}}})
    return sm, tm, dm


def _enzymes(n, same=None):
    return np.full(n, same) if same is not None else np.random.default_rng(SEED + 7).integers(0, 41, n)


def _colony(dev, sm, tm, dm, capacity=CAP, cells=True, environment='lattice', n=N, enzymes=None):
    from lens_amd import configs
    from lens_amd.cells import CellModel
    from lens_amd.colony import Colony
    env = _lattice(dev) if environment == 'lattice' else environment
    cm = CellModel(rng='philox', growth_rate=0.05, seed=SEED + 1) if cells else None
    extra = {} if dm is None else {'degradation': dm}
    col = Colony(configs.glc_lct_config(), n, capacity=capacity, device=dev, integrator='dopri5', environment=env,
                 cells=cm, agent_ids=['c%d.' % i for i in range(n)] if cells else None, stochastic=sm,
                 transcription=tm, **extra)
    if env not in ('held', 'nonspatial'):
        col.set_agents(location=np.random.default_rng(SEED).uniform(0.0, BOUNDS[0], (2, n)))
        col.gather_external()
    x, mol = _start(n, col.m2c[:n].cpu().numpy())
    col.ssa[:E_ROW, :n] = torch.from_numpy(x).to(dev)
    col.ssa[E_ROW, :n] = torch.from_numpy(_enzymes(n, enzymes).astype(np.int32)).to(dev)
    col.set_transcription_molecules(**{name: mol[row] for row, name in enumerate(tm.molecule_ids)})
    return col


@pytest.fixture(scope='module')
def trajectory(dev):
    """The colony and the restated loop, compared at every step."""
    from lens_amd import native
    from lens_amd.stochastic import passive_seed
    sm, tm, dm = _models()
    a = _colony(dev, sm, tm, dm)
    assert a.agent_array_names()[-6:] == ['ssa', 'ssa_key', 'rnap_slots', 'rnap_count', 'tx_molecules', 'deg_partial']
    assert a.ssa.shape == (9, a.ld) and a.deg_partial.shape == (4, a.ld) and a.deg_partial.dtype == torch.float64
    rows, deg_rows = tm.bind(sm), dm.bind(sm, tm)
    x, mol = _start(N, a.m2c[:N].cpu().numpy())
    x = np.concatenate([x, _enzymes(N)[None].astype(np.int32)])
    partial = np.zeros((4, N))
    lists = [[] for _ in range(N)]
    keys = np.arange(N, dtype=np.int64)
    key_base = N
    status, tx_status, deg_status = (np.zeros(N, dtype=np.int32) for _ in range(3))
    divisions, lost, carried = [], 0, False
    for step in range(STEPS):
        ids = a.agent_ids()
        m2c = a.m2c[:a.n].cpu().numpy().copy()           # what the previous step left: every launch's input
        a.step(1.0)
        torch.cuda.synchronize()
        tx_events, tx_status, margins = xref.step(tm, rows, lists, mol, x, m2c, keys, 1.0, tm.seed, step,
                                                  status=tx_status)
        degraded, deg_status = dref.step(dm, deg_rows, x, partial, mol, m2c, 1.0, status=deg_status)
        events, status, margin = sref.step(sm, x[:E_ROW], keys, 1.0, sm.seed, step, status=status)
        assert margins.min() >= xref.MARGIN and (margin >= sref.MARGIN).all(), step
        assert not status.any() and not tx_status.any() and not deg_status.any(), step
        lost += int(degraded.sum())
        after = a.agent_ids()
        if after != ids:
            src, kind, n_keep = _plan(ids, after)
            lists = xref.divide_rnaps(lists, keys, src, kind, tm.seed, step)
            mol, _ = sref.divide_counts(mol, keys, src, kind, n_keep, tm.seed ^ native.VK_TX_DIVIDE_DOMAIN, step,
                                        key_base)
            passive, _ = sref.divide_counts(x[E_ROW:], keys, src, kind, n_keep, passive_seed(sm.seed, 0), step, key_base)
            active, keys = sref.divide_counts(x[:E_ROW], keys, src, kind, n_keep, sm.seed, step, key_base)
            x = np.concatenate([active, passive])
            carried = carried or bool(partial[:, [s for s, k in zip(src, kind) if k >= 0]].any())
            partial = np.where(np.asarray(kind)[None, :] < 0, partial[:, src], 0.0)      # daughters start at 0
            key_base += len(src) - n_keep
            status, tx_status, deg_status = (np.zeros(len(src), dtype=np.int32) for _ in range(3))
            divisions.append(step)
            daughters = np.nonzero(np.asarray(kind) >= 0)[0]
            assert not a.deg_partial[:, daughters].any(), step
        else:
            assert np.array_equal(a.deg_degraded[:a.n].cpu().numpy(), degraded), step
        assert a.rnaps() == [[tuple(r) for r in l] for l in lists], step
        assert np.array_equal(a.tx_molecules[:, :a.n].cpu().numpy(), mol), step
        assert np.array_equal(a.ssa[:, :a.n].cpu().numpy(), x), step
        assert np.array_equal(a.ssa_key[:a.n].cpu().numpy(), keys), step
        assert np.array_equal(a.deg_partial[:, :a.n].cpu().numpy().view(np.int64), partial.view(np.int64)), step
    a.check_status()
    return a, x, partial, divisions, lost, carried


def test_colony_equals_the_restated_loop(trajectory):
    a, x, partial, divisions, lost, carried = trajectory
    assert len(divisions) >= 1 and a.n >= 2 * N
    # the oA the agents start with (1 each on average, lost at about 0.25 / s against a decay of 0.05 / s)
    # accounts for half of N alone; and mothers held carries that their daughters do not
    assert lost >= N // 2 and carried
    assert np.all((partial >= 0) & (partial < 1)) and partial.any()
    snap = a.snapshot()
    assert snap['degraded_transcripts'].shape == (a.n,)
    assert list(snap['stochastic']) == xref.SPECIES + ['endoRNAse']
    assert np.array_equal(snap['stochastic']['endoRNAse'], x[E_ROW])


def test_capacity_scratch_is_complete(trajectory):
    from lens_amd.colony import CAPACITY_SCRATCH
    a = trajectory[0]
    sized = {name for name, t in vars(a).items() if torch.is_tensor(t) and t.dim() and t.shape[-1] == a.ld}
    assert sized - set(a.agent_array_names()) - set(CAPACITY_SCRATCH) == set()
    assert {'deg_partial', 'deg_degraded', '_deg_status'} <= sized


def test_capacity_growth_keeps_the_carries(dev, trajectory):
    roomy = trajectory[0]
    tight = _colony(dev, *_models(), capacity=N)
    for step in range(STEPS):
        tight.step(1.0)
    torch.cuda.synchronize()
    assert tight.ld > N and tight.ld != roomy.ld
    _same(tight, roomy, [name for name in tight.agent_array_names() if name != 'rnap_slots'], 'capacity growth')
    for name in tight.agent_array_names() + ['deg_degraded', '_deg_status']:
        assert getattr(tight, name).shape[-1] == tight.ld, name


def test_sort_by_bin_moves_the_carries(dev):
    a = _colony(dev, *_models(), cells=False)
    for _ in range(3):
        a.step(1.0)
    carries, x = a.deg_partial[:, :a.n].clone(), a.ssa[:, :a.n].clone()
    order = a.sort_by_bin()
    assert not torch.equal(order, torch.arange(a.n, device=dev)) and bool(carries.any())
    assert torch.equal(a.deg_partial[:, :a.n], carries[:, order]) and torch.equal(a.ssa[:, :a.n], x[:, order])


def test_equals_the_colony_without_degradation_until_the_first_loss(dev):
    """Four endoRNAses per agent: the carries take a few steps to cross 1.  Until a transcript is
    lost the launch writes nothing but ``deg_partial``, so every array the twin without
    ``degradation=`` has is hers bit for bit, through whatever divides on the way."""
    sm, tm, dm = _models()
    a, b = _colony(dev, sm, tm, dm, enzymes=4), _colony(dev, *_models()[:2], None, enzymes=4)
    names = b.agent_array_names()
    assert a.agent_array_names() == names + ['deg_partial'] and b.deg_partial is None
    first = None
    for step in range(STEPS):
        a.step(1.0)
        b.step(1.0)
        torch.cuda.synchronize()
        if int(a.deg_degraded[:a.n].sum()) > 0:
            first = step
            break
        _same(a, b, names + ['bin_lin', 'bin_ix', 'ssa_events', '_ssa_status', 'tx_events', '_tx_status'], step)
        assert bool(a.deg_partial[:, :a.n].any())
    assert first is not None and first >= 3, first
    assert not torch.equal(a.ssa[:, :a.n], b.ssa[:, :b.n])
    a.check_status()


def test_remove_keeps_the_carries(dev):
    a = _colony(dev, *_models(), cells=False)
    for _ in range(3):
        a.step(1.0)
    n = a.n
    mask = torch.zeros(n, dtype=torch.int32, device=dev)
    mask[::3] = 1
    keep = torch.nonzero(mask == 0).flatten().tolist()
    carries, x = a.deg_partial[:, keep].clone(), a.ssa[:, keep].clone()
    assert bool(carries.any())
    assert a.remove(mask) == (n + 2) // 3 and a.n == len(keep)
    assert torch.equal(a.deg_partial[:, :a.n], carries) and torch.equal(a.ssa[:, :a.n], x)


def test_graph_replay_equals_eager_steps(dev):
    """capture() works without cells: 5 replayed steps are 5 plain ones."""
    a = _colony(dev, *_models(), cells=False)
    b = _colony(dev, *_models(), cells=False)
    replay = b.capture(1.0, 1)
    for k in range(5):
        a.step(1.0)
        replay()
        torch.cuda.synchronize()
        assert a.rnaps() == b.rnaps(), k
        _same(a, b, [name for name in a.agent_array_names() if name != 'rnap_slots'] +
              ['ssa_events', '_ssa_status', 'tx_events', '_tx_status', 'deg_degraded', '_deg_status'], k)
    assert int(b._ssa.step_counter.item()) == 5 == int(a._ssa.step_counter.item())
    assert bool(a.deg_partial[:, :a.n].any()) and int((a.ssa[:4, :a.n]).sum()) > 0


def test_status_bits_reach_check_status(dev):
    a = _colony(dev, *_models(), cells=False)
    a.tx_molecules[1, 5] = 2 ** 31 - 2                   # agent 5's GTP at the edge
    a.ssa[:4, 5] = 20
    a.ssa[E_ROW, 5] = 10 ** 6
    before = a.ssa[:4, 5].clone()
    a.step(1.0)
    with pytest.raises(FloatingPointError, match='agent 5: degradation step status 2'):
        a.check_status()
    # nothing of her was written: no carry, no loss, no nucleotide returned
    assert int(a.deg_degraded[5]) == 0 and not bool(a.deg_partial[:, 5].any())
    assert int(a.tx_molecules[1, 5]) <= 2 ** 31 - 2 and bool((a.ssa[1:4, 5] >= before[1:]).all())
    assert bool(a.deg_partial[:, :a.n].any())            # her neighbours were stepped


def _golden(name):
    with open(os.path.join(dref.GOLDEN, name)) as f:
        return json.load(f)


@pytest.mark.parametrize('placed', [False, True])
def test_whole_chromosome_in_one_colony(dev, placed):
    """All 15 operons: 77 rows, 37 of them the network's.  Two steps of 1 s from
    get_flagella_initial_state.  Per nucleotide, pool + transcripts x composition + the bases in
    nascent chains stays what it was for every agent.  No operon is finished in 2 s, so ``placed``
    puts 3 of every transcript into every agent and many endoRNAses into every other one, and the
    launch degrades; the free ribosomes are then cut to 10, since 100 of them on 45 transcripts
    would fill the 16 slots of the list."""
    from lens_amd import configs
    from lens_amd.colony import Colony
    deg = dref.flagella_data()
    cfg = configs.flagella_gene_expression(_golden('flagella_transcription.json'), _golden('flagella_translation.json'),
                                           _golden('flagella_complexation.json'), deg, operons=None, max_rnaps=16,
                                           max_ribosomes=16)
    sm, tm, lm, dm = cfg['stochastic'], cfg['transcription'], cfg['translation'], cfg['degradation']
    n = 65
    col = Colony(configs.glc_lct_config(), n, device=dev, environment='held', **cfg)
    assert col.ssa.shape == (sm.n_rows, col.ld) and sm.n_rows > 64 and col.deg_partial.shape[0] == 15
    pools = deg['initial_state']['molecules']
    col.set_transcription_molecules(**{m: pools[m] for m in tm.molecule_ids if m in pools})
    col.set_translation_molecules(**{m: pools[m] for m in lm.molecule_ids if m in pools})
    trow, erow = dm.bind(sm, tm)
    assert int(col.ssa[sm.index('RNA Polymerase'), 0]) == 100 and int(col.ssa[sm.index('flagella'), 0]) == 8
    assert int(col.ssa[sm.index('Ribosome'), 0]) == 100 and int(col.ssa[int(erow[0]), 0]) == 1
    if placed:
        col.ssa[torch.from_numpy(trow).long().to(dev), :n] = 3
        col.ssa[int(erow[0]), 1:n:2] = 2000
        col.ssa[sm.index('Ribosome'), :n] = 10

    def held():
        """[3, n]: GTP, UTP, CTP in the pool, in finished transcripts and in nascent chains."""
        mol = col.tx_molecules[:, :n].cpu().numpy().astype(np.int64)
        x = col.ssa[:, :n].cpu().numpy().astype(np.int64)
        out = []
        for name in ('GTP', 'UTP', 'CTP'):
            i = tm.monomer_ids.index(name)
            total = mol[i] + (x[trow] * dm.composition[:, i][:, None]).sum(axis=0)
            for a, rnaps in enumerate(col.rnaps()):
                for template, terminator, position, occluding in rnaps:
                    total[a] += int((tm.seq[tm.seq_ptr[template]:tm.seq_ptr[template] + position] == i).sum())
            out.append(total)
        return np.asarray(out)

    start = held()
    lost = 0
    for step in range(2):
        col.step(1.0)
        torch.cuda.synchronize()
        lost += int(col.deg_degraded[:n].sum())
        assert np.array_equal(held(), start), step
    col.check_status()
    if placed:
        assert lost == 45 * (n // 2) and int(col.deg_degraded[0:n:2].sum()) == 0        # all 3 x 15, in step one
        assert not bool(col.ssa[torch.from_numpy(trow).long().to(dev), 1:n:2].any())
    else:
        assert lost == 0 and not bool(col.deg_partial.any())     # no transcript yet: levels of 0.0
    assert int(col.rnap_count[:n].sum()) > 0 and int(col.tx_events[:n].sum()) > 0      # RNAPs bound and elongate
    assert col.snapshot()['degraded_transcripts'].shape == (n,)
