"""The RNA degradation step on the device (vk_rna_degradation_step) against the restatement
tests/degradation_ref.py, and passive rows of the count table under vk_ssa_step and the divider.

Every comparison is bitwise: counts, partials (FP64), pools, ``degraded`` and status.  Both sides do
the same IEEE operations in the same order (int -> double, divide, multiply, add, trunc, subtract;
the build does not contract), so nothing is left to a tolerance and no agent is left out.

Shapes: n in {1, 63, 64, 65, 257} with ld = n + 7 (one lane, a wave less one, a wave, a wave and
one, more than one block of 256); columns n..ld-1 hold a sentinel in every array and are compared
with the rest.  Models of 4, 16, 17 and 64 transcripts: at most 16 are held in registers between
the decision and the stores, more run the chunks twice."""

import ctypes
import types

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import degradation_ref as dref
import ssa_ref as sref

pytestmark = pytest.mark.gpu

SEED = 20261022
KM = 1e-23


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lens_amd import native
    native.load()
    return torch.device('cuda', 0)


def _table(model, extra=('other',), passive=False):
    """A StochasticModel whose rows hold the model's species between rows of its own; ``passive``:
    the transcripts are passive rows."""
    from lens_amd.stochastic import StochasticModel
    front = ['x0'] + list(model.enzyme_order) + list(extra)
    if passive:
        return StochasticModel(front, {'r': {'x0': 1}}, {'r': 1.0}, passive=model.transcript_names()[::-1])
    return StochasticModel(front + model.transcript_names()[::-1], {'r': {'x0': 1}}, {'r': 1.0})


def _engine(dev, model, sm):
    from lens_amd.degradation import DegradationEngine
    return DegradationEngine(model, sm, dref.Pools(model.molecule_ids), dev)


def _put(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _run(dev, model, sm, counts, partial, molecules, m2c, n, timestep, steps):
    """``steps`` launches and as many restated steps, compared after each, whole arrays (sentinel
    columns included).  Returns the last (counts, partial, molecules, degraded, status)."""
    eng = _engine(dev, model, sm)
    rows = dref.bind(model, sm.rows)
    assert [r.tolist() for r in rows] == [r.tolist() for r in model.bind(sm, dref.Pools(model.molecule_ids))]
    ld = counts.shape[1]
    x, p, mol, m = _put(dev, counts, partial, molecules, m2c)
    degraded = torch.full((ld,), -7, dtype=torch.int32, device=dev)
    status = torch.zeros(ld, dtype=torch.int32, device=dev)
    want_x, want_p, want_mol = counts.copy(), partial.copy(), molecules.copy()
    want_status = np.zeros(n, dtype=np.int32)
    for k in range(steps):
        eng.step(timestep, x, p, mol, m, n, degraded=degraded, status=status)
        want_degraded, want_status = dref.step(model, rows, want_x, want_p, want_mol, m2c, timestep, n, want_status)
        got = [t.cpu().numpy() for t in (x, p, mol, degraded, status)]
        assert np.array_equal(got[0], want_x), k
        assert np.array_equal(got[1].view(np.int64), want_p.view(np.int64)), k           # FP64, bit for bit
        assert np.array_equal(got[2], want_mol), k
        assert np.array_equal(got[3][:n], want_degraded) and np.all(got[3][n:] == -7), k
        assert np.array_equal(got[4][:n], want_status) and np.all(got[4][n:] == 0), k
    return want_x, want_p, want_mol, want_degraded, want_status


@pytest.mark.parametrize('passive', [False, True])
@pytest.mark.parametrize('n', dref.SIZES)
def test_toy_over_thirty_launches(dev, n, passive):
    """The reference's toy, enzyme counts 0..40 and mmol_to_counts 5..40 per agent: the carry crosses
    1 on different steps for different agents."""
    model = dref.toy_model()
    sm = _table(model, passive=passive)
    counts, partial, molecules, m2c = dref.case(model, sm.rows, n, SEED)
    x, p, mol, degraded, status = _run(dev, model, sm, counts, partial, molecules, m2c, n, 1.0, 30)
    assert not status.any()
    if n >= 63:
        trow = dref.bind(model, sm.rows)[0]
        lost = (counts[trow, :n] - x[trow, :n]).sum(axis=0)
        assert len(set(lost.tolist())) > 3 and lost.max() > 0      # agents lose at different rates
        assert np.all((p[:, :n] >= 0) & (p[:, :n] < 1)) and len(np.unique(p[:, :n])) > n
        others = [r for r in range(sm.n_rows) if r not in trow]
        assert np.array_equal(x[others], counts[others])           # no other row is written


@pytest.mark.parametrize('n', dref.SIZES)
def test_two_enzymes_on_one_transcript_and_one_without_a_pair(dev, n):
    from lens_amd.degradation import DegradationModel
    model = DegradationModel({'a': 'GACUUG', 'b': 'CCC', 'c': 'AUAUAUAU'}, {'slow': 0.01, 'fast': 0.3},
                             {'transcripts': {'fast': {'a': 3e-23, 'c': 1e-22}, 'slow': {'a': KM}}})
    assert np.diff(model.pair_ptr).tolist() == [2, 0, 1] and model.pair_enzyme.tolist() == [0, 1, 1]
    sm = _table(model)
    counts, partial, molecules, m2c = dref.case(model, sm.rows, n, SEED + 1, m2c=(1e-4, 2e-4))
    x, p, mol, degraded, status = _run(dev, model, sm, counts, partial, molecules, m2c, n, 0.7, 6)
    b = sm.index('b')
    assert np.array_equal(x[b], counts[b]) and not p[1, :n].any() and not status.any()
    if n >= 63:
        assert degraded.sum() > 0


@pytest.mark.parametrize('n', dref.SIZES)
def test_counts_of_zero(dev, n):
    """Transcripts and enzymes at 0 or 1: a level of 0.0 leaves the count, and the carry is stored."""
    model = dref.toy_model()
    sm = _table(model)
    counts, partial, molecules, m2c = dref.case(model, sm.rows, n, SEED + 2, enzymes=(0, 2), transcripts=(0, 2))
    partial[:, :n] = np.random.default_rng(SEED).uniform(0.0, 0.99, (4, n))
    x, p, mol, degraded, status = _run(dev, model, sm, counts, partial, molecules, m2c, n, 1.0, 3)
    trow, erow = dref.bind(model, sm.rows)
    idle = counts[erow[0], :n] == 0
    assert np.array_equal(x[:, :n][:, idle], counts[:, :n][:, idle]) and not status.any()
    assert np.array_equal(p[:, :n][:, idle], partial[:, :n][:, idle])      # total = 0.0 + partial


@pytest.mark.parametrize('n', dref.SIZES)
def test_clamp_at_the_count(dev, n):
    """An enzyme count so large that d exceeds the transcript's count: she loses all she has, the
    pools gain exactly her bases, the carry keeps the fraction only."""
    model = dref.toy_model()
    sm = _table(model)
    counts, partial, molecules, m2c = dref.case(model, sm.rows, n, SEED + 3, enzymes=(10 ** 6, 10 ** 7), transcripts=(0, 9))
    x, p, mol, degraded, status = _run(dev, model, sm, counts, partial, molecules, m2c, n, 1.0, 2)
    trow = dref.bind(model, sm.rows)[0]
    assert not x[trow, :n].any() and not status.any() and np.all((p[:, :n] >= 0) & (p[:, :n] < 1))
    held = (counts[trow, :n].astype(np.int64)[:, :, None] * model.composition[:, None, :]).sum(axis=0).T     # [4, n]
    gained = mol[:4, :n].astype(np.int64) - molecules[:4, :n]
    bases = held.sum(axis=0)
    assert np.array_equal(gained[1:], held[1:]) and np.array_equal(gained[0], held[0] + bases)
    assert np.array_equal(mol[4, :n].astype(np.int64), molecules[4, :n] - bases)         # ADP falls, below zero too


def _wide_model(T, enzymes=8, per_transcript=4):
    from lens_amd.degradation import DegradationModel
    rng = np.random.default_rng([SEED, T])
    sequences = {'t%d' % t: ''.join(rng.choice(list('GACU'), size=int(rng.integers(1, 40)))) for t in range(T)}
    rates = {'e%d' % e: float(rng.uniform(0.01, 0.5)) for e in range(enzymes)}
    kms = {'e%d' % e: {'t%d' % t: float(rng.uniform(1, 9)) * KM for t in range(T)
                       if (t + e) % enzymes < per_transcript} for e in range(enzymes)}
    return DegradationModel(sequences, rates, {'transcripts': kms})


@pytest.mark.parametrize('n', dref.SIZES)
def test_limits(dev, n):
    """64 transcripts, 8 enzymes, 256 pairs (each transcript named by 4 enzymes: 64 x 8 pairs would
    pass VK_DEG_MAX_PAIRS), 4 monomers, the transcripts passive rows: four chunks, run twice."""
    model = _wide_model(64)
    assert (model.n_transcripts, model.n_enzymes, model.n_pairs, model.n_monomers) == (64, 8, 256, 4)
    sm = _table(model, passive=True)
    assert sm.n_rows == 64 + 10
    counts, partial, molecules, m2c = dref.case(model, sm.rows, n, SEED + 4, m2c=(0.5, 2.0))
    x, p, mol, degraded, status = _run(dev, model, sm, counts, partial, molecules, m2c, n, 1.0, 3)
    assert not status.any() and degraded.sum() > 0


@pytest.mark.parametrize('T', [15, 16, 17, 33])
def test_around_the_register_chunk(dev, T):
    """16 transcripts stay in registers; 17 and 33 take the two-pass path with a partial last chunk."""
    n = 65
    model = _wide_model(T, enzymes=3, per_transcript=2)
    sm = _table(model)
    counts, partial, molecules, m2c = dref.case(model, sm.rows, n, SEED + 5, m2c=(0.5, 2.0))
    x, p, mol, degraded, status = _run(dev, model, sm, counts, partial, molecules, m2c, n, 1.0, 3)
    assert not status.any() and degraded.sum() > 0


def _failing(dev, n, spoil, bits, T=4):
    """Every third agent is spoilt by ``spoil(counts, partial, molecules, m2c, who)``: her columns
    stay bitwise what they were, her status takes ``bits``, her neighbours are stepped."""
    model = dref.toy_model() if T == 4 else _wide_model(T, enzymes=3, per_transcript=2)
    sm = _table(model)
    # enzymes of 50 and more: every transcript loses at least one a step, so every pool moves by 2 and more
    counts, partial, molecules, m2c = dref.case(model, sm.rows, n, SEED + 6, enzymes=(50, 90), transcripts=(5, 30))
    partial[:, :n] = 0.25
    who = np.arange(n) % 3 == 0
    spoil(counts, partial, molecules, m2c, np.nonzero(who)[0])
    x, p, mol, degraded, status = _run(dev, model, sm, counts, partial, molecules, m2c, n, 1.0, 2)
    assert np.all(status[who] == bits) and not status[~who].any()
    assert np.array_equal(x[:, :n][:, who], counts[:, :n][:, who])
    assert np.array_equal(p[:, :n][:, who].view(np.int64), partial[:, :n][:, who].view(np.int64))
    assert np.array_equal(mol[:, :n][:, who], molecules[:, :n][:, who]) and not degraded[who].any()
    if n > 1:
        trow = dref.bind(model, sm.rows)[0]
        assert np.all((counts[trow, :n] - x[trow, :n]).sum(axis=0)[~who] > 0)            # the neighbours were stepped


@pytest.mark.parametrize('T', [4, 17])
@pytest.mark.parametrize('n', dref.SIZES)
def test_a_pool_at_the_edge_overflows(dev, n, T):
    def spoil(counts, partial, molecules, m2c, who):
        molecules[1 + who % 3, who] = 2 ** 31 - 2                # GTP, UTP or CTP at INT32_MAX - 1
    _failing(dev, n, spoil, dref.OVERFLOW, T)


@pytest.mark.parametrize('n', dref.SIZES)
def test_adp_at_the_floor_overflows(dev, n):
    def spoil(counts, partial, molecules, m2c, who):
        molecules[4, who] = -2 ** 31 + 1
    _failing(dev, n, spoil, dref.OVERFLOW)


@pytest.mark.parametrize('T', [4, 17])
@pytest.mark.parametrize('n', dref.SIZES)
def test_bad_mmol_to_counts_is_nonfinite(dev, n, T):
    def spoil(counts, partial, molecules, m2c, who):
        m2c[who] = np.array([0.0, np.inf, np.nan, -1.0, -np.inf])[who % 5]
    _failing(dev, n, spoil, dref.NONFINITE, T)


@pytest.mark.parametrize('n', dref.SIZES)
def test_a_total_that_is_not_finite(dev, n):
    """A tiny mmol_to_counts: the levels overflow FP64.  And a carry that is NaN already."""
    def spoil(counts, partial, molecules, m2c, who):
        m2c[who[::2]] = 1e-300
        partial[2, who[1::2]] = np.nan
    _failing(dev, n, spoil, dref.NONFINITE)


def test_bad_arguments_return_err_arg_without_a_launch(dev):
    from lens_amd import native
    model = dref.toy_model()
    sm = _table(model)
    eng = _engine(dev, model, sm)
    n, ld = 5, 8
    counts, partial, molecules, m2c = dref.case(model, sm.rows, n, SEED + 7)
    x, p, mol, m = _put(dev, counts[:, :ld], partial[:, :ld], molecules[:, :ld], m2c[:ld])
    degraded = torch.full((ld,), -7, dtype=torch.int32, device=dev)
    status = torch.zeros(ld, dtype=torch.int32, device=dev)
    before = [t.clone() for t in (x, p, mol, degraded, status)]
    s = native.stream_handle()

    def call(d, n=n, ld=ld, T=1.0, args=None):
        args = [native.ptr(t) for t in (x, p, mol, m, degraded, status)] if args is None else args
        return native._lib.vk_rna_degradation_step(ctypes.byref(d) if d is not None else None, n, ld, T, *args, s)

    def table(**change):
        d = eng.table()
        for k, v in change.items():
            setattr(d, k, v)
        return d

    bad = [table(n_transcripts=65), table(n_transcripts=0), table(n_enzymes=9), table(n_enzymes=0), table(n_pairs=257),
           table(n_pairs=-1), table(n_monomers=5), table(n_monomers=0), table(n_rows=0), table(atp_row=5),
           table(adp_row=3), table(km=0), table(pair_ptr=0), table(composition=0), None]
    for d in bad:
        assert call(d) == native.VK_ERR_ARG
    assert call(eng.table(), n=-1) == native.VK_ERR_ARG
    assert call(eng.table(), n=9) == native.VK_ERR_ARG                       # ld < n
    for T in (-1.0, float('nan'), float('inf')):
        assert call(eng.table(), T=T) == native.VK_ERR_ARG
    for missing in range(6):
        args = [native.ptr(t) for t in (x, p, mol, m, degraded, status)]
        args[missing] = 0
        assert call(eng.table(), args=args) == native.VK_ERR_ARG
    assert b'vk_rna_degradation_step' in native._lib.vk_last_error()
    assert call(eng.table(), n=0, args=[0] * 6) == native.VK_OK             # no agents: nothing to read
    torch.cuda.synchronize()
    for t, b in zip((x, p, mol, degraded, status), before):
        assert torch.equal(t, b)
    assert call(eng.table()) == native.VK_OK
    # the wrapper refuses shapes before the library sees them
    for kw in (dict(counts=x[:-1]), dict(partial=p.float()), dict(molecules=mol[:, :-1]), dict(m2c=m.float()),
               dict(n=ld + 1)):
        a = dict(counts=x, partial=p, molecules=mol, m2c=m, n=n)
        a.update(kw)
        with pytest.raises(ValueError, match='DegradationEngine.step'):
            eng.step(1.0, a['counts'], a['partial'], a['molecules'], a['m2c'], a['n'])


# -- passive rows -------------------------------------------------------------------------
def _wide_tables(passive):
    """The complexation fixture's 37 species and three more (40 active rows, 7 reactions), alone and
    with ``passive`` further rows."""
    from lens_amd.stochastic import StochasticModel
    fx = sref.load_fixture()
    species = fx['monomer_ids'] + fx['complex_ids'] + ['e0', 'e1', 'e2']
    make = lambda **kw: StochasticModel(species, fx['stoichiometry'], fx['rates'], seed=SEED, **kw)
    return make(), make(passive=['p%d' % i for i in range(passive)])


@pytest.mark.parametrize('n', [65, 257])
def test_ssa_step_leaves_passive_rows_alone(dev, n):
    from lens_amd.stochastic import StochasticEngine
    plain, wide = _wide_tables(30)
    assert (plain.n_rows, wide.n_rows, wide.n_species) == (40, 70, 40)
    rng = np.random.default_rng([SEED, n])
    ld = n + 7
    x0 = rng.integers(0, 301, (70, ld)).astype(np.int32)
    x0[:, n:] = dref.SENTINEL
    keys = torch.from_numpy(rng.choice(2 ** 31, size=ld, replace=False).astype(np.int64)).to(dev)
    a, b = torch.from_numpy(x0).to(dev), torch.from_numpy(x0[:40].copy()).to(dev)
    ea, eb = StochasticEngine(wide, dev), StochasticEngine(plain, dev)
    with pytest.raises(ValueError, match='counts'):
        ea.step(1.0, b, keys, n)                         # a [n_species, ld] table is not this model's
    fired = 0
    for k in range(3):
        ev_a, st_a = ea.step(1.0, a, keys, n)
        ev_b, st_b = eb.step(1.0, b, keys, n)
        assert torch.equal(ev_a, ev_b) and torch.equal(st_a, st_b), k
        fired += int(ev_a[:n].sum())
    assert torch.equal(a[40:], torch.from_numpy(x0[40:]).to(dev))            # rows 40..69: bitwise untouched
    assert torch.equal(a[:40], b)
    assert not torch.equal(a[:40, :n], torch.from_numpy(x0[:40, :n]).to(dev)) and fired > 0
    assert torch.equal(ea.propensities(a, n), eb.propensities(b, n))


def _division(n_src, rng):
    mothers = np.sort(rng.choice(n_src, size=n_src // 3, replace=False))
    keep = [a for a in range(n_src) if a not in set(mothers.tolist())]
    src = keep + [m for m in mothers.tolist() for _ in range(2)]
    kind = [-1] * len(keep) + [0, 1] * len(mothers)
    return np.asarray(src, dtype=np.int32), np.asarray(kind, dtype=np.int32), len(keep), mothers


@pytest.mark.parametrize('active, passive', [(40, 30), (3, 130), (40, 0)])
def test_division_splits_every_row(dev, active, passive):
    """Rows [0, S) go by today's launch (same seed, same coins); the passive rows in chunks of at
    most 64 under passive_seed(seed, chunk); halves add up to the mother row by row."""
    from lens_amd.population import PopulationPlan
    from lens_amd.stochastic import StochasticModel, divide_agent_counts, divide_counts, passive_seed
    if active == 40:
        sm = _wide_tables(passive)[1]
    else:
        sm = StochasticModel(['A', 'B', 'AB'], {'bind': {'A': -1, 'B': -1, 'AB': 1}}, {'bind': 0.5}, seed=SEED,
                             passive=['p%d' % i for i in range(passive)])
    rng = np.random.default_rng([SEED, active, passive])
    n_src, ld, ld_new, step, base = 70, 75, 100, 9, 1000
    src, kind, n_keep, mothers = _division(n_src, rng)
    n_out = len(src)
    x = rng.integers(0, 1000, (sm.n_rows, ld)).astype(np.int32)
    keys = rng.choice(2 ** 31, size=ld, replace=False).astype(np.int64)
    plan = PopulationPlan(n_src, n_out, 0, *_put(dev, src, kind))
    assert (plan.n_keep, plan.n_daughters) == (n_keep, 2 * len(mothers))
    col = types.SimpleNamespace(stochastic=sm, step_index=step, _ssa_key_base=base, _ssa_complex=lambda: None)
    old = dict(zip(('ssa', 'ssa_key'), _put(dev, x, keys)))
    new = {'ssa': torch.full((sm.n_rows, ld_new), -9, dtype=torch.int32, device=dev),
           'ssa_key': torch.full((ld_new,), -9, dtype=torch.int64, device=dev)}
    divide_agent_counts(col, plan, old, new, ld_new)(col)
    assert col._ssa_key_base == base + 2 * len(mothers)
    got, got_keys = new['ssa'].cpu().numpy(), new['ssa_key'].cpu().numpy()
    S = sm.n_species
    want, want_keys = sref.divide_counts(x[:S, :n_src], keys[:n_src], src, kind, n_keep, sm.seed, step, base)
    assert np.array_equal(got[:S, :n_out], want) and np.array_equal(got_keys[:n_out], want_keys)
    # the active rows are bitwise today's divider: one vk_divide_counts launch over rows [0, S)
    today = {'ssa': torch.full((S, ld_new), -9, dtype=torch.int32, device=dev),
             'ssa_key': torch.full((ld_new,), -9, dtype=torch.int64, device=dev)}
    divide_counts(n_out, n_keep, n_src, plan.src, plan.kind, old['ssa'][:S].clone(), old['ssa_key'], today['ssa'],
                  today['ssa_key'], sm.seed, step, base)
    assert torch.equal(new['ssa'][:S], today['ssa']) and torch.equal(new['ssa_key'], today['ssa_key'])
    for chunk, lo in enumerate(range(S, sm.n_rows, 64)):
        hi = min(lo + 64, sm.n_rows)
        want, _ = sref.divide_counts(x[lo:hi, :n_src], keys[:n_src], src, kind, n_keep, passive_seed(sm.seed, chunk),
                                     step, base)
        assert np.array_equal(got[lo:hi, :n_out], want), chunk
    assert np.all(got[:, n_out:] == -9) and np.all(got_keys[n_out:] == -9)
    for k, m in enumerate(mothers.tolist()):
        pair = got[:, n_keep + 2 * k].astype(np.int64) + got[:, n_keep + 2 * k + 1]
        assert np.array_equal(pair, x[:, m]), m                  # row by row, passive rows included
    assert np.array_equal(got[:, :n_keep], x[:, src[:n_keep]])
    if passive:
        odd = x[S:, mothers] % 2 == 1
        first = got[S:, n_keep:n_out:2] > got[S:, n_keep + 1:n_out:2]
        assert 0.3 < first[odd].mean() < 0.7                     # the odd one goes either way
