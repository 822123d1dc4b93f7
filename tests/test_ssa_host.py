"""The batched Gillespie step on the host: the NumPy restatement (tests/ssa_ref.py) against
what can be known without a device -- the Philox pair against the oracle's single draw, the
multiplied-out binomial against math.comb, the draw-independent end state of the reference's
complexation network, the Poisson moments of a birth-death process, divide_split -- and the
packing and the refusals of lens_amd.stochastic.StochasticModel."""

import math

import numpy as np
import pytest

import ssa_ref as sref
from lens_amd.stochastic import StochasticModel


def test_philox_pair_first_value_is_the_oracles_draw():
    from oracle.colony import philox_uniform
    rng = np.random.default_rng(7)
    seeds = rng.integers(0, 2 ** 63, 1000)
    steps = rng.integers(0, 2 ** 32, 1000)
    keys = rng.integers(0, 2 ** 31, 1000)
    es = rng.integers(0, 2 ** 40, 1000)
    seen = set()
    for seed, step, key, e in zip(seeds.tolist(), steps.tolist(), keys.tolist(), es.tolist()):
        u1, u2 = sref.philox_pair(seed, step, np.array([key]), np.array([e]))
        assert u1[0] == philox_uniform(seed, step, key, 0, e)
        assert 0.0 <= u2[0] < 1.0 and u2[0] != u1[0]
        seen.add(float(u2[0]))
    assert len(seen) == 1000
    # vectorised == one at a time
    u1, u2 = sref.philox_pair(5, 9, keys, es)
    a1, a2 = sref.philox_pair(5, 9, keys[17:18], es[17:18])
    assert u1[17] == a1[0] and u2[17] == a2[0]


def test_choose_against_math_comb():
    for n in range(61):
        for k in range(n + 2):
            got = float(sref.choose(np.array([n]), k)[0])
            want = math.comb(n, k)
            assert abs(got - want) <= 1e-14 * want, (n, k, got, want)
    assert sref.choose(np.array([3]), 5)[0] == 0.0
    c = float(sref.choose(np.array([1000]), 120)[0])
    assert np.isfinite(c) and abs(c - math.comb(1000, 120)) <= 1e-12 * math.comb(1000, 120)
    assert np.isinf(sref.choose(np.array([100000]), 120)[0])


def test_model_packing():
    m = StochasticModel(['A', 'B', 'C'], {'r0': {'A': -2.0, 'B': -1, 'C': 1}, 'r1': {'C': -1, 'A': 2}, 'r2': {'B': 1}},
                        {'r0': 0.5, 'r1': 2.0, 'r2': 3.0}, initial={'A': 10}, seed=3, max_events=50)
    assert m.n_species == 3 and m.n_reactions == 3 and m.max_order == 2
    assert m.react_ptr.tolist() == [0, 2, 3, 3]
    assert m.react_species.tolist() == [0, 1, 2] and m.react_order.tolist() == [2, 1, 1]
    assert m.stoich_ptr.tolist() == [0, 3, 5, 6]
    assert m.stoich_species.tolist() == [0, 1, 2, 0, 2, 1] and m.stoich_delta.tolist() == [-2, -1, 1, 2, -1, 1]
    assert m.rates.tolist() == [0.5, 2.0, 3.0]
    assert m.inv.shape == (255,) and m.inv[2] == 1.0 / 3.0
    assert m.initial_counts(2, 4).tolist() == [[10, 10, 0, 0], [0] * 4, [0] * 4]
    assert m.react_ptr.dtype == np.int32 and m.inv.dtype == np.float64
    # rates as a sequence in the stoichiometry's order
    assert StochasticModel(['A'], {'r': {'A': 1}}, [2.0]).rates.tolist() == [2.0]
    fx = sref.fixture_model()
    assert fx.n_species == 37 and fx.n_reactions == 7 and fx.max_order == 120
    assert int((fx.matrix < 0).sum()) == 35            # 30 monomers, each in one reaction, and 5 complexes


@pytest.mark.parametrize('make', [
    lambda: StochasticModel(['s%d' % i for i in range(65)], {'r': {'s0': 1}}, {'r': 1.0}),           # S > 64
    lambda: StochasticModel(['A'], {'r%d' % i: {'A': 1} for i in range(33)}, [1.0] * 33),            # R > 32
    lambda: StochasticModel(['A'], {'r': {'A': -256}}, {'r': 1.0}),                                  # order > 255
    lambda: StochasticModel(['A'], {'r': {'A': -1.5}}, {'r': 1.0}),                                  # not integral
    lambda: StochasticModel(['A'], {'r': {'B': 1}}, {'r': 1.0}),                                     # unknown species
    lambda: StochasticModel(['A'], {'r': {'A': 1}}, {'q': 1.0}),                                     # unknown reaction
    lambda: StochasticModel(['A'], {'r': {'A': 1}}, {}),                                             # no rate
    lambda: StochasticModel(['A'], {'r': {'A': 1}}, {'r': -1.0}),                                    # negative rate
    lambda: StochasticModel(['A'], {'r': {'A': 1}}, {'r': float('nan')}),
    lambda: StochasticModel(['A', 'A'], {'r': {'A': 1}}, {'r': 1.0}),                                # duplicate ids
    lambda: StochasticModel(['A'], {'r': {'A': 1}}, {'r': 1.0}, initial={'B': 1}),
    lambda: StochasticModel(['A'], {'r': {'A': 1}}, {'r': 1.0}, initial={'A': -1}),
    lambda: StochasticModel(['A'], {'r': {'A': 1}}, {'r': 1.0}, initial={'A': 0.5}),
    lambda: StochasticModel(['A'], {'r': {'A': 1}}, {'r': 1.0}, max_events=0),
    lambda: StochasticModel([], {'r': {}}, {'r': 1.0}),
    lambda: StochasticModel(['A'], {}, {}),
])
def test_model_refusals(make):
    with pytest.raises(ValueError):
        make()


def test_order_255_and_float_entries_are_accepted():
    m = StochasticModel(['A', 'B'], {'r': {'A': -255.0, 'B': 1.0}}, {'r': 1e-4})
    assert m.max_order == 255 and m.stoich_delta.tolist() == [-255, 1]


def test_colony_refuses_before_anything_is_built():
    """Row bands, a response, a FlagellaModel(complexes=...) without the network or the
    species: ValueError before the colony compiles its table or allocates a buffer."""
    torch = pytest.importorskip('torch')
    from lens_amd import colony, configs
    from lens_amd.lattice import Lattice
    from lens_amd.motility import FlagellaModel, MotilityModel
    from lens_amd.response import ANTIBIOTICS_DEFAULTS, CellResponse
    model = sref.birth_death_model()
    cfg = configs.glc_lct_config()
    lattice = lambda **kw: Lattice(['glc__D_e', 'lcts_e', 'MeAsp'], (8, 8), (8.0, 8.0), 10.0, 5.0, device='cpu', **kw)
    motile = lambda fm: MotilityModel(flagella=fm)
    cases = [
        (dict(environment='held', stochastic='not a model'), 'StochasticModel'),
        (dict(environment=lattice(row_band=(0, 4), halo=1), stochastic=model), 'unbanded'),
        (dict(environment='nonspatial', stochastic=model,
              response=CellResponse(expression=ANTIBIOTICS_DEFAULTS['ode_expression'])), 'response'),
        (dict(environment=lattice(), motility=motile(FlagellaModel(0, complexes='X'))), 'stochastic='),
        (dict(environment=lattice(), motility=motile(FlagellaModel(0, complexes='flagella')), stochastic=model),
         'no species'),
    ]

    def refuse(*args, **kw):
        raise AssertionError('the colony went on building')

    saved = colony.compile_rate_laws
    colony.compile_rate_laws = refuse
    try:
        for kw, match in cases:
            with pytest.raises(ValueError, match=match):
                colony.Colony(cfg, 4, device='cpu', integrator='euler', **kw)
    finally:
        colony.compile_rate_laws = saved
    with pytest.raises(ValueError, match='not both'):
        FlagellaModel(0, expression=configs.flagella_expression(), complexes='flagella')
    with pytest.raises(ValueError):
        FlagellaModel(0, complexes=3)
    assert FlagellaModel(0, complexes='flagella').complexes == 'flagella' and FlagellaModel(3).complexes is None


def test_router_refuses_a_stochastic_colony():
    import types
    from lens_amd.distributed import AgentRouter
    with pytest.raises(ValueError, match='stochastic'):
        AgentRouter(types.SimpleNamespace(motility=None, mechanics=None, stochastic=sref.birth_death_model()), 0, 1,
                    agent_offset=0)


BURST_END = {'flhDC': 250, 'flagellar motor switch': 0, 'flagella': 8, 'flagellar export apparatus subunit': 83,
             'flagellar export apparatus': 75, 'flagellar hook': 0, 'flagellar motor': 21}


def test_complexation_burst_end_state():
    """From 1000 of every monomer, one step of 1 s: no monomer is shared between reactions,
    so the end state does not depend on the draws."""
    m = sref.fixture_model(1000, seed=11)
    n = 5
    x = m.initial_counts(n, n)
    keys = np.arange(n)
    events, status, _ = sref.step(m, x, keys, 1.0, m.seed, 0)
    assert events.tolist() == [573] * n and not status.any()
    for name, want in BURST_END.items():
        assert x[m.index(name)].tolist() == [want] * n, name
    for k in (1, 2):
        before = x.copy()
        events, status, _ = sref.step(m, x, keys, 1.0, m.seed, k)
        assert not events.any() and not status.any() and np.array_equal(x, before)


def test_status_bits_of_the_restatement():
    m = sref.fixture_model(1000, seed=1)
    x = m.initial_counts(2, 2)
    events, status, _ = sref.step(m, x, np.arange(2), 1.0, 1, 0, max_events=10)
    assert events.tolist() == [10, 10] and status.tolist() == [sref.MAX_EVENTS] * 2
    x = sref.fixture_model(100000).initial_counts(1, 1)
    before = x.copy()
    events, status, _ = sref.step(m, x, np.arange(1), 1.0, 1, 0)
    assert events.tolist() == [0] and status.tolist() == [sref.NONFINITE] and np.array_equal(x, before)
    birth = sref.birth_model()
    x = np.array([[2 ** 31 - 3, 5]], dtype=np.int32)       # two births fit, the third does not
    events, status, _ = sref.step(birth, x, np.arange(2), 1.0, 3, 0)
    assert status.tolist() == [sref.OVERFLOW, 0] and events[0] == 2 and x[0, 0] == 2 ** 31 - 1
    assert events[1] > 20 and x[0, 1] == 5 + events[1]


def birth_death_moments(x20):
    lam = 100.0 * (1.0 - math.exp(-10.0))
    n = x20.shape[0]
    assert n == 4096
    mean, var = float(x20.mean()), float(x20.var(ddof=1))
    assert abs(mean - lam) <= 5.0 * math.sqrt(lam / n), mean                        # 0.78
    assert abs(var - lam) <= 5.0 * math.sqrt((lam + 2.0 * lam * lam) / n), var      # 11


def test_birth_death_moments():
    """0 -> X at 50/s, X -> 0 at 0.5/s per molecule, from X = 0: X(20) is Poisson with
    lambda = 100 (1 - exp(-10))."""
    m = sref.birth_death_model(seed=2026)
    n = 4096
    x = np.zeros((1, n), dtype=np.int32)
    keys = np.arange(n)
    for k in range(20):
        _, status, _ = sref.step(m, x, keys, 1.0, m.seed, k)
        assert not status.any()
    birth_death_moments(x[0])


def test_divide_split_restated():
    rng = np.random.default_rng(5)
    S, n = 6, 40
    x = rng.integers(0, 2000, (S, n)).astype(np.int32)
    keys = np.arange(100, 100 + n)
    mothers = [3, 7, 8, 30]
    removed = [0, 12]
    keep = [a for a in range(n) if a not in mothers and a not in removed]
    src = keep + [a for mth in mothers for a in (mth, mth)]
    kind = [-1] * len(keep) + [0, 1] * len(mothers)
    out, new_keys = sref.divide_counts(x, keys, src, kind, len(keep), 77, 4, 1000)
    assert np.array_equal(out[:, :len(keep)], x[:, keep]) and np.array_equal(new_keys[:len(keep)], keys[keep])
    assert new_keys[len(keep):].tolist() == list(range(1000, 1000 + 2 * len(mothers)))
    for i, mth in enumerate(mothers):
        d0, d1 = out[:, len(keep) + 2 * i], out[:, len(keep) + 2 * i + 1]
        assert np.array_equal(d0 + d1, x[:, mth])
        assert np.abs(d0.astype(np.int64) - d1).max() <= 1
    # the odd one goes both ways over species and mothers
    odd = np.array([out[:, len(keep) + 2 * i] - out[:, len(keep) + 2 * i + 1] for i in range(len(mothers))])
    assert (odd == 1).any() and (odd == -1).any()
    assert sref.split_int(np.array([7, 7, 6]), np.array([0.2, 0.7, 0.2]))[0].tolist() == [4, 3, 3]
