"""FlagellaModel and the restatement of its kernel (tests/flagella_ref.py), on the host:
the reference's defaults, the rejections, known answers to the last bit of a float64
evaluation in the reference's operation order, and the reference's three quirks around
a changing flagella count."""

import numpy as np
import pytest

import flagella_ref as ref
from oracle.colony import philox_uniform

from lens_amd import configs, native
from lens_amd.motility import FLAGELLA_DEFAULTS, FlagellaModel, MotilityModel

BOUNDS = (34.0, 57.5)
FIELD = np.full((17, 23), 1e-2)


def test_defaults_are_the_references():
    want = {
        'n_flagella': 5,
        'initial_state': {'CheY': 2.59, 'CheY_P': 2.59, 'cw_bias': 0.5, 'motile_state': 0, 'PMF': 170},
        'ccw_to_cw': 0.26, 'cw_to_ccw': 1.7, 'CB': 0.13, 'lambda': 0.68, 'YP_ss': 2.59, 'sigma2_Y': 1.0, 'tau': 0.2,
        'K_d': 3.1, 'H': 10.3, 'omega': 1.3, 'g_0': 40, 'g_1': 40, 'K_D': 3.06, 'flagellum_thrust': 25,
        'tumble_jitter': 120.0, 'tumble_scaling': 1 / 170, 'run_scaling': 1 / 170, 'time_step': 0.01,
    }
    assert FLAGELLA_DEFAULTS == want
    m = FlagellaModel()
    assert m.parameters == want and int(m.n_flagella) == 5
    m = FlagellaModel(7, tau=0.5, initial_state={'PMF': 140})
    assert m.parameters['tau'] == 0.5 and m.parameters['initial_state'] == dict(want['initial_state'], PMF=140)
    p = m.vk_params()
    assert (p.tau, p.YP_ss, p.H, p.g_0, p.run_scaling) == (0.5, 2.59, 10.3, 40.0, 1 / 170)
    flag, flag_int = m.initial_rows(3, 4, seed=1)
    assert flag.shape == (native.VK_FLAG_ROWS, 4) and flag_int.shape == (native.VK_FLAGI_ROWS, 4)
    assert flag_int.dtype == np.int32
    assert flag[:, :3].T.tolist() == [[2.59, 2.59, 0.5, 0.0, 140.0]] * 3 and not flag[:, 3].any()
    assert flag_int[:2, :3].tolist() == [[7] * 3] * 2 and not flag_int[:, 3].any()
    assert (flag_int[2, :3].view(np.uint32) < 2 ** 7).all()           # bits at and above have are zero


def test_initial_masks_are_seeded_halves():
    m = FlagellaModel(np.arange(4000) % 33)
    _, a = m.initial_rows(4000, 4000, seed=3)
    _, b = m.initial_rows(4000, 4000, seed=3)
    _, c = m.initial_rows(4000, 4000, seed=4)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    have, mask = a[1].astype(np.int64), a[2].view(np.uint32).astype(np.uint64)
    assert np.array_equal(have, np.arange(4000) % 33) and (mask >> have.astype(np.uint64) == 0).all()
    bits = sum(int(x).bit_count() for x in mask)
    total = int(have.sum())
    assert abs(bits - total / 2) <= 5 * (total / 4) ** 0.5          # 5 binomial standard deviations
    assert (mask[have == 32] >= 2 ** 31).any()                       # the top bit is used


@pytest.mark.parametrize('bad', [-1, 33, [1, 2, 40], 2.5, [[1, 2], [3, 4]]])
def test_counts_outside_the_range_are_rejected(bad):
    with pytest.raises(ValueError):
        FlagellaModel(bad)


def test_rejections():
    with pytest.raises(ValueError, match='unknown flagella parameters'):
        FlagellaModel(5, omega_typo=1.0)
    with pytest.raises(ValueError, match='unknown flagella initial states'):
        FlagellaModel(5, initial_state={'pmf': 1})
    with pytest.raises(ValueError, match='tau'):
        FlagellaModel(5, tau=0.0)
    with pytest.raises(ValueError, match='FlagellaModel'):
        MotilityModel(flagella={'n_flagella': 5})
    with pytest.raises(ValueError, match='every agent'):
        FlagellaModel([1, 2]).initial_rows(3, 3)
    assert MotilityModel().flagella is None


def test_config_is_the_compartments():
    m = configs.chemotaxis_variable_flagella()
    assert (m.ligand_id, m.initial_ligand, int(m.flagella.n_flagella)) == ('MeAsp', 1e-2, 5)
    m = configs.chemotaxis_variable_flagella(n_flagella=8, substeps=100, seed=4)
    assert (int(m.flagella.n_flagella), m.substeps, m.seed) == (8, 100, 4)


def test_known_answers_at_the_defaults():
    f = FLAGELLA_DEFAULTS
    delta_g, cw_to_ccw, ccw_to_cw = ref.switch_rates(f, 2.59)
    assert delta_g == 0.8318584070796469
    assert cw_to_ccw == 2.9868600094999653
    assert ccw_to_cw == 0.5658115862895514
    assert ref.cw_bias(f, 2.59) == 0.13571263629578517
    assert ref.thrust(f, 'run_scaling', 170, 5) == 125.0
    assert ref.thrust(f, 'tumble_scaling', 140, 7) == 144.1176470588235
    p01, p10 = ccw_to_cw * 0.01, cw_to_ccw * 0.01
    assert p01 / (p01 + p10) == pytest.approx(0.15926368960196843, rel=1e-14)


def test_vectorised_draws_are_the_scalar_draws():
    keys = np.array([0, 1, 5, 1000, 2 ** 31 - 1])
    for s, path in ((0, 0), (7, 16), (2 ** 33 + 5, 64 + 31)):
        u = ref.uniforms(20261019, s, keys, path)
        assert u.tolist() == [philox_uniform(20261019, s, int(k), 0, path) for k in keys]


def _agents(model, n, have, target, mask, CheY_P=2.59, PMF=170.0):
    motil = np.zeros((9, n))
    motil[ref.R['n_methyl']], motil[ref.R['chemoreceptor_activity']] = model.n_methyl, model.chemoreceptor_activity
    motil[ref.R['angle']] = 0.3
    flag = np.zeros((5, n))
    flag[ref.F['CheY']], flag[ref.F['CheY_P']], flag[ref.F['PMF']] = 2.59, CheY_P, PMF
    flag[ref.F['cw_bias']] = 0.5
    flag_int = np.zeros((3, n), dtype=np.int32)
    flag_int[0], flag_int[1] = target, have
    flag_int[2] = np.asarray(mask, dtype=np.uint32).view(np.int32)
    loc = np.stack([np.full(n, 17.3), np.full(n, 20.1)])
    return motil, flag, flag_int, loc


def test_without_noise_chey_p_stays_at_its_steady_state():
    model = MotilityModel(seed=5, flagella=FlagellaModel(5, sigma2_Y=0.0))
    motil, flag, flag_int, loc = _agents(model, 64, 5, 5, 0)
    ref.step(model, motil, flag, flag_int, loc, FIELD, BOUNDS, 1.0, 100, 0)
    assert (flag[ref.F['CheY_P']] == 2.59).all() and (flag[ref.F['CheY']] == 2.59).all()
    assert (flag[ref.F['cw_bias']] == 0.13571263629578517).all()


def test_no_flagella_and_none_wanted_is_no_motile_state():
    model = MotilityModel(seed=5, flagella=FlagellaModel(0))
    motil, flag, flag_int, loc = _agents(model, 8, 0, 0, 0)
    loc0 = loc.copy()
    ref.step(model, motil, flag, flag_int, loc, FIELD, BOUNDS, 0.01, 1, 0)
    assert (flag[ref.F['motile_state']] == 0).all() and (motil[ref.R['thrust']] == 0).all()
    assert (motil[ref.R['torque']] == 0).all() and (motil[ref.R['motor_state']] == 0).all()
    assert np.array_equal(loc, loc0) and (motil[ref.R['angle']] == 0.3).all()      # stands still, keeps its heading


def test_new_flagella_run_in_the_update_that_adds_them():
    model = MotilityModel(seed=5, flagella=FlagellaModel(5))
    motil, flag, flag_int, loc = _agents(model, 64, 0, 5, 0)
    ref.step(model, motil, flag, flag_int, loc, FIELD, BOUNDS, 0.01, 1, 0)
    assert (flag[ref.F['motile_state']] == -1).all() and (motil[ref.R['thrust']] == 125.0).all()
    assert (flag_int[1] == 5).all()
    masks = flag_int[2].view(np.uint32)
    assert (masks < 32).all() and len(set(masks.tolist())) > 8       # each new flagellum CW or CCW on its own
    want = [sum((philox_uniform(5, 0, k, 0, 64 + r) < 0.5) << r for r in range(5)) for k in range(64)]
    assert masks.tolist() == want


def test_a_removed_flagellum_still_counts_in_its_last_update():
    model = MotilityModel(seed=5, flagella=FlagellaModel(1, sigma2_Y=0.0))      # CheY_P stays: p = 0.0299
    p_cw = ref.switch_rates(FLAGELLA_DEFAULTS, 2.59)[1] * 0.01
    # agents whose flagellum does not switch in update 0
    keys = [k for k in range(200) if philox_uniform(5, 0, k, 0, 16) > p_cw][:16]
    motil, flag, flag_int, loc = _agents(model, 16, 1, 0, 1)
    ref.step(model, motil, flag, flag_int, loc, FIELD, BOUNDS, 0.01, 1, 0, keys=keys)
    assert (flag[ref.F['motile_state']] == 1).all() and (motil[ref.R['motor_state']] == 1).all()
    assert (motil[ref.R['thrust']] == 0.0).all()                     # n_flagella, the target, is 0
    assert (flag_int[1] == 0).all() and (flag_int[2] == 0).all()
    ref.step(model, motil, flag, flag_int, loc, FIELD, BOUNDS, 0.01, 1, 1, keys=keys)
    assert (flag[ref.F['motile_state']] == 0).all() and (motil[ref.R['motor_state']] == 0).all()


def test_removal_closes_the_gap_and_keeps_the_survivors_order():
    mask = np.array([0b1011001110001111], dtype=np.uint64)
    bits = [(int(mask[0]) >> i) & 1 for i in range(16)]
    for j in range(16):
        got = int(ref.remove_bit(mask, j)[0])
        assert [(got >> i) & 1 for i in range(16)] == bits[:j] + bits[j + 1:] + [0]
    assert int(ref.remove_bit(np.array([2 ** 32 - 1], dtype=np.uint64), 31)[0]) == 2 ** 31 - 1
    # through a whole update: 32 -> 9 flagella, frozen switches (omega = 0), every agent its own removals
    model = MotilityModel(seed=9, flagella=FlagellaModel(9, omega=0.0))
    rng = np.random.default_rng(2)
    start = rng.integers(0, 2 ** 32, 50, dtype=np.uint64).astype(np.uint32)
    motil, flag, flag_int, loc = _agents(model, 50, 32, 9, start)
    ref.step(model, motil, flag, flag_int, loc, FIELD, BOUNDS, 0.01, 1, 3)
    assert (flag_int[1] == 9).all()
    for k in range(50):
        alive = list(range(32))
        for r in range(23):
            del alive[min(int(philox_uniform(9, 3, k, 0, 64 + r) * (32 - r)), 31 - r)]
        want = sum(((int(start[k]) >> i) & 1) << pos for pos, i in enumerate(alive))
        assert int(flag_int[2].view(np.uint32)[k]) == want and want < 2 ** 9


def test_colony_keeps_the_refusals_of_a_motile_colony():
    import types
    from lens_amd.cells import CellModel
    from lens_amd.colony import Colony
    from lens_amd.distributed import AgentRouter
    from lens_amd.lattice import Lattice
    from lens_amd.mechanics import ContactModel
    from lens_amd.response import ANTIBIOTICS_DEFAULTS, CellResponse
    cfg = configs.glc_lct_config()
    lattice = lambda **kw: Lattice(['glc__D_e', 'lcts_e', 'MeAsp'], (8, 8), (8.0, 8.0), 10.0, 5.0, device='cpu', **kw)
    m = MotilityModel(flagella=FlagellaModel(5))
    mk = lambda **kw: Colony(cfg, 4, device='cpu', integrator='euler', motility=m, **kw)
    with pytest.raises(ValueError, match='Lattice environment'):
        mk(environment='held')
    with pytest.raises(ValueError, match='unbanded'):
        mk(environment=lattice(row_band=(0, 4), halo=1))
    with pytest.raises(ValueError, match='cells'):
        mk(environment=lattice(), cells=CellModel())
    with pytest.raises(ValueError, match='mechanics with motility'):
        mk(environment=lattice(), mechanics=ContactModel())
    with pytest.raises(ValueError, match='response with motility'):
        mk(environment=lattice(), response=CellResponse(membrane=ANTIBIOTICS_DEFAULTS['diffusion']))
    with pytest.raises(ValueError, match='router'):
        AgentRouter(types.SimpleNamespace(motility=m), 0, 1, agent_offset=0)
