"""Host side of the motile colony (no GPU): the steady-state constructor of
MotilityModel against values computed from the reference's formulas, the
argument checks of Colony(motility=...), and self-checks of the NumPy
restatement the GPU tests compare the kernel with (tests/motility_ref.py)."""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import motility_ref as ref
from lens_amd import configs
from lens_amd.cells import CellModel
from lens_amd.motility import MotilityModel

# ReceptorCluster run to steady state (timestep 1.0, delta <= 1e-6) with the defaults
STEADY = {
    0.0: (1.9230337697803324, 0.3334335872209617, 127),
    0.1: (3.662184786345037, 0.3334052634844098, 354),
    5.0: (5.746220202941506, 0.3334035872034941, 569),
}


@pytest.mark.parametrize('ligand', sorted(STEADY))
def test_constructor_runs_the_receptor_to_steady_state(ligand):
    n_methyl, P_on, iterations = STEADY[ligand]
    m = MotilityModel(initial_ligand=ligand)
    assert abs(m.n_methyl - n_methyl) <= 1e-12 * n_methyl
    assert abs(m.chemoreceptor_activity - P_on) <= 1e-12 * P_on
    assert m.steady_iterations == iterations
    rows = m.initial_rows(3, 5)
    assert rows.shape == (9, 5)
    assert np.all(rows[ref.R['n_methyl'], :3] == m.n_methyl) and np.all(rows[:, 3:] == 0)
    # MotorActivity's initial_state: tumbling, CheY_P / bias / ccw_to_cw at 0.5
    assert np.all(rows[ref.R['motor_state'], :3] == 1) and np.all(rows[ref.R['CheY_P'], :3] == 0.5)
    assert np.all((rows[ref.R['angle'], :3] >= 0) & (rows[ref.R['angle'], :3] < 2 * np.pi))
    assert np.array_equal(rows, m.initial_rows(3, 5))         # seeded headings
    given = MotilityModel(initial_ligand=ligand, angles=[0.5, 1.5, 2.5]).initial_rows(3, 5)
    assert np.array_equal(given[ref.R['angle']], [0.5, 1.5, 2.5, 0.0, 0.0])
    with pytest.raises(ValueError, match='heading'):
        MotilityModel(angles=[0.5]).initial_rows(3, 5)


def test_model_rejects_unknown_parameters():
    with pytest.raises(ValueError, match='receptor'):
        MotilityModel(receptor={'K_Tar': 1.0})
    with pytest.raises(ValueError, match='motor'):
        MotilityModel(motor={'mb0': 1.0})
    with pytest.raises(ValueError, match='substeps'):
        MotilityModel(substeps=0)


def _lattice(molecules=('glc__D_e', 'lcts_e', 'MeAsp'), **kw):
    from lens_amd.lattice import Lattice
    return Lattice(list(molecules), (8, 8), (8.0, 8.0), 10.0, 5.0, device='cpu', **kw)


def test_colony_names_each_unsupported_combination():
    from lens_amd.colony import Colony
    cfg = configs.glc_lct_config()
    m = MotilityModel()
    mk = lambda **kw: Colony(cfg, 4, device='cpu', integrator='euler', motility=m, **kw)
    with pytest.raises(ValueError, match='Lattice environment'):
        mk(environment='held')
    with pytest.raises(ValueError, match='Lattice environment'):
        mk(environment='nonspatial')
    with pytest.raises(ValueError, match="no 'MeAsp' plane"):
        mk(environment=_lattice(('glc__D_e', 'lcts_e')))
    with pytest.raises(ValueError, match='unbanded'):
        mk(environment=_lattice(row_band=(0, 4), halo=1))
    with pytest.raises(ValueError, match='cells'):
        mk(environment=_lattice(), cells=CellModel())


def test_router_refuses_a_motile_colony():
    """The router attaches after construction, so it makes the check itself (before
    it touches the colony: a stand-in with the attribute is enough here)."""
    import types
    from lens_amd.distributed import AgentRouter
    with pytest.raises(ValueError, match='router'):
        AgentRouter(types.SimpleNamespace(motility=MotilityModel()), 0, 1, agent_offset=0)


def test_restatement_keeps_the_clamp_quirk():
    """An out-of-range n_methyl is clamped and NOT advanced in that update
    (chemoreceptor_cluster.py:177-183); an in-range one moves by d_methyl."""
    m = MotilityModel()
    nm0 = np.array([-0.5, 8.5, 3.0, 0.0, 8.0])
    P = np.full(5, 0.2)
    nm, _ = ref.receptor(m.receptor, nm0, P, np.full(5, 0.1), 0.1)
    d = 1.2 * (0.0625 * (0.00016 * 1e3) * (1.0 - 0.2) - 0.0714 * (0.00028 * 1e3) * 0.2) * 0.1
    assert d != 0
    assert nm[0] == 0.0 and nm[1] == 8.0
    assert nm[2] == 3.0 + d and nm[3] == 0.0 + d and nm[4] == 8.0 + d
    # and the model's own scalar restatement agrees with the vectorised one
    from lens_amd.motility import receptor_update
    for a in range(5):
        s_nm, s_P = receptor_update(m.receptor, float(nm0[a]), 0.2, 0.1, 0.1)
        v_nm, v_P = ref.receptor(m.receptor, nm0[a:a + 1], P[:1], np.array([0.1]), 0.1)
        assert s_nm == v_nm[0] and abs(s_P - v_P[0]) <= 1e-15


def test_restatement_switching_rate_rises_with_receptor_activity():
    """The reference's own test_variable_receptor assertion (coarse_motor.py:200-223)."""
    m = MotilityModel()
    _, _, c2c = ref.motor_rates(m.motor, np.linspace(0.0, 1.0, 501))
    assert np.all(c2c[:-1] <= c2c[1:])
    assert c2c.max() < 0.81 and c2c.min() == m.motor['cw_to_ccw_leak']
