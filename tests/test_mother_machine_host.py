"""Mother machine, host side: the ContactModel's ``channels=`` validation, the
placement of configs.mother_machine, and the NumPy restatement's own scenario
(tests/mother_machine_ref.py) -- the reference's mother-machine configuration,
20 x 20 um, channel height 14, channel space 1.5, three cells growing 0.6 % per
second and dividing at 2.6 fL, four contact iterations with jitter 0.005, 600
steps.  No GPU and no library."""

import math

import numpy as np
import pytest

import mother_machine_ref as mm_ref
from lens_amd import configs
from lens_amd.mechanics import ContactModel

CH = {'channel_height': 14.0, 'channel_space': 1.5}
STEPS, JITTER, SEED = 600, 0.005, 11


def test_defaults_round_trip():
    m = ContactModel(channels=CH)
    assert m.channels == {'channel_height': 14.0, 'channel_space': 1.5, 'spacer_thickness': 0.1}
    assert ContactModel().channels is None
    assert ContactModel(channels=dict(CH, spacer_thickness=0.2)).channels['spacer_thickness'] == 0.2
    assert m.n_lines((20.0, 20.0)) == 13
    assert CH == {'channel_height': 14.0, 'channel_space': 1.5}          # the caller's dict is not touched


def test_every_rule_raises():
    with pytest.raises(ValueError, match='unknown channels keys'):
        ContactModel(channels=dict(CH, channel_width=1.0))
    with pytest.raises(ValueError, match='channel_space'):
        ContactModel(channels={'channel_height': 14.0})
    with pytest.raises(ValueError, match='channel_height'):
        ContactModel(channels={'channel_space': 1.5})
    for h in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='channel_height must be positive'):
            ContactModel(channels=dict(CH, channel_height=h))
    with pytest.raises(ValueError, match='spacer_thickness'):
        ContactModel(channels=dict(CH, spacer_thickness=-0.1))
    # channel_space >= width + 2 * spacer_thickness: 1.2 is the least for width 1
    ContactModel(channels=dict(CH, channel_space=1.2))
    with pytest.raises(ValueError, match='width \\+ 2 \\* spacer_thickness'):
        ContactModel(channels=dict(CH, channel_space=1.19))
    with pytest.raises(ValueError, match='width \\+ 2 \\* spacer_thickness'):
        ContactModel(width=1.4, max_length=4.0, channels=CH)
    # against the plane
    m = ContactModel(channels=CH)
    m.check_channels((20.0, 14.0))
    with pytest.raises(ValueError, match='bound_y'):
        m.check_channels((20.0, 13.9))
    with pytest.raises(ValueError, match='no line'):
        m.check_channels((1.4, 20.0))


def test_colony_checks_the_channels_against_the_lattice_before_anything_is_built():
    """Colony.__init__ raises on the lattice's bounds before it touches the device."""
    from lens_amd.colony import Colony
    from lens_amd.lattice import Lattice

    class Plane(Lattice):                # bounds only: nothing is allocated
        def __init__(self, bounds):
            self.bounds, self.molecules = bounds, ['glc__D_e']
            self.pad_top = self.pad_bot = 0
            self.edge_top = self.edge_bot = True

    with pytest.raises(ValueError, match='bound_y'):
        Colony(configs.glc_lct_config(), 3, environment=Plane((20.0, 13.0)), mechanics=ContactModel(channels=CH))
    with pytest.raises(ValueError, match='no line'):
        Colony(configs.glc_lct_config(), 3, environment=Plane((1.0, 20.0)), mechanics=ContactModel(channels=CH))


def test_mother_machine_placement():
    mm = configs.mother_machine()
    assert mm['bounds'] == (20.0, 20.0) and mm['n_bins'] == (10, 10)
    assert mm['channels'] == {'channel_height': 0.7 * 20.0, 'channel_space': 1.5, 'spacer_thickness': 0.1}
    assert mm['growth_rate'] == 0.006 and mm['division_volume'] == 2.6 and mm['length'] == 2.0 and mm['width'] == 1.0
    loc = mm['location']
    assert loc.shape == (2, 3) and (loc[1] == 0.01).all() and (mm['angle'] == math.pi / 2).all()
    k = (loc[0] + 0.75) / 1.5                                   # x = k * space - space / 2
    assert np.array_equal(k, np.round(k)) and len(set(k)) == 3 and k.min() >= 1 and k.max() <= 12
    # every possible location once, in an order that is shuffled and seeded
    full = configs.mother_machine(n_agents=12)['location'][0]
    assert sorted(full) == [j * 1.5 - 0.75 for j in range(1, 13)] and list(full) != sorted(full)
    assert np.array_equal(full[:3], loc[0])
    assert not np.array_equal(configs.mother_machine(n_agents=12, seed=5)['location'][0], full)
    with pytest.raises(ValueError, match='more agents'):
        configs.mother_machine(n_agents=13)
    # the cell: DeriveGlobals gives the mass's length and volume back
    volume, length = mm_ref.derive(np.array([mm['mass']]), 1.0)
    assert abs(length[0] - 2.0) < 1e-12 and abs(volume[0] - mm['volume']) < 1e-12
    # a ContactModel takes the channels as they are
    assert ContactModel(channels=mm['channels']).n_lines(mm['bounds']) == 13


def test_plan_restatement():
    src, kind, n_out = mm_ref.plan([0, 1, 0, 1, 1], [0, 0, 1, 1, 0], 5)
    assert n_out == 5 and src.tolist() == [0, 1, 1, 4, 4] and kind.tolist() == [-1, 0, 1, 0, 1]
    assert mm_ref.plan(None, [1, 1], 2)[2] == 0 and mm_ref.plan(None, None, 3)[0].tolist() == [0, 1, 2]


def test_projection_restatement():
    b, kw = (20.0, 20.0), dict(width=1.0, height=14.0, space=1.5, spacer=0.1)
    one = lambda *a: [np.array([v], dtype=np.float64) for v in a]
    # a long tilted cell: turned until its spine fits (|cos| = 0.3 / 2.6), centred in its channel
    xs, x, y, th, L = one(2.2, 2.4, 5.0, 0.5, 3.6)
    nx, nth, out = mm_ref.project(xs, x, y, th, L, b, **kw)
    assert not out[0] and abs(abs(math.cos(nth[0])) - 0.3 / 2.6) < 1e-15 and math.sin(nth[0]) > 0 and \
        math.cos(nth[0]) > 0 and abs(nx[0] - 2.25) < 1e-15
    # above the channels: untouched, flagged
    nx, nth, out = mm_ref.project(*one(2.2, 2.9, 14.5, 0.5, 3.6), b, **kw)
    assert out[0] and nx[0] == 2.9 and nth[0] == 0.5
    # right of the last line (18): the plane's edge stands in
    nx, nth, out = mm_ref.project(*one(19.0, 19.99, 3.0, 0.0, 2.0), b, **kw)
    assert nth[0] == 0.0 and nx[0] == np.nextafter(20.0, 0.0) - 0.5
    # a disc keeps its angle
    nx, nth, out = mm_ref.project(*one(0.7, 0.1, 3.0, 0.3, 1.0), b, **kw)
    assert nth[0] == 0.3 and nx[0] == 0.6


@pytest.fixture(scope='module')
def scenario():
    sc = mm_ref.Scenario(configs.mother_machine(), jitter=JITTER, seed=SEED)
    occupied = sorted(set(sc.root_channel.tolist()))
    pop = mm_ref.check_scenario(lambda: sc.n, sc.step, sc.in_own_channels, sc.stale_above,
                                lambda: sc.removed_per_channel, STEPS, occupied)
    return sc, pop


def test_scenario(scenario):
    """The four assertions hold after every one of the 600 steps (check_scenario)."""
    sc, pop = scenario
    print('mother machine restatement: peak population', max(pop), 'final', pop[-1], 'removed',
          int(sc.removed_per_channel.sum()))
    assert max(pop) > pop[-1] > 0 and sc.removed_per_channel.sum() >= 3
