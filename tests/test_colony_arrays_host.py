"""colony.AGENT_ARRAYS on the host: agent_array_names() filters the table by what a colony
holds, also on objects made by Colony.__new__ that have only some attributes, and
lattice.whole_plane reads the four band attributes of whatever it is given."""

from types import SimpleNamespace

import pytest

torch = pytest.importorskip('torch')

from lens_amd.colony import AGENT_ARRAYS, CAPACITY_SCRATCH, Colony
from lens_amd.lattice import whole_plane

TABLE = ['params', 'conc', 'm2c', 'flux', 'counts', 'status', 'nsteps', 'h_state', 'location', 'cell', 'divide',
         'lin_root', 'lin_depth', 'lin_path', 'dead', 'frozen', 'motil', 'flag', 'flag_int', 'flag_expr', 'motile_key',
         'mech_angle', 'ordinal', 'env_fields']


def test_the_table_names_every_array_once_in_the_reported_order():
    names = [name for name, _ in AGENT_ARRAYS]
    assert names == TABLE and len(set(names)) == len(names)
    assert not set(names) & set(CAPACITY_SCRATCH)


def test_names_of_partly_built_colonies():
    col = Colony.__new__(Colony)
    assert col.agent_array_names() == []                 # nothing set: no AttributeError
    col.flag_int = torch.zeros((3, 5), dtype=torch.int32)
    col.conc = torch.zeros((4, 5))
    col.env_fields = torch.zeros((1, 5))
    col.status = torch.zeros(5, dtype=torch.int32)
    assert col.agent_array_names() == ['conc', 'status', 'flag_int', 'env_fields']         # table order
    col.location = None                                  # declared and absent
    col.ordinal = torch.zeros(5, dtype=torch.int64)
    col.cell = 'not a tensor'
    assert col.agent_array_names() == ['conc', 'status', 'flag_int', 'ordinal', 'env_fields']
    col.env_fields = None
    assert col.agent_array_names() == ['conc', 'status', 'flag_int', 'ordinal']
    for name in TABLE:
        setattr(col, name, torch.zeros(5))
    assert col.agent_array_names() == TABLE


def test_optional_attributes_are_declared():
    col = Colony.__new__(Colony)
    for name in ('agent_order', 'attempts', '_flag_flags', '_x_stream', '_p_stream', '_counts_alt', 'flux_steps',
                 'counts_steps', 'nsteps_steps', 'location', 'ordinal', 'env_fields'):
        assert getattr(col, name) is None, name


@pytest.mark.parametrize('pad', [False, True])
@pytest.mark.parametrize('edge', [False, True])
def test_whole_plane(pad, edge):
    lat = SimpleNamespace(pad_top=0, pad_bot=2 if pad else 0, edge_top=True, edge_bot=edge)
    assert whole_plane(lat) is (edge and not pad)
    lat = SimpleNamespace(pad_top=2 if pad else 0, pad_bot=0, edge_top=edge, edge_bot=True)
    assert whole_plane(lat) is (edge and not pad)
