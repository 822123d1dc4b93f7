"""colony.AGENT_ARRAYS on the host: agent_array_names() filters the table by what a colony
holds, also on objects made by Colony.__new__ that have only some attributes, and
lattice.whole_plane reads the four band attributes of whatever it is given.  The host side
of lens_amd/population.py: the dispatch of the named dividers and the order regather runs
them in, the plan's arithmetic against the restated plan, the capacity rule and the install."""

import inspect
import re
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import mother_machine_ref as mref
from lens_amd import native, population
from lens_amd import polymerize
from lens_amd.colony import AGENT_ARRAYS, CAPACITY_SCRATCH, STOCHASTIC_STAGES, Colony, stage_attributes
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


def test_every_named_divider_has_one_function():
    named = {divider for _, divider in population._ALL_AGENT_ARRAYS if isinstance(divider, str)}
    assert named == set(population.DIVIDERS) == {'locations', 'lineage', 'flagella', 'given', 'counts', 'ribosomes',
                                                 'molecules'}
    functions = list(population.DIVIDERS.values())
    assert all(callable(f) for f in functions) and len(set(functions)) == len(functions)


class _NoLibrary:
    """Every launch returns VK_OK and does nothing: the host side of regather alone."""

    def __getattr__(self, name):
        return lambda *args: 0


def _everything(n, ld):
    """A colony made by Colony.__new__ that holds every array of the table, on the CPU."""
    col = Colony.__new__(Colony)
    dtypes = {'counts': torch.int64, 'lin_path': torch.int64, 'motile_key': torch.int64, 'ordinal': torch.int64,
              'ssa_key': torch.int64}
    for name, _ in population._ALL_AGENT_ARRAYS:
        rows = native.VK_CELL_ROWS if name == 'cell' else 2
        shape = (ld,) if name in ('m2c', 'lin_root', 'lin_depth', 'lin_path', 'ordinal', 'ssa_key', 'motile_key') \
            else (rows, ld)
        setattr(col, name, torch.zeros(shape, dtype=dtypes.get(name, torch.float64)))
    col.n, col.ld, col.device, col._layout, col.lattice = n, ld, torch.device('cpu'), 0, None
    col.motility = col.mechanics = col.response = None
    return col


def test_a_divider_finds_only_the_arrays_before_it(monkeypatch):
    """regather runs the plain modes, then the named dividers in table order; of the new arrays
    a divider finds its own, the plain-mode ones and those of the named dividers before it --
    so whatever it reads of the new layout has been written.  The launches are stubbed out."""
    monkeypatch.setattr(native, '_lib', _NoLibrary())
    monkeypatch.setattr(native, 'stream_handle', lambda stream=None: 0)
    seen = []
    for divider in population.DIVIDERS:
        monkeypatch.setitem(population.DIVIDERS, divider,
                            lambda col, plan, old, new, ld, divider=divider: seen.append((divider, set(new), ld)))
    col = _everything(5, 8)
    old = {name: getattr(col, name) for name in col.agent_array_names()}
    src = torch.tensor([0, 1, 2, 3, 4, 4, 0, 0, 0, 0], dtype=torch.int32)
    plan = population.PopulationPlan(5, 9, 0, src, torch.full((10,), -1, dtype=torch.int32))
    population.regather(col, plan)
    table = population._ALL_AGENT_ARRAYS
    plain = {name for name, divider in table if not isinstance(divider, str)}
    order = list(dict.fromkeys(divider for _, divider in table if isinstance(divider, str)))
    assert [divider for divider, _, _ in seen] == order
    for k, (divider, found, ld) in enumerate(seen):
        assert found == plain | {name for name, d in table if d in order[:k + 1]}, divider
        assert ld == population.grown_capacity(8, 9) == 74
    # what the dividers in the library read of the new arrays: the daughters' places come from
    # the gathered ``cell`` rows, a plain mode; nothing else reads a new array of another divider
    assert 'cell' in plain
    assert col.n == 9 and col.ld == 74 and col._layout == 2         # the install and the capacity hook
    for name in old:
        assert getattr(col, name) is not old[name] and getattr(col, name).shape[-1] == 74, name


@pytest.mark.parametrize('n', [1, 7, 255, 256, 257, 1025])
@pytest.mark.parametrize('case', ['random', 'all zero', 'all removed', 'removed mothers', 'divide only', 'remove only'])
def test_population_plan_arithmetic(n, case):
    """n_daughters and n_keep from the three counts the host knows, against the restated plan."""
    rng = np.random.default_rng(1000 * n + len(case))
    divide, remove = (rng.random(n) < 0.3).astype(np.int32), (rng.random(n) < 0.3).astype(np.int32)
    if case == 'all zero':
        divide[:], remove[:] = 0, 0
    elif case == 'all removed':
        remove[:] = 1
    elif case == 'removed mothers':
        divide[:] = 1
        remove[::2] = 1                                 # a removed mother leaves no daughters
    elif case == 'divide only':
        remove = None
    elif case == 'remove only':
        divide = None
    src, kind, n_out = mref.plan(divide, remove, n)
    n_removed = 0 if remove is None else int((remove != 0).sum())
    plan = population.PopulationPlan(n, n_out, n_removed, torch.from_numpy(src), torch.from_numpy(kind))
    assert plan.n_daughters == int((kind >= 0).sum()) and plan.n_keep == int((kind < 0).sum())
    assert plan.n_keep + plan.n_daughters == n_out == len(src)
    if case == 'removed mothers':
        assert plan.n_daughters == 2 * (n - n_removed) and plan.n_keep == 0
    if case in ('all zero', 'remove only'):
        assert plan.n_daughters == 0
    with pytest.raises(AttributeError):
        plan.n_out = 0                                  # immutable


def test_grown_capacity():
    assert population.grown_capacity(64, 64) == 64 and population.grown_capacity(64, 0) == 64
    assert population.grown_capacity(64, 65) == int(64 * 1.25) + 64 == 144
    assert population.grown_capacity(64, 1000) == 1000
    assert population.grown_capacity(0, 1) == 64


def _plain_colony(n, ld):
    col = Colony.__new__(Colony)
    col.n, col.ld, col.device, col._layout, col.lattice = n, ld, torch.device('cpu'), 0, None
    col.motility = col.mechanics = col.response = None
    col.conc = torch.arange(3.0 * ld).reshape(3, ld)
    col.status = torch.arange(ld, dtype=torch.int32)
    return col


def test_install_sets_the_arrays_and_always_moves_the_layout(monkeypatch):
    col = _plain_colony(4, 6)
    hooks = []
    monkeypatch.setattr(Colony, '_capacity_scratch', lambda self: hooks.append(self.ld))
    conc, status = torch.ones(3, 6), torch.ones(6, dtype=torch.int32)
    population.install(col, {'conc': conc, 'status': status}, 5)
    assert col.conc is conc and col.status is status and (col.n, col.ld) == (5, 6)
    assert col._layout == 1 and hooks == []             # the capacity holds: no hook, and still a new layout
    assert col.agent_order is None
    # past the capacity: the caller sizes the arrays by the one rule, ld follows, the hook runs once
    ld = population.grown_capacity(col.ld, 7)
    assert ld == 71
    order = torch.arange(7)
    population.install(col, {'conc': torch.ones(3, ld), 'status': torch.ones(ld, dtype=torch.int32),
                             'agent_order': order}, 7)
    assert (col.n, col.ld) == (7, ld) and hooks == [ld] and col._layout == 2
    assert col.agent_order is order and col.conc.shape == (3, ld)


def test_install_through_the_real_capacity_hook():
    col = _plain_colony(4, 6)
    col.env_fields = torch.zeros(1, 6)
    population.install(col, {'conc': torch.ones(3, 9), 'status': torch.ones(9, dtype=torch.int32),
                             'env_fields': torch.ones(1, 9)}, 8)
    assert col.ld == 9 and col.env_bins.tolist() == list(range(9))
    assert col._layout == 2                             # the hook's bump and the install's


def test_install_refuses_what_is_no_per_agent_array():
    col = _plain_colony(4, 6)
    before = (col.conc, col.status, col.n, col.ld, col._layout)
    with pytest.raises(ValueError, match='bin_lin'):
        population.install(col, {'conc': torch.ones(3, 6), 'bin_lin': torch.zeros(6, dtype=torch.int32)}, 4)
    with pytest.raises(ValueError, match='one capacity'):
        population.install(col, {'conc': torch.ones(3, 6), 'status': torch.ones(7, dtype=torch.int32)}, 4)
    with pytest.raises(ValueError, match='one capacity'):
        population.install(col, {'conc': torch.ones(3, 6)}, 7)
    assert (col.conc, col.status, col.n, col.ld, col._layout) == before


def test_install_reads_the_status_words_before_the_columns_move():
    col = _plain_colony(4, 6)
    col._ssa, col._tl = object(), None
    col._ssa_status = torch.tensor([0, 0, 8, 0, 0, 0], dtype=torch.int32)
    conc = col.conc
    with pytest.raises(FloatingPointError, match='agent 2: stochastic step status 8'):
        population.install(col, {'conc': torch.ones(3, 6)}, 3)
    assert col.conc is conc and col.n == 4 and col._layout == 0


def test_the_stage_table_names_declared_attributes_and_capacity_scratch():
    for stage in STOCHASTIC_STAGES:
        for name in stage_attributes(stage):
            assert name in vars(Colony) and vars(Colony)[name] is None, name     # declared None at class level
        assert stage.events in CAPACITY_SCRATCH and stage.status in CAPACITY_SCRATCH
        pol = stage.polymerase
        if pol is not None:
            arrays = [name for name, _ in population._ALL_AGENT_ARRAYS]
            assert {pol.slots, pol.count, pol.molecules} <= set(arrays)
    assert [s.polymerase for s in STOCHASTIC_STAGES if s.polymerase] == list(population.POLYMERASES)[::-1]


def test_the_stages_stand_in_step_order():
    assert [s.engine for s in STOCHASTIC_STAGES] == ['_tx', '_tl', '_deg', '_ssa']
    assert [s.label for s in STOCHASTIC_STAGES] == ['transcription', 'translation', 'degradation', 'stochastic']
    # the statements of _finish_step that launch a stage (a line that begins with the call), in order
    launched = re.findall(r'^\s*self\.(_\w+)\.step\(', inspect.getsource(Colony._finish_step), flags=re.M)
    assert [e for e in launched if e != '_flag_expression'] == [s.engine for s in STOCHASTIC_STAGES]


# the wording of every stage's status bits as it stood before the table: (label, {bit: text})
OLD_TL = {1: 'ribosome list full', 2: 'key outside [0, 2**31)', 4: 'propensity not finite',
          8: 'a count would pass 2**31 - 1', 16: 'max_events reached'}
OLD_TX = {**OLD_TL, 1: 'RNAP list full'}
STAGE_BITS = {'_ssa': ('stochastic', native.VK_SSA_OVERFLOW, 'a count would pass 2**31 - 1'),
              '_tl': ('translation', native.VK_TL_SLOTS_FULL, 'ribosome list full'),
              '_tx': ('transcription', native.VK_TX_SLOTS_FULL, 'RNAP list full'),
              '_deg': ('degradation', native.VK_DEG_NONFINITE, 'mmol_to_counts not finite and > 0, or a level not finite')}


@pytest.mark.parametrize('engine', ['_ssa', '_tl', '_tx', '_deg'])
def test_ssa_check_names_the_stage_and_the_bit(engine):
    """A bit in one stage's status word, on an object that has every stage: the label and the
    description are that stage's, and the first agent with a bit is named."""
    col = _plain_colony(4, 6)
    for stage in STOCHASTIC_STAGES:
        setattr(col, stage.engine, object())
        setattr(col, stage.status, torch.zeros(6, dtype=torch.int32))
    label, bit, text = STAGE_BITS[engine]
    stage, = [s for s in STOCHASTIC_STAGES if s.engine == engine]
    getattr(col, stage.status)[2] = bit
    getattr(col, stage.status)[5] = bit                  # beyond n: not an agent
    with pytest.raises(FloatingPointError) as err:
        col._ssa_check()
    assert str(err.value) == 'agent 2: %s step status %d (%s)' % (label, bit, text)
    getattr(col, stage.status)[2] = 0
    col._ssa_check()                                     # columns >= n are not read


def test_ssa_check_reports_the_network_first_and_needs_the_network():
    col = _plain_colony(4, 6)
    for stage in STOCHASTIC_STAGES:
        setattr(col, stage.engine, object())
        setattr(col, stage.status, torch.full((6,), 16, dtype=torch.int32))
    order = []
    for _ in STOCHASTIC_STAGES:
        with pytest.raises(FloatingPointError) as err:
            col._ssa_check()
        label = str(err.value).split(': ')[1].split(' step status')[0]
        order.append(label)
        stage, = [s for s in STOCHASTIC_STAGES if s.label == label]
        getattr(col, stage.status).zero_()
    assert order == ['stochastic', 'translation', 'transcription', 'degradation']
    col._tl_status[0] = 1
    col._ssa = None
    col._ssa_check()                                     # no network: nothing is read


def test_describe_status_equals_the_two_old_tables():
    from lens_amd import transcription, translation
    for bits in range(32):
        for old, what, module in ((OLD_TL, 'ribosome', translation), (OLD_TX, 'RNAP', transcription)):
            want = ', '.join(text for bit, text in old.items() if bits & bit) or 'ok'
            assert polymerize.describe_status(bits, what) == want == module.describe_status(bits)
            assert dict(module.STATUS_NAMES) == old
    assert (native.VK_TL_SLOTS_FULL, native.VK_TL_BAD_KEY, native.VK_TL_NONFINITE, native.VK_TL_OVERFLOW,
            native.VK_TL_MAX_EVENTS) == (1, 2, 4, 8, 16)


@pytest.mark.parametrize('pad', [False, True])
@pytest.mark.parametrize('edge', [False, True])
def test_whole_plane(pad, edge):
    lat = SimpleNamespace(pad_top=0, pad_bot=2 if pad else 0, edge_top=True, edge_bot=edge)
    assert whole_plane(lat) is (edge and not pad)
    lat = SimpleNamespace(pad_top=2 if pad else 0, pad_bot=0, edge_top=edge, edge_bot=True)
    assert whole_plane(lat) is (edge and not pad)
