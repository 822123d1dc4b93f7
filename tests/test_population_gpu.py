"""lens_amd/population.py on the device: a plan that divides and removes at once, applied to a
stochastic colony with cells (and to one with translation), and the captured graph's guard
after an install that keeps the capacity.

The plan: 37 agents in a capacity of 44; five mothers (3, 11, 12, 25, 36) and five removed
(0, 11, 18, 30, 31) -- the first agent, the last one, and agent 11 who is both and leaves no
daughters: 36 agents after it, 8 of them daughters.  The plan comes from
population.plan_population and is compared with tests/mother_machine_ref.py's; ``ssa`` /
``ssa_key``, the ribosome lists and the pools are compared as integers with the restated
dividers over that plan (tests/ssa_ref.py, tests/translation_ref.py), every array with a
vk_divide_gather mode with the mode restated in NumPy, the lineage and the locations with
their kernels launched over the restated plan."""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import mother_machine_ref as mref
import ssa_ref as sref
import translation_ref as tref
from test_translation_colony_gpu import _colony, _models

pytestmark = pytest.mark.gpu

N, CAP = 37, 44
MOTHERS, REMOVED = (3, 11, 12, 25, N - 1), (0, 11, 18, 30, 31)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lens_amd import native
    native.load()
    return torch.device('cuda', 0)


def _by_mode(old, mode, src, kind):
    """A vk_divide_gather mode over a plan: set copies, split halves and zero clears the daughters'."""
    from lens_amd import native
    out = old[..., src]
    if mode == native.VK_DIVIDE_SPLIT:
        out[..., kind >= 0] = out[..., kind >= 0] / 2
    elif mode == native.VK_DIVIDE_ZERO:
        out[..., kind >= 0] = 0
    else:
        assert mode == native.VK_DIVIDE_SET
    return out


@pytest.mark.parametrize('translation', [False, True])
def test_a_plan_that_divides_and_removes(dev, translation):
    from lens_amd import native, population
    sm, tm = _models()
    col = _colony(dev, sm, tm if translation else None, capacity=CAP, n=N)
    for _ in range(3):
        col.step(1.0)                                    # fluxes, counts, bound ribosomes: every array is set
    n, step, key_base = col.n, col.step_index, col._ssa_key_base
    assert (n, col.ld, step, key_base) == (N, CAP, 3, N)
    names = col.agent_array_names()
    old = {name: getattr(col, name).clone() for name in names}
    host = {name: t.cpu().numpy() for name, t in old.items()}
    lists = col.ribosomes() if translation else None
    assert not translation or sum(len(l) for l in lists) > 0
    divide, remove = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    divide[list(MOTHERS)], remove[list(REMOVED)] = 1, 1
    src, kind, n_out = mref.plan(divide, remove, n)
    assert n_out == 36 and int((kind >= 0).sum()) == 8

    plan = population.plan_population(n, torch.from_numpy(divide).to(dev), torch.from_numpy(remove).to(dev), dev)
    assert (plan.n_src, plan.n_out, plan.n_removed, plan.n_daughters, plan.n_keep) == (n, 36, 5, 8, 28)
    assert np.array_equal(plan.src[:n_out].cpu().numpy(), src) and np.array_equal(plan.kind[:n_out].cpu().numpy(), kind)
    layout = col._layout
    population.regather(col, plan)
    torch.cuda.synchronize()
    assert (col.n, col.ld) == (n_out, CAP) and col._layout > layout and col.agent_array_names() == names

    # the stochastic arrays and the key base, as integers
    keys = host['ssa_key'][:n]
    want_x, want_keys = sref.divide_counts(host['ssa'][:, :n], keys, src, kind, plan.n_keep, sm.seed, step, key_base)
    assert np.array_equal(col.ssa[:, :n_out].cpu().numpy(), want_x)
    assert np.array_equal(col.ssa_key[:n_out].cpu().numpy(), want_keys)
    assert col._ssa_key_base == key_base + 8 and len(set(want_keys.tolist())) == n_out
    if translation:
        want = tref.divide_ribosomes([[list(r) for r in l] for l in lists], keys, src, kind, tm.seed, step)
        assert col.ribosomes() == [[tuple(r) for r in l] for l in want]
        want_mol, _ = sref.divide_counts(host['tl_molecules'][:, :n], keys, src, kind, plan.n_keep,
                                         tm.seed ^ native.VK_TL_DIVIDE_DOMAIN, step, key_base)
        assert np.array_equal(col.tl_molecules[:, :n_out].cpu().numpy(), want_mol)

    # every array with a plain mode
    checked = {'ssa', 'ssa_key', 'ribosome_slots', 'ribosome_count', 'tl_molecules'}
    for name, divider in population._ALL_AGENT_ARRAYS:
        if name not in old or isinstance(divider, str):
            continue
        ranges = ((0, None, divider),) if isinstance(divider, int) else divider
        got = getattr(col, name)[..., :n_out].cpu().numpy()
        assert got.dtype == host[name].dtype
        for lo, hi, mode in ranges:
            rows = slice(None) if host[name].ndim == 1 else slice(lo, hi)
            assert np.array_equal(got[rows], _by_mode(host[name][rows], mode, src, kind)), (name, lo)
        checked.add(name)

    # the lineage and the locations: their kernels over the restated plan
    st, i32 = native.stream_handle(), lambda a: torch.from_numpy(a).to(dev)
    src_dev, kind_dev = i32(src), i32(kind)
    plan_args = (n_out, native.ptr(src_dev), native.ptr(kind_dev))
    lineage = ('lin_root', 'lin_depth', 'lin_path')
    want_lin = [torch.zeros_like(old[name]) for name in lineage]
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    native.check(native._lib.vk_divide_lineage(*plan_args, *[native.ptr(old[name]) for name in lineage],
                                               *map(native.ptr, want_lin), native.ptr(overflow), st), 'lineage')
    for name, want in zip(lineage, want_lin):
        assert torch.equal(getattr(col, name)[:n_out], want[:n_out]), name
    want_loc = torch.zeros_like(old['location'])
    native.check(native._lib.vk_divide_locations(*plan_args, native.ptr(old['location']), CAP, native.ptr(want_loc),
                                                 CAP, native.ptr(col.cell), st), 'locations')
    assert torch.equal(col.location[:, :n_out], want_loc[:, :n_out]) and int(overflow.item()) == 0
    daughters = np.nonzero(kind >= 0)[0]
    assert not np.array_equal(col.location[:, daughters].cpu().numpy(), host['location'][:, src[daughters]])
    assert set(names) <= checked | set(lineage) | {'location'}          # nothing went unchecked

    # the bins follow the new places, and the colony steps on
    lin, ix = col.lattice.bin_sites(col.location, col.n)
    assert torch.equal(lin[:n_out], col.bin_lin[:n_out]) and torch.equal(ix[:n_out], col.bin_ix[:n_out])
    ids = col.agent_ids()
    assert len(set(ids)) == n_out and 'c11.' not in ids and 'c11.0' not in ids and 'c3.0' in ids and 'c36.1' in ids
    col.step(1.0)
    col.check_status()


def test_replay_after_an_install_at_the_same_capacity_raises(dev):
    """install_agents replaces every buffer the graph holds; ``n`` and ``ld`` stay, the layout
    word moves, and the replay refuses before it launches anything."""
    from lens_amd import configs
    from lens_amd.colony import Colony
    from lens_amd.distributed import install_agents, take_agents
    col = Colony(configs.glc_lct_config(), 64, capacity=64, device=dev, integrator='dopri5', environment='held')
    col.step(1.0)
    replay = col.capture(1.0, 1)
    replay()
    torch.cuda.synchronize()
    names = col.agent_array_names()
    old = {name: getattr(col, name) for name in names}
    copies = {name: t.clone() for name, t in old.items()}
    every = torch.arange(64, device=dev)
    install_agents(col, names, {name: take_agents(col, name, every) for name in names})
    assert (col.n, col.ld) == (64, 64)
    assert all(getattr(col, name).data_ptr() != old[name].data_ptr() for name in names)
    time, index = col.time, col.step_index
    with pytest.raises(RuntimeError, match='re-laid out'):
        replay()
    torch.cuda.synchronize()
    assert (col.time, col.step_index) == (time, index)
    for name in names:                                   # neither the new nor the old buffers were written
        assert torch.equal(getattr(col, name), copies[name]) and torch.equal(old[name], copies[name]), name
    col.capture(1.0, 1)()                                # captured again, it replays
    torch.cuda.synchronize()
    assert col.step_index == index + 1 and not torch.equal(col.conc, copies['conc'])
    col.check_status()
