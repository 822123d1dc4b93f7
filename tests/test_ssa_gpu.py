"""The batched Gillespie step on the device (vk_ssa_step, vk_ssa_propensities,
vk_divide_counts, vk_ssa_flagella_target) against the NumPy restatement tests/ssa_ref.py,
which takes the same Philox draws.

Propensities are compared bitwise: both sides do the same FP64 multiplies in the same order
(-ffp-contract=off on the device, NumPy's IEEE multiplies on the host; a NaN matches a NaN).
Counts, events and status are compared as integers.  The one operation the two sides do not
share bit for bit is log(): a last-bit difference in tau can flip `t + tau > T` only for an
agent whose restated |t + tau - T| / T is tiny, so agents whose margin fell below 1e-9 would
be left out (at most 1 % of them, asserted).  The seed of the cases (ssa_ref.CASE_SEED) was
chosen on the CPU so that NO agent of any case is left out, which is asserted too.

Shapes: n in {1, 63, 64, 65, 257} with ld = n + 7 -- one lane, one short of a wave, a wave,
one more, several workgroups with a ragged last one."""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import ssa_ref as sref
from test_ssa_host import BURST_END, birth_death_moments

pytestmark = pytest.mark.gpu

NETS = ('fixture', 'birth_death', 'limits')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lens_amd import native
    native.load()
    return torch.device('cuda', 0)


def _engine(model, dev):
    from lens_amd.stochastic import StochasticEngine
    return StochasticEngine(model, dev)


def _run(dev, model, x0, keys, n, duration, steps, max_events=None, step0=0):
    """The device twin of ssa_ref.trajectory: [(x, events, status)] per step."""
    eng = _engine(model, dev)
    x = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.int32)).to(dev)
    k = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.int64)).to(dev)
    ld = x.shape[1]
    counter = torch.tensor([step0], dtype=torch.int64, device=dev)
    events = torch.full((ld,), -7, dtype=torch.int32, device=dev)
    status = torch.zeros(ld, dtype=torch.int32, device=dev)
    out = []
    for _ in range(steps):
        eng.step(duration, x, k, n, events=events, status=status, step_counter=counter, max_events=max_events)
        out.append((x.cpu().numpy().copy(), events.cpu().numpy().copy(), status.cpu().numpy().copy()))
    assert int(counter.item()) == step0 + steps          # the launch advances the step word
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.int64) == b.view(np.int64)) | nan))


@pytest.mark.parametrize('n', sref.SIZES)
@pytest.mark.parametrize('net', NETS)
def test_propensities_bitwise(dev, net, n):
    model, x0, keys, _, _ = sref.step_case(net, n)
    eng = _engine(model, dev)
    x = torch.from_numpy(x0).to(dev)
    out = torch.full((model.n_reactions, x0.shape[1]), -3.0, dtype=torch.float64, device=dev)
    eng.propensities(x, n, out=out)
    got = out.cpu().numpy()
    want = sref.propensities(model, x0[:, :n])
    assert _same_bits(got[:, :n], want), np.abs(got[:, :n] - want).max()
    assert np.all(got[:, n:] == -3.0)                    # columns past n are not written
    assert np.isfinite(want).all() and (want > 0).any()


def test_choose_limits_on_the_device(dev):
    """C(1000, 120) is finite, C(100000, 120) is inf, as multiplied out."""
    model = sref.fixture_model()
    x0 = np.zeros((model.n_species, 2), dtype=np.int32)
    x0[model.index('flgE')] = [1000, 100000]
    got = _engine(model, dev).propensities(torch.from_numpy(x0).to(dev)).cpu().numpy()
    hook = model.reactions.index('flagellar hook reaction')
    assert _same_bits(got, sref.propensities(model, x0))
    assert np.isfinite(got[hook, 0]) and got[hook, 0] > 1e150 and np.isinf(got[hook, 1])


@pytest.mark.parametrize('n', sref.SIZES)
@pytest.mark.parametrize('net', NETS)
def test_step_equals_the_restatement(dev, net, n):
    model, x0, keys, duration, max_events = sref.step_case(net, n)
    want, out = sref.trajectory(model, x0, keys, n, duration, 3, max_events)
    assert out.sum() <= 0.01 * n                         # the cap on agents left out ...
    assert not out.any()                                 # ... and with this seed there is none
    keep = ~out
    got = _run(dev, model, x0, keys, n, duration, 3, max_events)
    fired = 0
    for k, ((gx, ge, gs), (wx, we, ws)) in enumerate(zip(got, want)):
        assert np.array_equal(ge[:n][keep], we[keep]), (net, n, k)
        assert np.array_equal(gx[:, :n][:, keep], wx[:, :n][:, keep]), (net, n, k)
        assert np.array_equal(gs[:n][keep], ws[keep]), (net, n, k)
        assert np.all(gx[:, n:] == 7) and np.all(ge[n:] == -7) and not gs[n:].any()     # past n: untouched
        fired += int(we.sum())
    assert fired >= 20 * n
    if net == 'limits':
        assert np.all(want[-1][2] == sref.MAX_EVENTS)     # stopped at 20 events in every step
    else:
        assert not want[-1][2].any()


def test_burst_end_state(dev):
    """1000 of every monomer: 573 events, the end state that does not depend on the draws,
    then nothing in the next two steps."""
    n = 65
    model = sref.fixture_model(1000, seed=3)
    x0 = model.initial_counts(n, n + 7)
    keys = np.arange(n + 7, dtype=np.int64)
    got = _run(dev, model, x0, keys, n, 1.0, 3)
    x, events, status = got[0]
    assert events[:n].tolist() == [573] * n and not status.any()
    for name, value in BURST_END.items():
        assert x[model.index(name), :n].tolist() == [value] * n, name
    for k in (1, 2):
        assert not got[k][1][:n].any() and np.array_equal(got[k][0], x) and not got[k][2].any()


def test_status_max_events(dev):
    """max_events = 10 on the burst; the agents beside them (no monomers) are not affected."""
    n = 70
    model = sref.fixture_model(1000, seed=4)
    x0 = model.initial_counts(n, n)
    x0[:, 1::2] = 0
    keys = np.arange(n, dtype=np.int64)
    (x, events, status), = _run(dev, model, x0, keys, n, 1.0, 1, max_events=10)
    (wx, we, ws), = sref.trajectory(model, x0, keys, n, 1.0, 1, 10)[0]
    assert events[0::2].tolist() == [10] * 35 and status[0::2].tolist() == [sref.MAX_EVENTS] * 35
    assert not events[1::2].any() and not status[1::2].any() and not x[:, 1::2].any()
    assert np.array_equal(x, wx) and np.array_equal(events, we) and np.array_equal(status, ws)


def test_status_nonfinite(dev):
    """Monomers at 100000: C(100000, 120) is inf, the agent stops with her counts as they
    were; her neighbours run the burst."""
    n = 66
    model = sref.fixture_model(1000, seed=5)
    x0 = model.initial_counts(n, n)
    x0[:len(sref.load_fixture()['monomer_ids']), 7] = 100000
    keys = np.arange(n, dtype=np.int64)
    (x, events, status), = _run(dev, model, x0, keys, n, 1.0, 1)
    others = np.arange(n) != 7
    assert status[7] == sref.NONFINITE and events[7] == 0 and np.array_equal(x[:, 7], x0[:, 7])
    assert not status[others].any() and events[others].tolist() == [573] * (n - 1)
    (wx, we, ws), = sref.trajectory(model, x0, keys, n, 1.0, 1)[0]
    assert np.array_equal(x, wx) and np.array_equal(status, ws)


def test_status_overflow(dev):
    """A count two below INT32_MAX on a birth reaction: two births fire, the third would
    pass INT32_MAX and is not fired; the other agents go on."""
    n = 65
    model = sref.birth_model(seed=6)
    x0 = np.full((1, n), 5, dtype=np.int32)
    x0[0, 64] = 2 ** 31 - 3
    keys = np.arange(n, dtype=np.int64)
    (x, events, status), = _run(dev, model, x0, keys, n, 1.0, 1)
    assert status[64] == sref.OVERFLOW and events[64] == 2 and x[0, 64] == 2 ** 31 - 1
    assert not status[:64].any() and np.array_equal(x[0, :64], 5 + events[:64]) and events[:64].min() > 20
    (wx, we, ws), = sref.trajectory(model, x0, keys, n, 1.0, 1)[0]
    assert np.array_equal(x, wx) and np.array_equal(events, we) and np.array_equal(status, ws)


def test_status_bad_key_and_sticky_bits(dev):
    """A key outside [0, 2**31) is flagged and the agent not stepped; bits stay set."""
    model = sref.birth_death_model(seed=7)
    x0 = np.zeros((1, 3), dtype=np.int32)
    keys = np.array([5, 2 ** 31, -1], dtype=np.int64)
    got = _run(dev, model, x0, keys, 3, 1.0, 2)
    for x, events, status in got:
        assert status.tolist() == [0, sref.BAD_KEY, sref.BAD_KEY] and events[1:].tolist() == [0, 0]
        assert x[0, 0] > 0 and not x[0, 1:].any()


def test_bad_arguments_and_empty_launch(dev):
    from lens_amd import native
    model = sref.birth_death_model()
    eng = _engine(model, dev)
    x = torch.zeros((1, 8), dtype=torch.int32, device=dev)
    keys = torch.arange(8, dtype=torch.int64, device=dev)
    ev = torch.zeros(8, dtype=torch.int32, device=dev)
    st = torch.zeros(8, dtype=torch.int32, device=dev)
    out = torch.zeros((2, 8), dtype=torch.float64, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    s = native.stream_handle()

    def step(net, n=4, ld=8, duration=1.0, max_events=100, counter=counter, x=x):
        return native._lib.vk_ssa_step(ctypes.byref(net), n, ld, duration, native.ptr(x), native.ptr(keys), 0,
                                       native.ptr(counter), max_events, native.ptr(ev), native.ptr(st), s)

    def prop(net, n=4, ld=8):
        return native._lib.vk_ssa_propensities(ctypes.byref(net), n, ld, native.ptr(x), native.ptr(out), s)

    def net(**fields):
        d = eng.net()
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    for bad in (net(n_species=65), net(n_species=0), net(n_reactions=33), net(n_reactions=0), net(max_order=256),
                net(max_order=200, n_inv=100), net(rates=None), net(stoich_ptr=None)):
        assert step(bad) == native.VK_ERR_ARG and prop(bad) == native.VK_ERR_ARG
    assert step(net(), n=9) == native.VK_ERR_ARG and prop(net(), n=9) == native.VK_ERR_ARG      # n > ld
    assert step(net(), n=-1) == native.VK_ERR_ARG
    assert step(net(), max_events=0) == native.VK_ERR_ARG
    assert step(net(), duration=float('nan')) == native.VK_ERR_ARG
    assert step(net(), duration=-1.0) == native.VK_ERR_ARG
    assert step(net(), counter=None) == native.VK_ERR_ARG
    assert step(net(), x=None) == native.VK_ERR_ARG
    assert b'vk_ssa_step' in native._lib.vk_last_error()
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and not ev.any() and not x.any()       # refused calls launched nothing
    assert step(net(), n=0) == native.VK_OK and prop(net(), n=0) == native.VK_OK
    assert step(net(), n=0, x=None) == native.VK_OK
    torch.cuda.synchronize()
    assert int(counter.item()) == 2 and not x.any()                        # the step word counts steps
    # the host checks of the engine
    with pytest.raises(ValueError):
        eng.step(1.0, x, keys, 9)
    with pytest.raises(ValueError):
        eng.step(1.0, x.to(torch.int64), keys, 4)
    with pytest.raises(ValueError):
        eng.step(1.0, x, keys.to(torch.int32), 4)
    with pytest.raises(ValueError):
        eng.propensities(torch.zeros((2, 8), dtype=torch.int32, device=dev))
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    assert native._lib.vk_ssa_flagella_target(4, native.ptr(ev), native.ptr(ev), 0, s) == native.VK_ERR_ARG
    assert native._lib.vk_ssa_flagella_target(0, 0, 0, native.ptr(bad), s) == native.VK_OK
    assert native._lib.vk_divide_counts(4, 5, 4, native.ptr(ev), native.ptr(ev), native.ptr(x), 8, native.ptr(keys),
                                        native.ptr(x), 8, native.ptr(keys), 1, 0, 0, 0, s) == native.VK_ERR_ARG
    assert native._lib.vk_divide_counts(4, 2, 4, native.ptr(ev), native.ptr(ev), native.ptr(x), 8, native.ptr(keys),
                                        native.ptr(x), 8, native.ptr(keys), 1, 0, 0, 2 ** 31, s) == native.VK_ERR_ARG
    assert native._lib.vk_divide_counts(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, s) == native.VK_OK


def test_storage_independence(dev):
    """Permuting the agents' columns, carrying their keys, permutes the results."""
    n = 130
    model, x0, keys, duration, _ = sref.step_case('fixture', n)
    perm = np.random.default_rng(9).permutation(n)
    a = _run(dev, model, x0[:, :n], keys[:n], n, duration, 2)
    b = _run(dev, model, x0[:, :n][:, perm], keys[:n][perm], n, duration, 2)
    for (ax, ae, as_), (bx, be, bs) in zip(a, b):
        assert np.array_equal(ax[:, perm], bx) and np.array_equal(ae[perm], be) and np.array_equal(as_[perm], bs)
    assert a[0][1].sum() > 20 * n


def _divide(dev, x, keys, src, kind, n_keep, seed, step, key_base, ld_dst):
    from lens_amd.stochastic import divide_counts
    xs = torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    ks = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.int64)).to(dev)
    n_out = len(src)
    xd = torch.full((x.shape[0], ld_dst), -9, dtype=torch.int32, device=dev)
    kd = torch.full((ld_dst,), -9, dtype=torch.int64, device=dev)
    divide_counts(n_out, n_keep, x.shape[1], torch.tensor(src, dtype=torch.int32, device=dev),
                  torch.tensor(kind, dtype=torch.int32, device=dev), xs, ks, xd, kd, seed, step, key_base)
    return xd.cpu().numpy(), kd.cpu().numpy()


def test_divide_counts(dev):
    """A plan with survivors, mothers and removed agents, more than one workgroup."""
    rng = np.random.default_rng(5)
    S, n = 37, 300
    x = rng.integers(0, 2000, (S, n)).astype(np.int32)
    x[:, 3] = 1                                          # every species odd: 37 coins of one mother
    keys = rng.choice(2 ** 31, size=n, replace=False).astype(np.int64)
    role = rng.choice(3, size=n, p=[0.6, 0.3, 0.1])      # survivor, mother, removed
    role[3] = 1
    keep = np.nonzero(role == 0)[0].tolist()
    mothers = np.nonzero(role == 1)[0].tolist()
    src = keep + [a for m in mothers for a in (m, m)]
    kind = [-1] * len(keep) + [0, 1] * len(mothers)
    n_out = len(src)
    assert n_out > 256 and len(keep) + len(mothers) < n
    want_x, want_k = sref.divide_counts(x, keys, src, kind, len(keep), 77, 4, 1000)
    got_x, got_k = _divide(dev, x, keys, src, kind, len(keep), 77, 4, 1000, n_out + 5)
    assert np.array_equal(got_x[:, :n_out], want_x) and np.array_equal(got_k[:n_out], want_k)
    assert np.all(got_x[:, n_out:] == -9) and np.all(got_k[n_out:] == -9)
    d0, d1 = got_x[:, len(keep)::2][:, :len(mothers)], got_x[:, len(keep) + 1:n_out:2]
    assert np.array_equal(d0 + d1, x[:, mothers]) and np.abs(d0 - d1).max() == 1
    i = mothers.index(3)
    assert 0 < d0[:, i].sum() < S                        # her coins fell both ways
    # another step word, another seed: other coins
    other, _ = _divide(dev, x, keys, src, kind, len(keep), 77, 5, 1000, n_out)
    assert not np.array_equal(other, got_x[:, :n_out])


def test_divide_one_agent(dev):
    x = np.array([[7], [0], [2 ** 31 - 1]], dtype=np.int32)
    got_x, got_k = _divide(dev, x, np.array([41]), [0, 0], [0, 1], 0, 1, 2, 10, 2)
    want_x, want_k = sref.divide_counts(x, np.array([41]), [0, 0], [0, 1], 0, 1, 2, 10)
    assert np.array_equal(got_x, want_x) and got_k.tolist() == [10, 11] == want_k.tolist()
    assert sorted(got_x[0].tolist()) == [3, 4] and got_x[1].tolist() == [0, 0]
    assert sorted(got_x[2].tolist()) == [2 ** 30 - 1, 2 ** 30]


@pytest.mark.parametrize('n', [1, 65, 300])
def test_flagella_target(dev, n):
    from lens_amd.stochastic import flagella_target
    row = (np.arange(n) % 33).astype(np.int32)           # 0..32: no flag
    r = torch.from_numpy(row).to(dev)
    target = torch.full((n + 3,), -7, dtype=torch.int32, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    flagella_target(n, r, target, flags)
    want, flag = sref.flagella_target(row)
    assert np.array_equal(target.cpu().numpy()[:n], want) and not flag and int(flags.item()) == 0
    assert np.all(target.cpu().numpy()[n:] == -7)
    for value, clamped in ((33, 32), (-1, 0), (2 ** 31 - 1, 32)):
        row[n - 1] = value
        flags.zero_()
        flagella_target(n, torch.from_numpy(row).to(dev), target, flags)
        assert int(target[n - 1].item()) == clamped == sref.flagella_target(row)[0][n - 1]
        assert int(flags.item()) == 1 and sref.flagella_target(row)[1]
    row[n - 1] = 0
    flagella_target(n, torch.from_numpy(row).to(dev), target, flags)
    assert int(flags.item()) == 1                        # never cleared by the kernel


def test_birth_death_moments_on_the_device(dev):
    model = sref.birth_death_model(seed=2027)
    n = 4096
    got = _run(dev, model, np.zeros((1, n), dtype=np.int32), np.arange(n, dtype=np.int64), n, 1.0, 20)
    assert not got[-1][2].any()
    birth_death_moments(got[-1][0][0])
