"""The translation step on the device (vk_translation_step, vk_divide_ribosomes) against the
restatement tests/translation_ref.py, which takes the same Philox draws.

Lists, counts, monomers, events and status are compared as integers.  The one operation the
two sides do not share bit for bit is log(): a last-bit difference in tau can flip
`t + tau > interval` only where the restated |t + tau - interval| is tiny.  "No agent is left
out" is a condition, not a measurement: the seed of the cases (translation_ref.CASE_SEED =
20261021) was chosen on the CPU so that every |t + tau - interval| and every
|cum_i - u2 * total| / total of every case stays above 1e-9, which is asserted here; the
smallest the cases meet are 6.44e-6 (time; n = 257, either release) and 7.32e-5 (choice;
n = 64, either release).

Shapes: n in {1, 63, 64, 65, 257} with ld = n + 7; 3 templates of 3, 12 and 5 residues on 2
operons, 4 monomers; neighbouring lanes hold lists of length 0, 1, capacity - 1 and capacity."""

import copy
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import translation_ref as tref

pytestmark = pytest.mark.gpu

CAP = 8


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lens_amd import native
    native.load()
    return torch.device('cuda', 0)


def _engine(model, sm, dev):
    from lens_amd.translation import TranslationEngine
    return TranslationEngine(model, sm, dev)


def _to_dev(dev, model, lists, molecules, counts, keys, stale=-1):
    ld = counts.shape[1]
    slots, length = tref.pack_lists(lists, model.max_ribosomes, ld)
    for a, ribosomes in enumerate(lists):
        slots[len(ribosomes):, a] = stale            # words beyond the length are never read
    put = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return put(slots), put(length), put(molecules.astype(np.int32)), put(counts.astype(np.int32)), put(keys)


def _run(dev, model, sm, lists, molecules, counts, keys, n, dt, steps, step0=0, max_events=None):
    """The device twin of translation_ref.trajectory."""
    eng = _engine(model, sm, dev)
    slots, length, mol, x, k = _to_dev(dev, model, lists, molecules, counts, keys)
    ld = x.shape[1]
    counter = torch.tensor([step0], dtype=torch.int64, device=dev)
    events = torch.full((ld,), -7, dtype=torch.int32, device=dev)
    status = torch.zeros(ld, dtype=torch.int32, device=dev)
    out = []
    for _ in range(steps):
        eng.step(dt, slots, length, mol, x, k, n, events=events, status=status, step_counter=counter,
                 max_events=max_events)
        host = [t.cpu().numpy().copy() for t in (slots, length, mol, x, events, status)]
        out.append((tref.unpack_lists(host[0], host[1], n),) + tuple(host[1:]))
    assert int(counter.item()) == step0 + steps          # the launch advances the step word
    return out


def _compare(got, want, n):
    for k, (g, w) in enumerate(zip(got, want)):
        lists, length, mol, x, events, status = g
        assert lists == w[0], (k, [a for a in range(n) if lists[a] != w[0][a]][:5])
        assert np.array_equal(mol, w[1]), k                  # columns >= n included: they must stay
        assert np.array_equal(x, w[2]), k
        assert np.array_equal(events[:n], w[3]) and np.all(events[n:] == -7), k
        assert np.array_equal(status[:n], w[4]) and np.all(status[n:] == 0), k


@pytest.mark.parametrize('n', tref.SIZES)
def test_deterministic_elongation_bit_for_bit(dev, n):
    """No free ribosome, no transcript and nobody occluding (a release would unbind a transcript
    that is not there): elongation, stalls, completions and the books alone."""
    model, sm, lists, molecules, counts, keys = tref.step_case(n, cap=CAP)
    counts[[tref.SPECIES.index(s) for s in ('o1', 'o2', 'Ribosome')], :n] = 0
    lists = [[[t, p, False] for t, p, _ in ribosomes] for ribosomes in lists]
    ref = copy.deepcopy(lists), molecules.copy(), counts.copy()
    want, _, _ = tref.trajectory(model, model.bind(sm), *ref, keys, 1.0, 2)
    got = _run(dev, model, sm, lists, molecules, counts, keys, n, 1.0, 2)
    _compare(got, want, n)
    assert sum(w[3].sum() for w in want) == 0
    if n >= 63:
        done = want[-1][2][tref.SPECIES.index('Ribosome'), :n]
        assert done.max() > 0 and any(len(l) for l in want[-1][0])       # completions and stalls both happen


@pytest.mark.parametrize('release', ('reference', 'template'))
@pytest.mark.parametrize('n', tref.SIZES)
def test_three_stochastic_steps_equal_the_restatement(dev, n, release):
    model, sm, lists, molecules, counts, keys = tref.step_case(n, release, cap=CAP)
    ref = copy.deepcopy(lists), molecules.copy(), counts.copy()
    want, margin_t, margin_q = tref.trajectory(model, model.bind(sm), *ref, keys, 1.0, 3, step0=5)
    assert margin_t >= tref.MARGIN and margin_q >= tref.MARGIN          # no agent is left out
    got = _run(dev, model, sm, lists, molecules, counts, keys, n, 1.0, 3, step0=5)
    _compare(got, want, n)
    assert sum(w[3].sum() for w in want) >= 3                            # initiations happened


def _one(dev, model, sm, ribosomes, molecules, counts, key=5, dt=1.0, max_events=None):
    """One agent (ld = 3): the device's and the restatement's (lists, molecules, counts, events, status)."""
    mol = np.zeros((model.n_monomers + 2, 3), dtype=np.int64)
    x = np.zeros((sm.n_species, 3), dtype=np.int64)
    mol[:, 0], x[:, 0] = molecules, counts
    keys = np.array([key, 1, 2], dtype=np.int64)
    l, m2, x2 = [copy.deepcopy(ribosomes)], mol.copy(), x.copy()
    ev, st, _, _ = tref.step(model, model.bind(sm), l, m2, x2, keys, dt, model.seed, 0, max_events=max_events)
    want = [(l, m2, x2, ev, st)]
    got = _run(dev, model, sm, [ribosomes], mol, x, keys, 1, dt, 1, max_events=max_events)
    _compare(got, want, 1)
    return got[0]


def _x(**named):
    x = np.zeros(len(tref.SPECIES), dtype=np.int64)
    for name, value in named.items():
        x[tref.SPECIES.index(name)] = value
    return x


def test_every_status_bit(dev):
    from lens_amd import native
    sm = tref.small_stochastic()
    pools = [50, 50, 50, 50, 1000, 0]
    # a full list and eager transcripts: the initiation is not fired
    model = tref.small_model(max_ribosomes=2, affinities=(50.0, 50.0, 50.0))
    g = _one(dev, model, sm, [[1, 0, True], [1, 1, True]], pools, _x(o1=5, o2=5, Ribosome=5))
    assert g[5][0] == native.VK_TL_SLOTS_FULL and g[4][0] == 0 and len(g[0][0]) == 2
    # a key outside [0, 2**31): not stepped, nothing written
    model = tref.small_model(max_ribosomes=CAP)
    g = _one(dev, model, sm, [[0, 0, True]], pools, _x(o1=5, Ribosome=5), key=2 ** 31)
    assert g[5][0] == native.VK_TL_BAD_KEY and g[0][0] == [[0, 0, True]] and list(g[2][:, 0]) == pools
    g = _one(dev, model, sm, [], pools, _x(o1=5, Ribosome=5), key=-1)
    assert g[5][0] == native.VK_TL_BAD_KEY
    # an infinite propensity
    model = tref.small_model(max_ribosomes=CAP, affinities=(1e308, 1e308, 1e308))
    g = _one(dev, model, sm, [], pools, _x(o1=2 ** 30, o2=2 ** 30, Ribosome=2 ** 30))
    assert g[5][0] == native.VK_TL_NONFINITE and g[4][0] == 0
    # a completion that would take the product past INT32_MAX is not made; the agent stops
    model = tref.small_model(max_ribosomes=CAP)
    g = _one(dev, model, sm, [[0, 2, False], [2, 0, False]], pools, _x(pX=2 ** 31 - 1))
    assert g[5][0] == native.VK_TL_OVERFLOW and g[0][0] == [[0, 2, False], [2, 0, False]]
    assert g[3][tref.SPECIES.index('pX'), 0] == 2 ** 31 - 1 and list(g[2][:, 0]) == pools
    # ADP past INT32_MAX is clamped
    g = _one(dev, model, sm, [[1, 0, False]], [50, 50, 50, 50, 1000, 2 ** 31 - 2], _x())
    assert g[5][0] == native.VK_TL_OVERFLOW and g[2][5, 0] == 2 ** 31 - 1 and g[2][4, 0] == 1000 - 8
    # max_events initiations
    model = tref.small_model(max_ribosomes=CAP, affinities=(0.0, 50.0, 0.0))     # 12 residues: nobody completes
    g = _one(dev, model, sm, [], pools, _x(o1=9, o2=9, Ribosome=9), max_events=2)
    assert g[5][0] == native.VK_TL_MAX_EVENTS and g[4][0] == 2 and len(g[0][0]) == 2
    # the bits are OR-ed in and never cleared
    eng = _engine(model, sm, dev)
    slots, length, mol, x, k = _to_dev(dev, model, [[]], np.zeros((6, 1)), np.zeros((8, 1)), np.array([3]))
    status = torch.full((1,), 64, dtype=torch.int32, device=dev)
    eng.step(1.0, slots, length, mol, x, k, 1, status=status)
    assert int(status[0]) == 64


def test_bad_arguments(dev):
    from lens_amd import native
    model, sm, lists, molecules, counts, keys = tref.step_case(5, cap=CAP)
    eng = _engine(model, sm, dev)
    slots, length, mol, x, k = _to_dev(dev, model, lists, molecules, counts, keys)
    ld = x.shape[1]
    events, status = torch.zeros(ld, dtype=torch.int32, device=dev), torch.zeros(ld, dtype=torch.int32, device=dev)
    lib, st = native._lib, native.stream_handle()

    def call(d=None, n=5, ld_=ld, slots_=slots, counter=eng.step_counter, max_events=10, null=None):
        d = d or eng.table(1.0)
        p = {name: native.ptr(t) for name, t in (('slots', slots_), ('length', length), ('mol', mol), ('x', x),
                                                 ('keys', k), ('events', events), ('status', status))}
        if null:
            p[null] = 0
        return lib.vk_translation_step(ctypes.byref(d), n, ld_, p['slots'], p['length'], p['mol'], p['x'], p['keys'], 1,
                                       native.ptr(counter), 1, max_events, p['events'], p['status'], st)

    assert call() == native.VK_OK
    step_after = int(eng.step_counter.item())
    snap = [t.clone() for t in (slots, length, mol, x)]
    assert call(n=-1) == native.VK_ERR_ARG and call(n=ld + 1) == native.VK_ERR_ARG
    assert call(max_events=0) == native.VK_ERR_ARG and call(counter=None) == native.VK_ERR_ARG
    for null in ('slots', 'length', 'mol', 'x', 'keys', 'events', 'status'):
        assert call(null=null) == native.VK_ERR_ARG, null
    for field, value in (('max_slots', 0), ('max_slots', native.VK_TL_MAX_SLOTS + 1), ('n_templates', 0),
                         ('n_templates', native.VK_TL_MAX_TEMPLATES + 1), ('n_monomers', native.VK_TL_MAX_MONOMERS + 1),
                         ('ribosome_species', 8), ('release', 2), ('affinity', 0), ('seq', 0)):
        d = eng.table(1.0)
        setattr(d, field, value)
        assert call(d=d) == native.VK_ERR_ARG, field
    assert b'vk_translation_step' in lib.vk_last_error()
    torch.cuda.synchronize()
    assert int(eng.step_counter.item()) == step_after                      # a refused call launches nothing
    assert all(torch.equal(a, b) for a, b in zip(snap, (slots, length, mol, x)))
    assert call(n=0) == native.VK_OK and int(eng.step_counter.item()) == step_after + 1    # the step word counts steps
    # the divider
    src = torch.zeros(2, dtype=torch.int32, device=dev)
    dst, dlen = torch.zeros_like(slots), torch.zeros_like(length)
    div = lambda n_out=2, n_src=5, cap=CAP, null=False: lib.vk_divide_ribosomes(
        n_out, n_src, native.ptr(src), native.ptr(src), 0 if null else native.ptr(slots), native.ptr(length), ld,
        native.ptr(k), native.ptr(dst), native.ptr(dlen), ld, cap, 1, 0, st)
    assert div() == native.VK_OK and div(n_out=0, null=True) == native.VK_OK
    assert div(n_out=-1) == native.VK_ERR_ARG and div(n_src=ld + 1) == native.VK_ERR_ARG
    assert div(n_out=ld + 1) == native.VK_ERR_ARG and div(null=True) == native.VK_ERR_ARG
    assert div(cap=0) == native.VK_ERR_ARG and div(cap=native.VK_TL_MAX_SLOTS + 1) == native.VK_ERR_ARG


@pytest.mark.parametrize('n', (65, 257))
def test_storage_independence(dev, n):
    """Permuted columns give the same result per key."""
    model, sm, lists, molecules, counts, keys = tref.step_case(n, cap=CAP)
    got = _run(dev, model, sm, lists, molecules, counts, keys, n, 1.0, 2)
    perm = np.random.default_rng(n).permutation(n)
    full = np.concatenate([perm, np.arange(n, n + 7)])
    again = _run(dev, model, sm, [lists[a] for a in perm], molecules[:, full], counts[:, full], keys[full], n, 1.0, 2)
    for g, h in zip(got, again):
        assert [g[0][a] for a in perm] == h[0]
        for i in (1, 2, 3, 4, 5):
            assert np.array_equal(g[i][..., full], h[i])


@pytest.mark.parametrize('n', (1, 65, 257))
def test_divide_ribosomes(dev, n):
    from lens_amd.translation import divide_ribosomes
    model, sm, lists, molecules, counts, keys = tref.step_case(n, cap=CAP)
    ld = n + 7
    slots, length, _, _, k = _to_dev(dev, model, lists, molecules, counts, keys)
    # every third agent divides, every fifth is removed; the survivors first, the daughters follow
    mothers = [a for a in range(n) if a % 3 == 0]
    keep = [a for a in range(n) if a % 3 and a % 5]
    src = np.array(keep + [a for a in mothers for _ in (0, 1)], dtype=np.int32)
    kind = np.array([-1] * len(keep) + [0, 1] * len(mothers), dtype=np.int32)
    n_out, ld_dst = len(src), len(src) + 3
    dst = torch.full((CAP, ld_dst), -5, dtype=torch.int32, device=dev)
    dlen = torch.full((ld_dst,), -5, dtype=torch.int32, device=dev)
    divide_ribosomes(n_out, n, torch.from_numpy(src).to(dev), torch.from_numpy(kind).to(dev), slots, length, k, dst,
                     dlen, model.seed, 9)
    want = tref.divide_ribosomes(lists, keys, src, kind, model.seed, 9)
    got_slots, got_len = dst.cpu().numpy(), dlen.cpu().numpy()
    assert tref.unpack_lists(got_slots, got_len, n_out) == want
    assert np.all(got_len[n_out:] == -5) and np.all(got_slots[:, n_out:] == -5)
    for j in range(n_out):
        assert np.all(got_slots[got_len[j]:, j] == 0)                     # zeroed beyond the new length
    for i, a in enumerate(mothers):                                       # order kept, nobody lost or doubled
        d0, d1 = want[len(keep) + 2 * i], want[len(keep) + 2 * i + 1]
        assert sorted(map(tuple, d0 + d1)) == sorted(map(tuple, lists[a]))
    if n >= 65:
        assert any(want[len(keep) + 2 * i] and want[len(keep) + 2 * i + 1] for i in range(len(mothers)))


def ragged_wave_case():
    """step_case(65) at ld = 70, a full wave and a wave of one lane, arranged so that the lanes of the
    full wave leave the shared initiation loop at different rounds: two keys outside [0, 2**31), one
    full list that stalls (no monomers) in front of free ribosomes, and max_events = 2.  Returns
    (model, sm, the inputs, the restatement's two steps, its smallest margins)."""
    n, ld = 65, 70
    model, sm, lists, molecules, counts, keys = tref.step_case(n, cap=CAP)
    molecules, counts, keys = molecules[:, :ld].copy(), counts[:, :ld].copy(), keys[:ld].copy()
    keys[3], keys[40] = -1, 2 ** 31
    assert len(lists[7]) == CAP
    molecules[:4, 7] = 0
    counts[[tref.SPECIES.index(s) for s in ('o1', 'o2', 'Ribosome')], 7] = 5
    l, mol, x = copy.deepcopy(lists), molecules.copy(), counts.copy()
    status, want, worst = np.zeros(n, dtype=np.int32), [], np.inf
    for k in range(2):
        events, status, margin_t, margin_q = tref.step(model, model.bind(sm), l, mol, x, keys, 1.0, model.seed, k,
                                                       status, max_events=2)
        worst = min(worst, margin_t.min(), margin_q.min())
        want.append((copy.deepcopy(l), mol.copy(), x.copy(), events.copy(), status.copy()))
    return model, sm, (lists, molecules, counts, keys), want, worst


def test_lanes_leave_the_shared_loop_at_different_rounds(dev):
    """The status tests above run one agent at a time; here the exits of vk_polymerize.h's loop are
    taken per lane under the wave-wide __any, beside neighbours that go on.  Two steps, every array
    bitwise against the restatement, columns >= n included."""
    from lens_amd import native
    model, sm, (lists, molecules, counts, keys), want, worst = ragged_wave_case()
    n = len(lists)
    assert worst >= tref.MARGIN                                          # no agent is left out
    first, last = want[0], want[-1]
    assert [a for a in range(n) if last[4][a] & native.VK_TL_BAD_KEY] == [3, 40]
    assert first[4][7] & native.VK_TL_SLOTS_FULL and len(first[0][7]) == CAP
    stopped = (first[4] & native.VK_TL_MAX_EVENTS) != 0
    assert np.all(first[3][stopped] == 2) and 0 < stopped[:64].sum() < 64 and first[3][:64].min() == 0
    assert len({int(e) for e in first[3][:64]}) == 3                    # lanes that fired 0, 1 and 2 times
    got = _run(dev, model, sm, lists, molecules, counts, keys, n, 1.0, 2, max_events=2)
    _compare(got, want, n)
