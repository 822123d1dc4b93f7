"""The transcription step on the device (vk_transcription_step, and vk_divide_ribosomes under the
transcription seed) against the restatement tests/transcription_ref.py, which takes the same
Philox draws.

Lists, counts, molecules, events and status are compared as integers.  The operations the two
sides do not share bit for bit are log() and nothing else, but four comparisons could flip on a
last-bit difference, so "no agent is left out" is a condition, not a measurement: the seed of the
cases (transcription_ref.CASE_SEED = 20261021, the first tried) was chosen on the CPU so that
every |t + tau - interval|, |cum_q - u2 * total| / total, |choice - strength| / strength_from and
|level - threshold| / threshold of every case stays above 1e-9, which is asserted here.  The
smallest the stochastic cases meet: 4.65e-5 (time; n = 257), 5.89e-4 (promoter choice; n = 257),
2.73e-4 (read-through; n = 257) and 3.58e-4 (level; n = 65).

Shapes: n in {1, 63, 64, 65, 257} with ld = n + 7; the toy chromosome (two promoters of 9 bases,
directions +1 and -1, two terminators each), max_rnaps = 8; neighbouring lanes hold lists of
length 0, 1, capacity - 1 and capacity; mmol_to_counts differs per agent and the factor counts sit
on both sides of both thresholds."""

import copy
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import transcription_ref as xref

pytestmark = pytest.mark.gpu

CAP = 8
DT = xref.TIMESTEP


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lens_amd import native
    native.load()
    return torch.device('cuda', 0)


def _engine(model, sm, dev):
    from lens_amd.transcription import TranscriptionEngine
    return TranscriptionEngine(model, sm, dev)


def _to_dev(dev, model, lists, molecules, counts, m2c, keys, stale=-1):
    ld = counts.shape[1]
    slots, length = xref.pack_lists(lists, model.max_rnaps, ld)
    for a, rnaps in enumerate(lists):
        slots[len(rnaps):, a] = stale                # words beyond the length are never read
    put = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return (put(slots), put(length), put(molecules.astype(np.int32)), put(counts.astype(np.int32)),
            put(np.asarray(m2c, dtype=np.float64)), put(keys))


def _run(dev, model, sm, lists, molecules, counts, m2c, keys, n, dt, steps, step0=0, max_events=None):
    """The device twin of transcription_ref.trajectory."""
    eng = _engine(model, sm, dev)
    slots, length, mol, x, per, k = _to_dev(dev, model, lists, molecules, counts, m2c, keys)
    ld = x.shape[1]
    counter = torch.tensor([step0], dtype=torch.int64, device=dev)
    events = torch.full((ld,), -7, dtype=torch.int32, device=dev)
    status = torch.zeros(ld, dtype=torch.int32, device=dev)
    out = []
    for _ in range(steps):
        eng.step(dt, slots, length, mol, x, per, k, n, events=events, status=status, step_counter=counter,
                 max_events=max_events)
        host = [t.cpu().numpy().copy() for t in (slots, length, mol, x, events, status)]
        out.append((xref.unpack_lists(host[0], host[1], n),) + tuple(host[1:]))
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


@pytest.mark.parametrize('n', xref.SIZES)
def test_deterministic_elongation_bit_for_bit(dev, n):
    """No free RNAP at the start and promoters without affinity, so nothing initiates: elongation,
    stalls, terminations, read-through draws, unocclusion and the books alone."""
    model, sm, lists, molecules, counts, m2c, keys = xref.step_case(n, cap=CAP, free=False, affinity=0.0)
    ref = copy.deepcopy(lists), molecules.copy(), counts.copy()
    want, worst = xref.trajectory(model, model.bind(sm), *ref, m2c, keys, DT, 2)
    assert worst[2] >= xref.MARGIN and worst[3] >= xref.MARGIN
    got = _run(dev, model, sm, lists, molecules, counts, m2c, keys, n, DT, 2)
    _compare(got, want, n)
    assert sum(w[3].sum() for w in want) == 0                # nothing initiates
    if n >= 63:
        done = want[-1][2][xref.SPECIES.index('RNA Polymerase'), :n]
        assert done.max() > 0 and any(len(l) for l in want[-1][0])       # terminations and stalls both happen


@pytest.mark.parametrize('n', xref.SIZES)
def test_three_stochastic_steps_equal_the_restatement(dev, n):
    model, sm, lists, molecules, counts, m2c, keys = xref.step_case(n, cap=CAP)
    ref = copy.deepcopy(lists), molecules.copy(), counts.copy()
    want, worst = xref.trajectory(model, model.bind(sm), *ref, m2c, keys, DT, 3, step0=5)
    print('n = %d margins (time, promoter, read-through, level): %s' % (n, worst))
    assert np.all(worst >= xref.MARGIN)                                  # no agent is left out
    got = _run(dev, model, sm, lists, molecules, counts, m2c, keys, n, DT, 3, step0=5)
    _compare(got, want, n)
    if n >= 63:
        assert sum(w[3].sum() for w in want) >= 3                        # initiations happened
        s = lambda name: want[-1][2][xref.SPECIES.index(name), :n].astype(np.int64) - counts[
            xref.SPECIES.index(name), :n]
        # both read-through outcomes: the short and the long operon of a promoter were both made
        assert s('oA').max() > 0 and s('oAZ').max() > 0 and s('oB').max() > 0 and s('oBY').max() > 0


def _one(dev, model, sm, rnaps, molecules, counts, key=5, dt=DT, m2c=10.0, max_events=None):
    """One agent (ld = 3): the device's and the restatement's (lists, length, molecules, counts, events, status)."""
    mol = np.zeros((len(model.molecule_ids), 3), dtype=np.int64)
    x = np.zeros((sm.n_species, 3), dtype=np.int64)
    mol[:, 0], x[:, 0] = molecules, counts
    keys = np.array([key, 1, 2], dtype=np.int64)
    per = np.full(3, m2c)
    l, m2, x2 = [copy.deepcopy(rnaps)], mol.copy(), x.copy()
    ev, st, _ = xref.step(model, model.bind(sm), l, m2, x2, per, keys, dt, model.seed, 0, max_events=max_events)
    want = [(l, m2, x2, ev, st)]
    got = _run(dev, model, sm, [rnaps], mol, x, per, keys, 1, dt, 1, max_events=max_events)
    _compare(got, want, 1)
    return got[0]


def _x(**named):
    x = np.zeros(len(xref.SPECIES), dtype=np.int64)
    for name, value in named.items():
        x[xref.SPECIES.index(name.replace('_', ' '))] = value
    return x


def test_every_status_bit(dev):
    from lens_amd import native
    sm = xref.toy_stochastic()
    pools = [50, 50, 50, 50, 0]
    # a full list and eager promoters: the initiation is not fired
    model = xref.toy_model(2, affinity=500.0)
    g = _one(dev, model, sm, [[0, 1, 6, False], [1, 1, 7, False]], [0, 0, 0, 0, 0], _x(RNA_Polymerase=5))
    assert g[5][0] == native.VK_TX_SLOTS_FULL and g[4][0] == 0 and len(g[0][0]) == 2
    # a key outside [0, 2**31): not stepped, nothing written
    model = xref.toy_model(CAP)
    g = _one(dev, model, sm, [[0, 0, 0, True]], pools, _x(RNA_Polymerase=5), key=2 ** 31)
    assert g[5][0] == native.VK_TX_BAD_KEY and g[0][0] == [[0, 0, 0, True]] and list(g[2][:, 0]) == pools
    g = _one(dev, model, sm, [], pools, _x(RNA_Polymerase=5), key=-1)
    assert g[5][0] == native.VK_TX_BAD_KEY
    # an infinite propensity
    model = xref.toy_model(CAP, affinity=1e308)
    g = _one(dev, model, sm, [], pools, _x(RNA_Polymerase=2 ** 30))
    assert g[5][0] == native.VK_TX_NONFINITE and g[4][0] == 0
    # a termination that would take the product past INT32_MAX is not made; the agent stops
    model = xref.toy_model(CAP)
    g = _one(dev, model, sm, [[0, 1, 8, False], [1, 1, 7, False]], pools, _x(oAZ=2 ** 31 - 1))
    assert g[5][0] == native.VK_TX_OVERFLOW and g[0][0] == [[0, 1, 8, False], [1, 1, 7, False]]
    assert g[3][xref.SPECIES.index('oAZ'), 0] == 2 ** 31 - 1 and list(g[2][:, 0]) == pools
    # ... and so would the free RNAPs
    g = _one(dev, model, sm, [[1, 1, 8, False]], pools, _x(RNA_Polymerase=2 ** 31 - 1, tfA=100, tfB=100), dt=0.1)
    assert g[5][0] & native.VK_TX_OVERFLOW and g[0][0] == [[1, 1, 8, False]]
    # ADP past INT32_MAX is clamped; ATP goes below zero and is kept
    g = _one(dev, model, sm, [[0, 1, 3, False]], [1, 50, 50, 50, 2 ** 31 - 2], _x())
    assert g[5][0] == native.VK_TX_OVERFLOW and g[2][4, 0] == 2 ** 31 - 1 and g[2][0, 0] < 0
    # max_events initiations
    model = xref.toy_model(CAP, affinity=500.0, polymerase_occlusion=0)
    g = _one(dev, model, sm, [], [0, 0, 0, 0, 0], _x(RNA_Polymerase=9), max_events=2)
    assert g[5][0] == native.VK_TX_MAX_EVENTS and g[4][0] == 2 and len(g[0][0]) == 2
    # the bits are OR-ed in and never cleared
    eng = _engine(model, sm, dev)
    slots, length, mol, x, per, k = _to_dev(dev, model, [[]], np.zeros((5, 1)), np.zeros((8, 1)), np.ones(1),
                                            np.array([3]))
    status = torch.full((1,), 64, dtype=torch.int32, device=dev)
    eng.step(DT, slots, length, mol, x, per, k, 1, status=status)
    assert int(status[0]) == 64


def test_bad_arguments(dev):
    from lens_amd import native
    model, sm, lists, molecules, counts, m2c, keys = xref.step_case(5, cap=CAP)
    eng = _engine(model, sm, dev)
    slots, length, mol, x, per, k = _to_dev(dev, model, lists, molecules, counts, m2c, keys)
    ld = x.shape[1]
    events, status = torch.zeros(ld, dtype=torch.int32, device=dev), torch.zeros(ld, dtype=torch.int32, device=dev)
    lib, st = native._lib, native.stream_handle()

    def call(d=None, n=5, ld_=ld, counter=eng.step_counter, max_events=10, null=None):
        d = d or eng.table(DT)
        p = {name: native.ptr(t) for name, t in (('slots', slots), ('length', length), ('mol', mol), ('x', x),
                                                 ('per', per), ('keys', k), ('events', events), ('status', status))}
        if null:
            p[null] = 0
        return lib.vk_transcription_step(ctypes.byref(d), n, ld_, p['slots'], p['length'], p['mol'], p['x'], p['per'],
                                         p['keys'], 1, native.ptr(counter), 1, max_events, p['events'], p['status'], st)

    assert call() == native.VK_OK
    step_after = int(eng.step_counter.item())
    snap = [t.clone() for t in (slots, length, mol, x)]
    assert call(n=-1) == native.VK_ERR_ARG and call(n=ld + 1) == native.VK_ERR_ARG
    assert call(max_events=0) == native.VK_ERR_ARG and call(counter=None) == native.VK_ERR_ARG
    for null in ('slots', 'length', 'mol', 'x', 'per', 'keys', 'events', 'status'):
        assert call(null=null) == native.VK_ERR_ARG, null
    for field, value in (('max_slots', 0), ('max_slots', native.VK_TX_MAX_SLOTS + 1), ('n_templates', 0),
                         ('n_templates', native.VK_TX_MAX_TEMPLATES + 1), ('n_monomers', native.VK_TX_MAX_MONOMERS + 1),
                         ('n_monomers', 0), ('rnap_species', 8), ('rnap_species', -1), ('n_affinities', 0),
                         ('n_affinities', native.VK_TX_MAX_AFFINITIES + 1), ('atp_row', 5), ('adp_row', 3),
                         ('sequence', 3), ('sequence', -1), ('n_bases', 0), ('n_plan', -1), ('affinity', 0), ('seq', 0), ('seq2', 0),
                         ('term_pos', 0), ('thr_value', 0), ('copy', 0), ('interval', 0)):
        d = eng.table(DT)
        setattr(d, field, value)
        assert call(d=d) == native.VK_ERR_ARG, field
    assert b'vk_transcription_step' in lib.vk_last_error()
    torch.cuda.synchronize()
    assert int(eng.step_counter.item()) == step_after                      # a refused call launches nothing
    assert all(torch.equal(a, b) for a, b in zip(snap, (slots, length, mol, x)))
    assert call(n=0) == native.VK_OK and int(eng.step_counter.item()) == step_after + 1    # the step word counts steps


@pytest.mark.parametrize('n', (65, 257))
def test_storage_independence(dev, n):
    """Permuted columns give the same result per key."""
    model, sm, lists, molecules, counts, m2c, keys = xref.step_case(n, cap=CAP)
    got = _run(dev, model, sm, lists, molecules, counts, m2c, keys, n, DT, 2)
    perm = np.random.default_rng(n).permutation(n)
    full = np.concatenate([perm, np.arange(n, n + 7)])
    again = _run(dev, model, sm, [lists[a] for a in perm], molecules[:, full], counts[:, full], m2c[full], keys[full],
                 n, DT, 2)
    for g, h in zip(got, again):
        assert [g[0][a] for a in perm] == h[0]
        for i in (1, 2, 3, 4, 5):
            assert np.array_equal(g[i][..., full], h[i])


def test_global_sequence_path_equals_the_lds_path(dev):
    """sequence_path='global' forces the global byte table of the sequence, 'lds' the staged words (which
    'auto' takes too for the toy's 18 bases: they cost no occupancy): same outputs."""
    n = 65
    model, sm, lists, molecules, counts, m2c, keys = xref.step_case(n, cap=CAP)
    other, staged = (xref.step_case(n, cap=CAP, sequence_path=s)[0] for s in ('global', 'lds'))
    assert (model.sequence_path, other.sequence_path, staged.sequence_path) == ('auto', 'global', 'lds')
    got = _run(dev, model, sm, lists, molecules, counts, m2c, keys, n, DT, 2)
    again = _run(dev, other, sm, lists, molecules, counts, m2c, keys, n, DT, 2)
    third = _run(dev, staged, sm, lists, molecules, counts, m2c, keys, n, DT, 2)
    for g, h, s in zip(got, again, third):
        assert g[0] == h[0] == s[0]
        for i in (1, 2, 3, 4, 5):
            assert np.array_equal(g[i], h[i]) and np.array_equal(g[i], s[i])
    want, _ = xref.trajectory(other, other.bind(sm), copy.deepcopy(lists), molecules.copy(), counts.copy(), m2c, keys,
                              DT, 2)
    _compare(again, want, n)


@pytest.mark.parametrize('n', (1, 65, 257))
def test_divide_rnaps(dev, n):
    """The RNAP lists through vk_divide_ribosomes with the transcription seed, against the restated coins."""
    from lens_amd.transcription import divide_rnaps
    from lens_amd.translation import divide_ribosomes
    model, sm, lists, molecules, counts, m2c, keys = xref.step_case(n, cap=CAP)
    slots, length, _, _, _, k = _to_dev(dev, model, lists, molecules, counts, m2c, keys)
    # every third agent divides, every fifth is removed; the survivors first, the daughters follow
    mothers = [a for a in range(n) if a % 3 == 0]
    keep = [a for a in range(n) if a % 3 and a % 5]
    src = np.array(keep + [a for a in mothers for _ in (0, 1)], dtype=np.int32)
    kind = np.array([-1] * len(keep) + [0, 1] * len(mothers), dtype=np.int32)
    n_out, ld_dst = len(src), len(src) + 3
    dst = torch.full((CAP, ld_dst), -5, dtype=torch.int32, device=dev)
    dlen = torch.full((ld_dst,), -5, dtype=torch.int32, device=dev)
    args = (n_out, n, torch.from_numpy(src).to(dev), torch.from_numpy(kind).to(dev), slots, length, k)
    divide_rnaps(*args, dst, dlen, model.seed, 9)
    want = xref.divide_rnaps(lists, keys, src, kind, model.seed, 9)
    got_slots, got_len = dst.cpu().numpy(), dlen.cpu().numpy()
    assert xref.unpack_lists(got_slots, got_len, n_out) == want
    assert np.all(got_len[n_out:] == -5) and np.all(got_slots[:, n_out:] == -5)
    for j in range(n_out):
        assert np.all(got_slots[got_len[j]:, j] == 0)                     # zeroed beyond the new length
    for i, a in enumerate(mothers):                                       # order kept, nobody lost or doubled
        d0, d1 = want[len(keep) + 2 * i], want[len(keep) + 2 * i + 1]
        assert sorted(map(tuple, d0 + d1)) == sorted(map(tuple, lists[a]))
    if n >= 65:
        assert any(want[len(keep) + 2 * i] and want[len(keep) + 2 * i + 1] for i in range(len(mothers)))
        # a seed of its own: the ribosomes' coins under the same model seed fall differently
        dst2, dlen2 = torch.zeros_like(dst), torch.zeros_like(dlen)
        divide_ribosomes(*args, dst2, dlen2, model.seed, 9)
        assert not torch.equal(dlen2[:n_out], dlen[:n_out])


def ragged_wave_case():
    """step_case(65) at ld = 70, a full wave and a wave of one lane, arranged so that the lanes of the
    full wave leave the shared initiation loop at different rounds: two keys outside [0, 2**31), one
    full list that stalls (no nucleotides, nobody occluding) in front of free RNAPs, and max_events = 2.  Returns
    (model, sm, the inputs, the restatement's two steps, its smallest margins)."""
    n, ld = 65, 70
    model, sm, lists, molecules, counts, m2c, keys = xref.step_case(n, cap=CAP)
    molecules, counts = molecules[:, :ld].copy(), counts[:, :ld].copy()
    m2c, keys = m2c[:ld].copy(), keys[:ld].copy()
    keys[3], keys[40] = -1, 2 ** 31
    assert len(lists[7]) == CAP
    lists[7] = [[t, i, p, False] for t, i, p, _ in lists[7]]             # both promoters stay open
    molecules[:4, 7] = 0
    counts[xref.SPECIES.index('RNA Polymerase'), 7] = 4
    l, mol, x = copy.deepcopy(lists), molecules.copy(), counts.copy()
    status, want, worst = np.zeros(n, dtype=np.int32), [], np.full(4, np.inf)
    for k in range(2):
        events, status, margins = xref.step(model, model.bind(sm), l, mol, x, m2c, keys, DT, model.seed, k, status,
                                            max_events=2)
        worst = np.minimum(worst, margins.min(axis=0))
        want.append((copy.deepcopy(l), mol.copy(), x.copy(), events.copy(), status.copy()))
    return model, sm, (lists, molecules, counts, m2c, keys), want, worst


def test_lanes_leave_the_shared_loop_at_different_rounds(dev):
    """The status tests above run one agent at a time; here the exits of the kernel's initiation loop
    are taken per lane under the wave-wide __any, beside neighbours that go on.  Two steps, every array bitwise against the
    restatement, columns >= n included."""
    from lens_amd import native
    model, sm, (lists, molecules, counts, m2c, keys), want, worst = ragged_wave_case()
    n = len(lists)
    assert np.all(worst >= xref.MARGIN)                                  # no agent is left out
    first, last = want[0], want[-1]
    assert [a for a in range(n) if last[4][a] & native.VK_TX_BAD_KEY] == [3, 40]
    assert first[4][7] & native.VK_TX_SLOTS_FULL and len(first[0][7]) == CAP
    stopped = (first[4] & native.VK_TX_MAX_EVENTS) != 0
    assert np.all(first[3][stopped] == 2) and 0 < stopped[:64].sum() < 64 and first[3][:64].min() == 0
    assert len({int(e) for e in first[3][:64]}) == 3                    # lanes that fired 0, 1 and 2 times
    got = _run(dev, model, sm, lists, molecules, counts, m2c, keys, n, DT, 2, max_events=2)
    _compare(got, want, n)
