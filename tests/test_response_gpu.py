"""vk_response_begin / vk_response_end / vk_response_cells and the float exchanges
against the NumPy restatement (tests/response_ref.py), bit for bit.

Sizes: a lone lane, both sides of a wavefront, past a block; ld > n with sentinel
values in the padding columns that must survive; live, dying and frozen agents
mixed within one wave; two porins, two diffusing molecules, two detector keys."""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import response_ref as ref
from lens_amd import native

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
N_A = 6.022140857e23
# rows of the test's conc: two molecules (internal, external), two porins, a pump, an RNA
ROWS = 9
MOL_INT, MOL_EXT = [0, 5], [3, 7]
PORIN_ROW, PORIN_PERM = [4, 1], [0.1, 0.35]
DET_ROW, DET_THR = [0, 5], [0.95, 0.4]
SAVE_ROW = [0, 5]                 # the "kinetics" of this test writes rows 0 and 5
EXPR_ROW = [8, 2]
N_FLUX, N_EXT = 3, 2


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    native.load()
    return torch.device('cuda', 0)


def _table(dev, volume_fl=1.2, keep=None, **over):
    arrays = dict(mol_int_row=(MOL_INT, np.int32), mol_ext_row=(MOL_EXT, np.int32), porin_row=(PORIN_ROW, np.int32),
                  porin_perm=(PORIN_PERM, np.float64), det_row=(DET_ROW, np.int32), det_thr=(DET_THR, np.float64),
                  save_row=(SAVE_ROW, np.int32), expr_row=(EXPR_ROW, np.int32))
    t = native.VkResponseTable()
    t.n_mol, t.n_porin, t.n_det, t.n_save, t.n_expr = 2, 2, 2, 2, 2
    t.n_flux, t.n_ext = N_FLUX, N_EXT
    for name, (values, dtype) in arrays.items():
        d = torch.from_numpy(np.array(values, dtype=dtype)).to(dev)
        keep.append(d)
        setattr(t, name, d.data_ptr())
    t.avogadro, t.volume_fl = N_A, volume_fl
    for k, v in over.items():
        setattr(t, k, v)
    return t


def _same(got, want, what):
    """array_equal with the first differing elements in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, [(tuple(i), got[tuple(i)], want[tuple(i)]) for i in bad[:6]])


def _padded(rng, rows, n, ld, dtype=np.float64, lo=0.0, hi=1.0):
    shape = (rows, ld) if rows else (ld,)
    a = np.full(shape, SENTINEL, dtype=dtype) if dtype == np.float64 else np.full(shape, -77, dtype=dtype)
    vals = rng.uniform(lo, hi, shape[:-1] + (n,)) if dtype == np.float64 else rng.integers(1, 50, shape[:-1] + (n,))
    a[..., :n] = vals
    return a


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('with_volume', [True, False])
def test_begin_and_end_match_the_restatement(dev, n, with_volume):
    rng = np.random.default_rng(100 + n)
    ld = n + 7
    dt = 0.5
    conc = _padded(rng, ROWS, n, ld, hi=1.3)            # rows 0 and 5 straddle their thresholds
    conc[[4, 1], :n] = rng.uniform(1e-16, 3e-15, (2, n))
    volume = _padded(rng, 0, n, ld, lo=1.0, hi=2.4)
    frozen = np.full(ld, -77, dtype=np.int32)
    frozen[:n] = rng.integers(0, 3, n) == 0            # about a third frozen, anywhere in a wave
    flux = _padded(rng, N_FLUX, n, ld)
    status = _padded(rng, 0, n, ld, dtype=np.int32)
    nsteps = _padded(rng, 0, n, ld, dtype=np.int32)
    dead = np.full(ld, -77, dtype=np.int32)
    dead[:n] = frozen[:n]
    keep = []
    t = _table(dev, keep=keep)
    up = lambda a: torch.from_numpy(a.copy()).to(dev)
    d = {k: up(v) for k, v in dict(conc=conc, volume=volume, frozen=frozen, flux=flux, status=status, nsteps=nsteps,
                                   dead=dead).items()}
    z = lambda rows, dtype=torch.float64: torch.full((rows, ld) if rows else (ld,), SENTINEL if dtype == torch.float64
                                                     else -77, dtype=dtype, device=dev)
    dying, delta, fcounts = z(0, torch.int32), z(2), z(2)
    save_conc, save_flux, save_status, save_nsteps = z(2), z(N_FLUX), z(0, torch.int32), z(0, torch.int32)
    native.check(native._lib.vk_response_begin(
        ctypes.byref(t), n, ld, dt, native.ptr(d['conc']), native.ptr(d['volume']) if with_volume else 0,
        native.ptr(d['frozen']), native.ptr(dying), native.ptr(delta), native.ptr(fcounts), native.ptr(save_conc),
        native.ptr(d['flux']), native.ptr(save_flux), native.ptr(d['status']), native.ptr(save_status),
        native.ptr(d['nsteps']), native.ptr(save_nsteps), native.stream_handle()), 'vk_response_begin')

    # the restatement, agent after agent
    want_dying = np.zeros(n, dtype=np.int32)
    want_delta, want_fc = np.zeros((2, n)), np.zeros((2, n))
    for a in range(n):
        col = conc[:, a]
        want_dying[a] = (not frozen[a]) and any(col[r] > thr for r, thr in zip(DET_ROW, DET_THR))
        want_delta[:, a], want_fc[:, a] = ref.membrane_terms(col, volume[a] if with_volume else 1.2, dt, N_A, MOL_INT,
                                                              MOL_EXT, PORIN_ROW, PORIN_PERM)
    assert np.array_equal(dying[:n].cpu().numpy(), want_dying)
    assert np.array_equal(delta[:, :n].cpu().numpy(), want_delta)
    assert np.array_equal(fcounts[:, :n].cpu().numpy(), want_fc)
    live, fr = frozen[:n] == 0, frozen[:n] != 0
    assert want_dying.sum() > 0 or n == 1
    assert np.array_equal(save_conc[:, :n].cpu().numpy()[:, fr], conc[SAVE_ROW][:, :n][:, fr])
    assert np.array_equal(save_flux[:, :n].cpu().numpy()[:, fr], flux[:, :n][:, fr])
    assert (save_conc[:, :n].cpu().numpy()[:, live] == SENTINEL).all()          # only frozen agents are saved
    for pad in (dying, delta, fcounts, save_conc, save_flux, save_status, save_nsteps):
        p = pad[..., n:].cpu().numpy()
        assert ((p == SENTINEL) | (p == -77)).all()

    # what the existing launches do in between: the kinetics overwrites its rows, fluxes, status,
    # attempts and counts of EVERY agent; the gather writes every agent's external rows
    kin = _padded(rng, ROWS, n, ld, hi=1.3)
    new_flux, new_status, new_nsteps = _padded(rng, N_FLUX, n, ld), _padded(rng, 0, n, ld, dtype=np.int32), \
        _padded(rng, 0, n, ld, dtype=np.int32)
    counts = np.full((N_EXT, ld), -77, dtype=np.int64)
    counts[:, :n] = rng.integers(-1000, 1000, (N_EXT, n))
    after = conc.copy()
    after[SAVE_ROW, :n] = kin[SAVE_ROW, :n]
    field = rng.uniform(0.0, 3.0, (2, 16))
    bins = np.full(ld, 0, dtype=np.int32)
    bins[:n] = rng.integers(0, 16, n)
    d['conc'].copy_(up(after))
    d['flux'].copy_(up(new_flux))
    d['status'].copy_(up(new_status))
    d['nsteps'].copy_(up(new_nsteps))
    d_counts = up(counts)
    # every device array stays referenced until its launch has run (a freed block is handed out again)
    d_field, d_bins = up(field), up(bins)
    d_planes, d_rows = up(np.array([0, 1], dtype=np.int32)), up(np.array(MOL_EXT, dtype=np.int32))
    native.check(native._lib.vk_gather(
        native.ptr(d_field), 16, native.ptr(d_bins), n, native.ptr(d_planes), native.ptr(d_rows), 2,
        native.ptr(d['conc']), ld, native.stream_handle()), 'vk_gather')
    expr_update = up(_padded(rng, 2, n, ld, lo=-0.1, hi=0.1))
    native.check(native._lib.vk_response_end(
        ctypes.byref(t), n, ld, native.ptr(d['conc']), native.ptr(delta), native.ptr(expr_update),
        native.ptr(d['frozen']), native.ptr(dying), native.ptr(d['dead']), native.ptr(save_conc),
        native.ptr(d['flux']), native.ptr(save_flux), native.ptr(d['status']), native.ptr(save_status),
        native.ptr(d['nsteps']), native.ptr(save_nsteps), native.ptr(d_counts), native.stream_handle()),
        'vk_response_end')
    eu = expr_update.cpu().numpy()
    want = after.copy()
    want_flux, want_status, want_nsteps, want_counts = new_flux.copy(), new_status.copy(), new_nsteps.copy(), counts.copy()
    for a in range(n):
        for m in range(2):
            want[MOL_EXT[m], a] = field[m, bins[a]]                 # frozen agents take the gather too
        if frozen[a]:
            want[SAVE_ROW, a] = conc[SAVE_ROW, a]
            want_flux[:, a], want_status[a], want_nsteps[a] = flux[:, a], status[a], nsteps[a]
            want_counts[:, a] = 0
        else:
            for j, r in enumerate(EXPR_ROW):
                want[r, a] = want[r, a] + eu[j, a]
        for m, r in enumerate(MOL_INT):
            want[r, a] = want[r, a] + want_delta[m, a]              # (conc + kinetics) + membrane, last
    want_frozen, want_dead = frozen.copy(), dead.copy()
    want_frozen[:n] |= want_dying
    want_dead[:n] |= want_dying
    got = {k: v.cpu().numpy() for k, v in d.items()}
    del d_field, d_bins, d_planes, d_rows, keep
    _same(got['conc'], want, 'conc')                                # the padding columns included
    _same(got['flux'], want_flux, 'flux')
    _same(got['status'], want_status, 'status')
    _same(got['nsteps'], want_nsteps, 'nsteps')
    _same(d_counts.cpu().numpy(), want_counts, 'counts')
    _same(got['frozen'], want_frozen, 'frozen')
    _same(got['dead'], want_dead, 'dead')


def test_cells_save_and_restore_only_frozen_agents(dev):
    rng = np.random.default_rng(5)
    n, ld = 65, 70
    cell = _padded(rng, native.VK_CELL_ROWS, n, ld, lo=1.0, hi=3.0)
    m2c = _padded(rng, 0, n, ld, lo=7e5, hi=8e5)
    divide = np.zeros(ld, dtype=np.int32)
    frozen = np.zeros(ld, dtype=np.int32)
    frozen[:n] = rng.integers(0, 2, n)
    dying = np.zeros(ld, dtype=np.int32)
    dying[:n] = frozen[:n] * (rng.integers(0, 3, n) == 0)     # frozen by this very step: still grows and divides
    up = lambda a: torch.from_numpy(a.copy()).to(dev)
    d_cell, d_m2c, d_div, d_fr, d_dy = up(cell), up(m2c), up(divide), up(frozen), up(dying)
    s_cell, s_m2c, s_div = torch.zeros_like(d_cell), torch.zeros_like(d_m2c), torch.zeros_like(d_div)

    def call(restore):
        native.check(native._lib.vk_response_cells(
            restore, n, ld, native.ptr(d_fr), native.ptr(d_dy), native.ptr(d_cell), native.ptr(d_m2c), native.ptr(d_div),
            native.ptr(s_cell), native.ptr(s_m2c), native.ptr(s_div), native.stream_handle()), 'vk_response_cells')

    call(0)
    grown, m2c2 = cell * 1.01, m2c * 1.01                     # the growth launch, on every agent
    d_cell.copy_(up(grown))
    d_m2c.copy_(up(m2c2))
    d_div.fill_(1)
    call(1)
    fr = (frozen != 0) & (dying == 0)
    assert dying.sum() > 0 and fr.sum() > 0
    want_cell, want_m2c, want_div = grown.copy(), m2c2.copy(), np.ones(ld, dtype=np.int32)
    want_cell[:, fr], want_m2c[fr], want_div[fr] = cell[:, fr], m2c[fr], 0
    assert np.array_equal(d_cell.cpu().numpy(), want_cell)
    assert np.array_equal(d_m2c.cpu().numpy(), want_m2c)
    assert np.array_equal(d_div.cpu().numpy(), want_div)


# -- the float exchange --------------------------------------------------------------

# a 4 x 4 plane; bins hold 0, 1, 2 and 5 agents; storage order is not key order
BINS = np.array([5, 9, 2, 9, 2, 2, 2, 2], dtype=np.int32)
KEYS = np.array([40, 7, 33, 21, 5, 2, 60, 11], dtype=np.int64)
BVA = (2.0 * 1e-15) * N_A


def _exchange_case(seed=3):
    rng = np.random.default_rng(seed)
    n = len(BINS)
    counts = rng.integers(-500000, 500000, (2, n)).astype(np.int64)      # up to 0.4 mM against fields of 1
    fcounts = rng.uniform(-300000.0, 300000.0, (2, n))
    fields = rng.uniform(0.5, 2.0, (3, 16))
    return counts, fcounts, fields


def _ordered(bins, keys):
    order = np.lexsort((keys, bins)).astype(np.int32)
    return order, bins[order].astype(np.int32)


def _loop_exchange(fields, order, bins, counts, fcounts, map_int, map_float, two_pass=False):
    """Agent after agent in (bin, key) order; map_*: [(row, plane)]."""
    out = fields.copy()
    for plane in range(out.shape[0]):
        ints = [r for r, p in map_int if p == plane]
        flts = [r for r, p in map_float if p == plane]
        if two_pass:
            for a in order:
                for r in ints:
                    out[plane, bins[a]] = out[plane, bins[a]] + ref.mM(counts[r, a], BVA)
            for a in order:
                for r in flts:
                    out[plane, bins[a]] = out[plane, bins[a]] + ref.mM(fcounts[r, a], BVA)
            continue
        for a in order:
            v = out[plane, bins[a]]
            for r in ints:
                v = v + ref.mM(counts[r, a], BVA)
            for r in flts:
                v = v + ref.mM(fcounts[r, a], BVA)
            out[plane, bins[a]] = v
    return out


# plane 0 takes both arrays, plane 1 only ints, plane 2 only floats
MAP_INT, MAP_FLOAT = [(1, 0), (0, 1)], [(0, 2), (1, 0)]


def _mixed(dev, fields, order, sorted_bin, counts, fcounts, map_int, map_float, n=None):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    i32 = lambda xs: up(np.array(xs, dtype=np.int32))
    f = up(fields)
    c, fc = (None if counts is None else up(counts)), (None if fcounts is None else up(fcounts))
    mi = (i32([r for r, _ in map_int]), i32([p for _, p in map_int]))
    mf = (i32([r for r, _ in map_float]), i32([p for _, p in map_float]))
    d_sorted, d_order = up(sorted_bin), up(order)      # held until the launch has run
    rc = native._lib.vk_exchange_ordered_mixed(
        native.ptr(f), fields.shape[1], native.ptr(d_sorted), native.ptr(d_order),
        len(order) if n is None else n, native.ptr(c), len(BINS), native.ptr(mi[0]), native.ptr(mi[1]), len(map_int),
        native.ptr(fc), len(BINS), native.ptr(mf[0]), native.ptr(mf[1]), len(map_float), BVA, native.stream_handle())
    torch.cuda.synchronize()
    del d_sorted, d_order, c, fc, mi, mf
    return rc, f.cpu().numpy()


def test_mixed_exchange_interleaves_per_agent(dev):
    counts, fcounts, fields = _exchange_case()
    order, sorted_bin = _ordered(BINS, KEYS)
    assert not np.array_equal(order, np.arange(len(BINS)))
    assert set(np.bincount(BINS, minlength=16).tolist()) == {0, 1, 2, 5}
    want = _loop_exchange(fields, order, BINS, counts, fcounts, MAP_INT, MAP_FLOAT)
    # the companion: all ints and then all floats rounds differently where agents share a bin
    other = _loop_exchange(fields, order, BINS, counts, fcounts, MAP_INT, MAP_FLOAT, two_pass=True)
    assert not np.array_equal(want[0], other[0])
    assert np.array_equal(want[1:], other[1:])
    # and so does storage order instead of key order
    assert not np.array_equal(want, _loop_exchange(fields, np.arange(len(BINS)), BINS, counts, fcounts, MAP_INT, MAP_FLOAT))
    rc, got = _mixed(dev, fields, order, sorted_bin, counts, fcounts, MAP_INT, MAP_FLOAT)
    assert rc == native.VK_OK
    assert np.array_equal(got, want)
    # either array may be absent
    rc, got = _mixed(dev, fields, order, sorted_bin, None, fcounts, [], MAP_FLOAT)
    assert rc == native.VK_OK
    assert np.array_equal(got, _loop_exchange(fields, order, BINS, counts, fcounts, [], MAP_FLOAT))
    rc, got = _mixed(dev, fields, order, sorted_bin, counts, None, MAP_INT, [])
    assert rc == native.VK_OK
    assert np.array_equal(got, _loop_exchange(fields, order, BINS, counts, fcounts, MAP_INT, []))


def test_mixed_exchange_equals_the_ordered_exchange_without_floats(dev):
    counts, fcounts, fields = _exchange_case(8)
    order, sorted_bin = _ordered(BINS, KEYS)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f = up(fields)
    held = [up(sorted_bin), up(order), up(counts), up(np.array([1, 0], dtype=np.int32)),
            up(np.array([0, 1], dtype=np.int32))]             # held until the launch has run
    native.check(native._lib.vk_exchange_ordered(
        native.ptr(f), 16, native.ptr(held[0]), native.ptr(held[1]), len(BINS), native.ptr(held[2]), len(BINS),
        native.ptr(held[3]), native.ptr(held[4]), 2, BVA, native.stream_handle()), 'vk_exchange_ordered')
    torch.cuda.synchronize()
    rc, got = _mixed(dev, fields, order, sorted_bin, counts, None, MAP_INT, [])
    assert rc == native.VK_OK and np.array_equal(got, f.cpu().numpy())


def _atomic(dev, fields, bins, fcounts, rows, planes):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f = up(fields)
    held = [up(bins), up(fcounts), up(np.array(rows, dtype=np.int32)), up(np.array(planes, dtype=np.int32))]
    native.check(native._lib.vk_exchange_atomic_f64(
        native.ptr(f), fields.shape[1], native.ptr(held[0]), len(bins), native.ptr(held[1]), fcounts.shape[1],
        native.ptr(held[2]), native.ptr(held[3]), len(rows), BVA, native.stream_handle()), 'vk_exchange_atomic_f64')
    torch.cuda.synchronize()                               # `held` is referenced until the launch has run
    return f.cpu().numpy()


def test_atomic_f64_one_agent_per_bin_is_exact(dev):
    rng = np.random.default_rng(12)
    n = 300                                              # more than one block
    fields = rng.uniform(0.5, 2.0, (2, n + 5))
    bins = rng.permutation(n + 5)[:n].astype(np.int32)
    fcounts = rng.uniform(-3000.0, 3000.0, (2, n))
    want = fields.copy()
    for a in range(n):
        want[1, bins[a]] = want[1, bins[a]] + ref.mM(fcounts[0, a], BVA)
        want[0, bins[a]] = want[0, bins[a]] + ref.mM(fcounts[1, a], BVA)
    assert np.array_equal(_atomic(dev, fields, bins, fcounts, [0, 1], [1, 0]), want)


def test_atomic_f64_shared_bins_within_the_atomic_bound(dev):
    counts, fcounts, fields = _exchange_case(4)
    want = _loop_exchange(fields, np.arange(len(BINS)), BINS, counts, fcounts, [], MAP_FLOAT)
    got = _atomic(dev, fields, BINS, fcounts, [r for r, _ in MAP_FLOAT], [p for _, p in MAP_FLOAT])
    # the bound tests/test_gpu_parity.py uses for the atomic exchange
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)


def test_bad_arguments_return_err_arg(dev):
    keep = []
    t = _table(dev, keep=keep)
    n, ld = 4, 4
    buf = torch.zeros((ROWS, ld), dtype=torch.float64, device=dev)
    i32 = torch.zeros(ld, dtype=torch.int32, device=dev)
    i64 = torch.zeros((N_EXT, ld), dtype=torch.int64, device=dev)
    p, q, c = native.ptr(buf), native.ptr(i32), native.ptr(i64)
    s = native.stream_handle()
    lib = native._lib
    begin = lambda tt=t, n=n, ld=ld, conc=p, frozen=q, delta=p: lib.vk_response_begin(
        ctypes.byref(tt) if tt is not None else None, n, ld, 1.0, conc, 0, frozen, q, delta, p, p, p, p, q, q, q, q, s)
    assert begin() == native.VK_OK
    assert begin(tt=None) == native.VK_ERR_ARG
    assert begin(n=-1) == native.VK_ERR_ARG
    assert begin(n=5) == native.VK_ERR_ARG                       # ld < n
    assert begin(conc=0) == native.VK_ERR_ARG
    assert begin(frozen=0) == native.VK_ERR_ARG
    assert begin(delta=0) == native.VK_ERR_ARG
    assert begin(tt=_table(dev, keep=keep, n_porin=-1)) == native.VK_ERR_ARG
    assert begin(tt=_table(dev, keep=keep, det_row=None)) == native.VK_ERR_ARG
    assert b'vk_response_begin' in lib.vk_last_error()
    assert begin(n=0, conc=0, frozen=0, delta=0) == native.VK_OK
    end = lambda tt=t, n=n, conc=p, dead=q, counts=c: lib.vk_response_end(
        ctypes.byref(tt), n, ld, conc, p, 0, q, q, dead, p, p, p, q, q, q, q, counts, s)
    assert end() == native.VK_OK
    assert end(n=5) == native.VK_ERR_ARG
    assert end(conc=0) == native.VK_ERR_ARG
    assert end(dead=0) == native.VK_ERR_ARG
    assert end(counts=0) == native.VK_ERR_ARG
    assert b'vk_response_end' in lib.vk_last_error()
    assert lib.vk_response_cells(0, n, ld, q, q, p, p, q, p, p, 0, s) == native.VK_ERR_ARG
    assert lib.vk_response_cells(0, n, ld, q, 0, p, p, q, p, p, q, s) == native.VK_ERR_ARG
    assert lib.vk_response_cells(0, 5, ld, q, q, p, p, q, p, p, q, s) == native.VK_ERR_ARG
    counts, fcounts, fields = _exchange_case()
    order, sorted_bin = _ordered(BINS, KEYS)
    assert _mixed(dev, fields, order, sorted_bin, None, fcounts, MAP_INT, MAP_FLOAT)[0] == native.VK_ERR_ARG
    assert _mixed(dev, fields, order, sorted_bin, counts, None, MAP_INT, MAP_FLOAT)[0] == native.VK_ERR_ARG
    assert _mixed(dev, fields, order, sorted_bin, counts, fcounts, MAP_INT, MAP_FLOAT, n=len(BINS) + 1)[0] == native.VK_ERR_ARG
    assert _mixed(dev, fields, order, sorted_bin, counts, fcounts, MAP_INT, MAP_FLOAT, n=-1)[0] == native.VK_ERR_ARG
    assert b'vk_exchange_ordered_mixed' in lib.vk_last_error()
    assert lib.vk_exchange_atomic_f64(p, 16, q, n, 0, ld, q, q, 1, BVA, s) == native.VK_ERR_ARG
    assert lib.vk_exchange_atomic_f64(p, 16, q, 5, p, ld, q, q, 1, BVA, s) == native.VK_ERR_ARG
    assert b'vk_exchange_atomic_f64' in lib.vk_last_error()
    torch.cuda.synchronize()
