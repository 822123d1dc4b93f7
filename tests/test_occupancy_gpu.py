"""The device occupancy (vk_occupancy_sort) and the ordered exchange
(vk_exchange_ordered) against the host path they replace: lattice.occupancy
(two torch sorts + unique_consecutive) followed by vk_exchange_sorted.  The
fields must come out bit for bit the same -- each bin's agents are added in
reference agent order either way -- and ``order`` must be occupancy's."""

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

PLANES = {'17x23': (17, 23), '64x64': (64, 64)}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _bins(pattern, n, n_bins, rng):
    if pattern == 'random':
        return rng.integers(0, n_bins, n)
    if pattern == 'one_bin':
        return np.full(n, n_bins - 1)          # the last bin: the widest sort key
    # one agent per bin (as far as the bins go: round-robin beyond), in shuffled order
    return rng.permutation(n) % n_bins


@pytest.mark.parametrize('keys', ['identity', 'permuted'])
@pytest.mark.parametrize('pattern', ['random', 'one_bin', 'one_per_bin'])
@pytest.mark.parametrize('plane', sorted(PLANES))
@pytest.mark.parametrize('n', [0, 1, 257, 5000])
def test_device_occupancy_and_ordered_exchange_equal_the_host_path(dev, n, plane, pattern, keys):
    from lens_amd.lattice import Lattice, occupancy
    from lens_amd.motility import DeviceOccupancy
    nx, ny = PLANES[plane]
    rng = np.random.default_rng(1000 * n + 10 * nx + len(pattern) + len(keys))
    ld = n + 5
    bins = np.zeros(ld, dtype=np.int32)
    bins[:n] = _bins(pattern, n, nx * ny, rng)
    bin_lin = torch.from_numpy(bins).to(dev)
    key = None
    if keys == 'permuted':
        k = np.zeros(ld, dtype=np.int64)
        k[:n] = rng.permutation(n)
        key = torch.from_numpy(k).to(dev)
    # int64 counts with negatives and zeros, large enough that the order of the
    # additions shows in the last bits
    c = rng.integers(-10**9, 10**9, (3, ld))
    c[:, rng.random(ld) < 0.2] = 0
    counts = torch.from_numpy(c).to(dev)
    map_count = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    map_field = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    start = {m: rng.random((nx, ny)) for m in ('a', 'b', 'c')}
    mk = lambda: Lattice(['a', 'b', 'c'], (nx, ny), (float(nx), float(ny)), 10.0, 5.0, device=dev, initial=start)
    host, device = mk(), mk()

    occ = occupancy(bin_lin, n, key)
    host.exchange_sorted(occ, counts, map_count, map_field)

    d = DeviceOccupancy(ld, dev)
    order, sorted_bin = d.sort(bin_lin, n, nx * ny, key)
    device.exchange_ordered(order, sorted_bin, n, counts, map_count, map_field)
    torch.cuda.synchronize()

    assert torch.equal(order[:n], occ[2])
    assert torch.equal(sorted_bin[:n].to(torch.int64), bin_lin[:n].to(torch.int64)[order[:n].to(torch.int64)])
    assert bool((order[n:] == 0).all()) and bool((sorted_bin[n:] == 0).all())     # nothing past n is written
    assert torch.equal(host.fields, device.fields)
    if c[2, :n].any():
        assert not torch.equal(host.fields[0], torch.from_numpy(start['a']).to(dev))   # something was exchanged
    assert torch.equal(host.fields[1], torch.from_numpy(start['b']).to(dev))           # the unmapped plane
