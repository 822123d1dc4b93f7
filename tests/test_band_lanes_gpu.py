"""A whole-plane step run as row bands on two streams (vk_set_stencil_bands, the launch
loop of run_plan in lens_amd/csrc/vk_lattice.hip) against the same step unbanded: a
cell's bits do not depend on the launch that computes it, so the fields must be equal
bit for bit -- eager, and captured into a HIP graph and replayed.

300 x 300 planes, one random and one uniform (which every pass skips), tolerance mode,
depth 10, variants 20 and 70, 8- and 64-row tiles.  Steps of 100 substeps with the top
band starting at 160 rows and at 110 rows (its last launch is then 20 rows, shorter than
a 64-row chunk), and of 30 substeps starting at 50 rows.
"""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
N = 300
# (timestep, substeps, m_0)
CASES = [(1.0, 100, 160), (1.0, 100, 110), (0.295, 30, 50)]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def f0():
    return np.random.default_rng(31).random((N, N)) + 0.5


class _settings:
    """Tolerance mode, depth 10, the variant and tile rows; bands off on the way out."""

    def __init__(self, variant, rows):
        self.variant, self.rows = variant, rows

    def __enter__(self):
        from lens_amd.lattice import stencil_bands, stencil_depth, stencil_kernel, stencil_mode
        self.prev = (stencil_mode('fma'), stencil_depth(10), stencil_kernel(self.variant, self.rows), stencil_bands(1))

    def __exit__(self, *exc):
        from lens_amd.lattice import stencil_bands, stencil_depth, stencil_kernel, stencil_mode
        stencil_mode(self.prev[0])
        stencil_depth(self.prev[1])
        stencil_kernel(self.prev[2], 0)
        stencil_bands(self.prev[3])


def lattice(dev, f0):
    from lens_amd.lattice import Lattice
    return Lattice(['a', 'b'], (N, N), (float(N), float(N)), 10.0, 5.0, device=dev,
                   initial={'a': f0, 'b': np.full((N, N), 2.5)})


def lanes_of(n_sub):
    """The lanes of the step's plan under the current settings (vk_diffuse_plan_lanes)."""
    from lens_amd import native
    buf = (native.VkPass * 64)()
    lane, after, n = (ctypes.c_int32 * 64)(), (ctypes.c_int32 * 64)(), ctypes.c_int32(0)
    native.check(native._lib.vk_diffuse_plan_lanes(0, N, 0, N, 1, 1, 0, n_sub, n_sub, 0, 0, 0, buf, lane, after, 64,
                                                   ctypes.byref(n)), 'vk_diffuse_plan_lanes')
    return list(lane[:n.value])


def steps(dev, f0, timestep, count):
    """The planes after each of `count` eager steps."""
    lat = lattice(dev, f0)
    out = []
    for _ in range(count):
        lat.diffuse(timestep)
        out.append(lat.fields.clone())
    torch.cuda.synchronize()
    return out


def test_capture_before_any_eager_banded_call_runs_unbanded_and_agrees(dev, f0):
    """First in the file: no call has run banded yet, so the second stream and its events
    do not exist and nothing may be created under capture -- the captured step runs the
    unbanded plan.  (Were they there already, it would run banded; the bits are the same.)"""
    from lens_amd.lattice import n_substeps, stencil_bands
    timestep, n_sub, m0 = CASES[0]
    assert n_substeps(timestep) == n_sub
    with _settings(70, 64):
        want = steps(dev, f0, timestep, 2)          # bands off (this also loads the kernels)
        stencil_bands(2, m0)
        assert set(lanes_of(n_sub)) == {0, 1}
        lat = lattice(dev, f0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            lat.diffuse(timestep)
        for ref in want:
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(lat.fields, ref)
        assert not torch.equal(want[0][0], torch.as_tensor(f0, device=dev))


@pytest.mark.parametrize('timestep,n_sub,m0', CASES)
@pytest.mark.parametrize('rows', [8, 64])
@pytest.mark.parametrize('variant', [20, 70])
def test_banded_step_bitwise_equals_unbanded_eager_and_replayed(dev, f0, variant, rows, timestep, n_sub, m0):
    from lens_amd.lattice import n_substeps, stencil_bands
    assert n_substeps(timestep) == n_sub
    with _settings(variant, rows):
        assert lanes_of(n_sub) == [0] * (n_sub // 10)
        want = steps(dev, f0, timestep, 3)
        assert not torch.equal(want[0][0], torch.as_tensor(f0, device=dev))
        assert torch.equal(want[2][1], torch.full((N, N), 2.5, dtype=torch.float64, device=dev))
        stencil_bands(2, m0)
        assert lanes_of(n_sub) == [0, 1] * (n_sub // 10)
        got = steps(dev, f0, timestep, 3)           # eager, banded (creates the second stream)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        # the banded step captured (the second stream joins the capture and leaves it at
        # the end of the call), replayed twice after one eager step
        lat = lattice(dev, f0)
        lat.diffuse(timestep)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            lat.diffuse(timestep)
        for ref in want[1:]:
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(lat.fields, ref)
