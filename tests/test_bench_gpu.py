"""bench.py's timed path on a GPU: a plain run measures the headline only, and what
--dump-outputs writes is the state a fixed number of steps after the seeded start,
whatever the clock made of the untimed settle steps."""

import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402
from test_configs import _bench_stencil  # noqa: E402

STEPS, WARMUP, AGENTS = 4, 1, 20000
NAMES = ['conc', 'counts', 'field_ac_e', 'field_glc__D_e', 'flux']


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def _args(out_dir, *extra):
    args = bench.parse(['--workload', 'c3', '--steps', str(STEPS), '--warmup', str(WARMUP),
                        '--dump-outputs', str(out_dir)] + list(extra))
    args.agents = AGENTS
    return args


def _load(path):
    assert sorted(os.listdir(path)) == [n + '.npy' for n in NAMES]
    return {n: np.load(os.path.join(path, n + '.npy')) for n in NAMES}


def test_plain_run_times_the_steps_and_dumps_the_same_arrays_every_time(dev, tmp_path):
    """Two plain C3 runs (graph replay, clock-counted settle replays): the line holds
    the headline keys and no measurement of its own run; both dumps equal, bit for
    bit, WARMUP + STEPS eager steps of the same seeded colony."""
    outs = []
    with _bench_stencil('c3'):
        for d in ('a', 'b'):
            line = bench.run(_args(tmp_path / d), 0, 1, dev, None)
            assert line['steps'] == STEPS and line['warmup'] == WARMUP
            assert line['ms_per_step'] > 0 and line['value'] > 0
            assert line['unit'] == 'agent-steps/s' and line['higher_is_better'] is True and line['dtype'] == 'f64'
            assert line['untimed_settle_steps'] > 0          # the state was put back after them
            assert line['roofline'] is None and line['integrator']['avg_ms_per_step'] is None
            assert 'cpu_baseline' not in line and 'cpu_baseline_odeint' not in line
            outs.append(_load(tmp_path / d))
        col, lat, _ = bench.build_rank(_args(tmp_path / 'c'), 0, 1, dev)
        for _ in range(WARMUP + STEPS):
            col.step(1.0)
        torch.cuda.synchronize()
        col.check_status()
        want = {n: t.to(torch.float64).cpu().numpy().reshape(-1, t.shape[-1])
                for n, t in bench.colony_outputs(col, lat)}
    a, b = outs
    for n in NAMES:
        assert a[n].dtype == np.float64 and np.isfinite(a[n]).all()
        assert np.array_equal(a[n], b[n]), n
        assert np.array_equal(a[n], want[n]), n
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES
    assert a['conc'].shape[1] == AGENTS and a['field_ac_e'].shape == (1, 1024 * 1024)
    assert np.any(a['field_ac_e'] != 0) and np.any(a['counts'] != 0)
