"""Timing of the colony-mechanics launches at the C4 size (the
mechanics section): 1M capsules of 2 x 1 um on 4096^2 bins of 1 um, neighbour
grid 1024^2 cells of 4 um, at several areal densities (agents uniform over a
centred square of side sqrt(n / density); the first density is the whole plane).

    python scripts/mechanics_timing.py [--agents N] [--nx NX] [--reps R] [--densities D ...]
    python scripts/mechanics_timing.py --only-contact --densities D      # the launches alone, for a profiler
    python scripts/mechanics_timing.py --fold D=trace.csv ...            # add the per-kernel split of such runs

Per density: HIP-event times (median of R repetitions after a warm-up, min and
max) of vk_contact_step with 1 and with 4 iterations, the mean number of
neighbours a thread of the relax kernel visits, and that kernel's algorithmic
bytes.  ``--fold`` reads rocprofv3 kernel traces (``--kernel-trace
--output-format csv``) of ``--only-contact`` runs and adds each iteration's
split: cells + sort (k_contact_cells and vk_occupancy_sort's kernels), pack,
relax (kernel time per iteration), and the relax kernel's achieved bytes/s.
Then the step time of a C4-like colony (glc_ac kinetics, the bench's stencil
settings) with and without mechanics, replayed from captured graphs,
alternating.  Prints one JSON line.  Needs a GPU: there is no fallback.
"""

import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lens_amd import configs                                      # noqa: E402
from lens_amd.colony import Colony                                # noqa: E402
from lens_amd.lattice import Lattice, stencil_depth, stencil_kernel, stencil_mode   # noqa: E402
from lens_amd.mechanics import ContactModel, contact_step         # noqa: E402
from lens_amd.rate_law_compiler import compile_rate_laws          # noqa: E402

# the parent commit's figures for the motile colony's launches at this size
YARDSTICKS_MS = {'sort_plus_ordered_exchange': 0.29, 'motility_launch': 0.38}


def model(iterations=4):
    return ContactModel(iterations=iterations, jitter=0.01, jitter_angle=0.02, seed=configs.SEED)


def locations(n, nx, density, seed=configs.SEED):
    rng = np.random.default_rng(seed)
    side = float(nx) if density is None else min(float(nx), (n / density) ** 0.5)
    return (nx - side) / 2 + rng.uniform(0.0, side, (2, n))


def build(dev, n, nx, density, mechanics):
    cfg = configs.glc_ac_config()
    table = compile_rate_laws(cfg['reactions'], cfg['kinetic_parameters'])
    lat = Lattice(['glc__D_e', 'ac_e'], (nx, nx), (float(nx), float(nx)), 10.0, 5.0, device=dev,
                  initial={'glc__D_e': configs.gaussian_bump_field((nx, nx)), 'ac_e': np.zeros((nx, nx))})
    params, conc = configs.heterogeneous_colony(table, cfg, n, seed=configs.SEED)
    col = Colony(cfg, n, device=dev, integrator='dopri5', environment=lat, table=table, specialize=True,
                 mechanics=model() if mechanics else None)
    col.set_agents(params=params, conc=conc, location=locations(n, nx, density))
    col.gather_external()
    return col


def event_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms))}


def neighbours_visited(loc, n, bounds, m):
    """Mean over agents of the other agents in the 3 x 3 grid cells around their own."""
    gx, gy = m.grid(bounds)
    cx = torch.clamp((loc[0, :n] / (bounds[0] / gx)).floor().long(), 0, gx - 1)
    cy = torch.clamp((loc[1, :n] / (bounds[1] / gy)).floor().long(), 0, gy - 1)
    count = torch.nn.functional.pad(torch.bincount(cx * gy + cy, minlength=gx * gy).reshape(gx, gy), (1, 1, 1, 1))
    box = sum(count[i:i + gx, j:j + gy] for i in range(3) for j in range(3))
    return float(box.reshape(-1)[cx * gy + cy].double().mean()) - 1.0


def relax_bytes(n, visited):
    """Algorithmic bytes of one k_contact_relax launch: per thread its own slot (32 B), direction
    (16), key, column and cell (12) and 9 pairs of table entries (72); per neighbour visited a
    slot (32; the direction, 16 more, only for the one pair in ten within reach: not counted);
    the centre and the angle written (24)."""
    return int(n * (32 + 16 + 12 + 72 + 24 + 32 * visited))


def contact_launcher(col, iterations):
    m = model(iterations)
    return lambda: contact_step(m, col.lattice, col.location, col.mech_angle, col.n, col._mech,
                                bin_lin=col.bin_lin, bin_ix=col.bin_ix)


def fold_trace(path):
    """Kernel time (ms) per iteration of each kernel group of one --only-contact trace."""
    rows = list(csv.DictReader(open(path)))
    n_relax = sum('k_contact_relax' in r['Kernel_Name'] for r in rows)
    total = {'cells_sort': 0.0, 'pack': 0.0, 'relax': 0.0}
    relax = []
    for r in rows:
        name, ms = r['Kernel_Name'], (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6
        if 'k_contact_relax' in name:
            total['relax'] += ms
            relax.append(ms)
        elif 'k_contact_pack' in name:
            total['pack'] += ms
        elif 'k_contact_cells' in name or 'k_occupancy' in name or 'rocprim' in name:
            total['cells_sort'] += ms
    out = {k + '_ms_per_iteration': v / max(n_relax, 1) for k, v in total.items()}
    out['iterations_traced'] = n_relax
    out['relax_median_ms'] = statistics.median(relax) if relax else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1_000_000)
    ap.add_argument('--nx', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--graph-steps', type=int, default=10)
    ap.add_argument('--densities', type=float, nargs='+', default=[0.0, 0.25, 0.5],
                    help='agents per um^2; 0: uniform over the whole plane')
    ap.add_argument('--only-contact', action='store_true',
                    help='run reps x vk_contact_step (4 iterations) at the first density and exit')
    ap.add_argument('--fold', nargs='*', default=[], metavar='DENSITY=TRACE.csv')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mechanics_timing: needs a GPU')
    dev = torch.device('cuda', 0)
    stencil_mode('fma'), stencil_depth(10), stencil_kernel(70, 64)     # the bench's C4 settings
    n, nx = args.agents, args.nx
    densities = [d or None for d in args.densities]

    if args.only_contact:
        col = build(dev, n, nx, densities[0], True)
        event_ms(contact_launcher(col, 4), args.reps)
        col.check_status()
        return

    traces = dict(item.split('=', 1) for item in args.fold)
    res = {'agents': n, 'bins': [nx, nx], 'capsule_um': [2.0, 1.0], 'grid_cell_um': 4.0, 'reps': args.reps,
           'device': torch.cuda.get_device_name(0), 'yardsticks_parent_ms': YARDSTICKS_MS, 'densities': []}
    col = build(dev, n, nx, None, True)
    col.step(1.0)                                                    # loads every kernel
    for d in densities:
        col.location[:, :n].copy_(torch.from_numpy(locations(n, nx, d)))
        visited = neighbours_visited(col.location, n, col.lattice.bounds, col.mechanics)
        entry = {'agents_per_um2': n / float(nx) ** 2 if d is None else d, 'neighbours_visited_mean': visited,
                 'relax_algorithmic_bytes': relax_bytes(n, visited)}
        entry['contact_step_1_iteration'] = summary(event_ms(contact_launcher(col, 1), args.reps))
        col.location[:, :n].copy_(torch.from_numpy(locations(n, nx, d)))
        entry['contact_step_4_iterations'] = summary(event_ms(contact_launcher(col, 4), args.reps))
        key = '%g' % (d or 0.0)
        if key in traces:
            split = fold_trace(traces[key])
            entry['per_iteration_split_from_trace'] = split
            if split['relax_median_ms']:
                entry['relax_achieved_TB_per_s'] = entry['relax_algorithmic_bytes'] / (split['relax_median_ms'] * 1e-3) / 1e12
        res['densities'].append(entry)
    col.check_status()

    # the full step, with and without mechanics, at the densest setting
    d = densities[-1]
    mech, plain = build(dev, n, nx, d, True), build(dev, n, nx, d, False)
    mech.step(1.0)
    plain.step(1.0)
    k = args.graph_steps
    replays = {'mechanics': mech.capture(1.0, k), 'plain': plain.capture(1.0, k)}
    steps = {name: [] for name in replays}
    for name, r in replays.items():
        r()
    for _ in range(5):                                               # alternating
        for name, r in replays.items():
            steps[name] += [t / k for t in event_ms(r, 1, warmup=0)]
    res['step_density'] = d
    res['step_ms_mechanics'] = summary(steps['mechanics'])
    res['step_ms_plain'] = summary(steps['plain'])
    mech.check_status()
    res['agents_with_status'] = int((mech.status[:n] != 0).sum())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
