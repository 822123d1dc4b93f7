"""Timing of the colony metrics (vk_colony_metrics) at the C4 size: 1M
capsules of 2 x 1 um on 4096^2 um, on the sparse plane (uniform over the whole plane) and the
packed plane (0.5 agents per um^2) of scripts/mechanics_timing.py.

    python scripts/colony_metrics_timing.py [--agents N] [--nx NX] [--reps R] [--out FILE]
    python scripts/colony_metrics_timing.py --only-metrics --plane packed     # the call alone, for a profiler
    python scripts/colony_metrics_timing.py --fold sparse=trace.csv packed=trace.csv [--out FILE]

The first form times, per plane and in the same run, the whole call (HIP events, median of R
repetitions after a warm-up, min and max), the labels-only call (metrics == NULL) and ONE
relaxation iteration of vk_contact_step on the same agents: the yardstick, parent code that
shares the grid and the sort.  It writes ``profiles/colony_metrics_timing.json`` (``--out``).
The parts of the call -- grid, link and union, census, second sort, reductions -- are kernel
times: ``--fold`` reads rocprofv3 kernel traces (``--kernel-trace --output-format csv``) of
``--only-metrics`` runs, takes per part and per kernel the median over the traced calls, and adds them to
that file (no GPU needed for this form).  Needs a GPU otherwise: there is no fallback.
"""

import argparse
import csv
import ctypes
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PLANES = {'sparse': None, 'packed': 0.5}         # agents per um^2; None: the whole plane
PARTS = ('grid', 'link_union', 'census', 'second_sort', 'reductions')
SEED = 20240229


def locations(n, nx, density, seed=SEED):
    """scripts/mechanics_timing.py's planes: uniform over a centred square of side sqrt(n / density)."""
    rng = np.random.default_rng(seed)
    side = float(nx) if density is None else min(float(nx), (n / density) ** 0.5)
    return (nx - side) / 2 + rng.uniform(0.0, side, (2, n))


def event_ms(fn, reps, warmup=3):
    import torch
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


def fold_trace(path):
    """Kernel time (ms) of each part of the call: the median over the calls of one trace.  A
    call begins with k_contact_cells; its kernels run in a fixed order, which tells the first
    sort (grid) from the second."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    calls, kernels, cur, part = [], [], None, None
    for r in rows:
        name, ms = r['Kernel_Name'], (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6
        if 'k_contact_cells' in name:
            cur, part = dict.fromkeys(PARTS, 0.0), 'grid'
            calls.append(cur)
            kernels.append({})
        elif cur is None or 'k_contact_relax' in name or 'k_contact_advance' in name:
            cur = None                       # a contact launch: not part of a metrics call
            continue
        elif 'k_colony_init' in name:
            part = 'link_union'
        elif 'k_colony_census' in name:
            part = 'census'
        elif 'k_occupancy_keys' in name and part == 'census':
            part = 'second_sort'
        elif 'k_colony_reduce' in name:
            part = 'reductions'
        elif part == 'reductions':
            continue                         # after the last pass: the next launch's flag clearing
        cur[part] += ms
        # per kernel too (a template's argument kept, arguments dropped; the sort's own kernels under one name)
        short = 'rocprim (sort)' if 'rocprim' in name else name.split('(')[0].replace('void ', '')
        kernels[-1][part + ': ' + short] = kernels[-1].get(part + ': ' + short, 0.0) + ms * 1e3
    kernels = [k for c, k in zip(calls, kernels) if c['reductions'] > 0.0]
    calls = [c for c in calls if c['reductions'] > 0.0]
    out = {p + '_ms': statistics.median(c[p] for c in calls) for p in PARTS} if calls else {}
    out['calls_traced'] = len(calls)
    if calls:
        out['kernel_total_ms'] = statistics.median(sum(c.values()) for c in calls)
        out['dominant_part'] = max(PARTS, key=lambda p: out[p + '_ms'])
        out['kernel_us'] = {k: round(statistics.median(c.get(k, 0.0) for c in kernels), 1) for k in kernels[0]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1_000_000)
    ap.add_argument('--nx', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'colony_metrics_timing.json'))
    ap.add_argument('--only-metrics', action='store_true', help='run reps x the call on --plane and exit')
    ap.add_argument('--plane', choices=sorted(PLANES), default='packed')
    ap.add_argument('--fold', nargs='*', default=[], metavar='PLANE=TRACE.csv')
    args = ap.parse_args()

    if args.fold:
        res = json.load(open(args.out))
        for item in args.fold:
            plane, path = item.split('=', 1)
            res['planes'][plane]['kernel_ms_by_part_from_trace'] = fold_trace(path)
        json.dump(res, open(args.out, 'w'), indent=1)
        print(json.dumps(res))
        return

    import torch
    from lens_amd import native
    from lens_amd.colonies import ColonyShape, ColonyShapeModel
    from lens_amd.mechanics import ContactBuffers, ContactModel
    if not torch.cuda.is_available():
        raise SystemExit('colony_metrics_timing: needs a GPU')
    dev = torch.device('cuda', 0)
    native.load()
    n, nx = args.agents, args.nx
    bounds = (float(nx), float(nx))
    rng = np.random.default_rng(SEED + 1)
    angle = torch.from_numpy(rng.uniform(0.0, 2.0 * np.pi, n)).to(dev)
    loc = torch.zeros((2, n), dtype=torch.float64, device=dev)
    shape = ColonyShape(ColonyShapeModel(), bounds, n, dev, length=2.0, mass=1339.0)      # gap 0.5, 3 cells
    labels = ColonyShape(ColonyShapeModel(), bounds, n, dev, length=2.0, mass=1339.0, labels_only=True)
    contact = ContactModel(iterations=1, jitter=0.01, jitter_angle=0.02, seed=SEED)
    cp = contact.vk_params(bounds)
    buf = ContactBuffers(n, cp.gx * cp.gy, dev)
    loc_c, angle_c = loc.clone(), angle.clone()
    bin_lin = torch.zeros(n, dtype=torch.int32, device=dev)

    def contact_iteration():
        native.check(native._lib.vk_contact_step(
            ctypes.byref(cp), n, n, native.ptr(loc_c), native.ptr(angle_c), 0, 0, native.ptr(buf.counter),
            native.ptr(buf.flags), nx, nx, bounds[0], bounds[1], native.ptr(bin_lin), 0,
            buf.scratch.data_ptr() + buf._off, buf._bytes, native.stream_handle()), 'vk_contact_step')

    if args.only_metrics:
        loc.copy_(torch.from_numpy(locations(n, nx, PLANES[args.plane])))
        event_ms(lambda: shape.launch(n, loc, angle), args.reps)
        shape.check()
        return

    res = {'agents': n, 'plane_um': [nx, nx], 'capsule_um': [2.0, 1.0], 'link_gap_um': 0.5, 'min_cells': 3,
           'grid': list(shape.model.grid(bounds)), 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'planes': {}}
    for plane, density in PLANES.items():
        loc.copy_(torch.from_numpy(locations(n, nx, density)))
        entry = {'agents_per_um2': n / float(nx) ** 2 if density is None else density}
        entry['colony_metrics'] = summary(event_ms(lambda: shape.launch(n, loc, angle), args.reps))
        entry['labels_only'] = summary(event_ms(lambda: labels.launch(n, loc, angle), args.reps))
        loc_c.copy_(loc)
        angle_c.copy_(angle)
        entry['contact_step_1_iteration'] = summary(event_ms(contact_iteration, args.reps))
        entry['ratio_to_contact_iteration'] = (entry['colony_metrics']['median_ms'] /
                                               entry['contact_step_1_iteration']['median_ms'])
        got = shape.result()
        entry['colonies'] = got.n_colonies
        entry['largest_colony_cells'] = int(got.cells.max()) if got.n_colonies else 0
        entry['agents_in_colonies'] = int((got.colony >= 0).sum())
        res['planes'][plane] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
