"""Timing of the motile colony's new launches at the C4 size (the
motility section): 1M agents on 4096^2 bins, dt = 1 s, 10 inner motility updates.

    python scripts/motility_timing.py [--agents N] [--nx NX] [--reps R]

HIP-event times (median of R repetitions after a warmup) of
  (a) the motility launch (vk_motility_step),
  (b) the device re-binning: vk_occupancy_sort + vk_exchange_ordered,
  (c) the host route to the same state: Colony.refresh_bins() (two torch sorts,
      unique_consecutive, host reads) + vk_exchange_sorted -- host wall clock
      around a synchronise, since the route itself synchronises,
and the step time of a C4-like colony (glc_ac kinetics, the bench's stencil
settings, three planes) with and without motility, replayed from captured
graphs, alternating.  Prints one JSON line.  Needs a GPU: there is no fallback.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lens_amd import configs                                      # noqa: E402
from lens_amd.colony import Colony                                # noqa: E402
from lens_amd.lattice import Lattice, stencil_depth, stencil_kernel, stencil_mode   # noqa: E402
from lens_amd.motility import MotilityModel                       # noqa: E402
from lens_amd.rate_law_compiler import compile_rate_laws          # noqa: E402

SUBSTEPS = 10


def build(dev, n, nx, motile):
    cfg = configs.glc_ac_config()
    table = compile_rate_laws(cfg['reactions'], cfg['kinetic_parameters'])
    rng = np.random.default_rng(configs.SEED)
    x = np.linspace(0.0, 1.0, nx)
    lat = Lattice(['glc__D_e', 'ac_e', 'MeAsp'], (nx, nx), (float(nx), float(nx)), 10.0, 5.0, device=dev,
                  initial={'glc__D_e': configs.gaussian_bump_field((nx, nx)), 'ac_e': np.zeros((nx, nx)),
                           'MeAsp': 0.2 * x[:, None] + 0.05 * x[None, :] ** 2})
    params, conc = configs.heterogeneous_colony(table, cfg, n, seed=configs.SEED)
    model = MotilityModel(initial_ligand=0.1, substeps=SUBSTEPS, seed=configs.SEED) if motile else None
    col = Colony(cfg, n, device=dev, integrator='dopri5', environment=lat, table=table, specialize=True,
                 motility=model)
    col.set_agents(params=params, conc=conc, location=rng.uniform(0.0, float(nx), (2, n)))
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


def wall_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1_000_000)
    ap.add_argument('--nx', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--graph-steps', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('motility_timing: needs a GPU')
    dev = torch.device('cuda', 0)
    stencil_mode('fma'), stencil_depth(10), stencil_kernel(70, 64)     # the bench's C4 settings
    n = args.agents
    col = build(dev, n, args.nx, True)
    lat = col.lattice
    col.step(1.0)                                                    # loads every kernel
    res = {'agents': n, 'bins': [args.nx, args.nx], 'dt': 1.0, 'substeps': SUBSTEPS, 'reps': args.reps,
           'device': torch.cuda.get_device_name(0)}

    from lens_amd.motility import motility_step
    a = event_ms(lambda: motility_step(col.motility, lat, col.location, col.motil, n, 1.0, col._motil_counter,
                                       bin_lin=col.bin_lin, bin_ix=col.bin_ix), args.reps)
    res['a_motility_launch'] = summary(a)
    # algorithmic bytes: 9 state rows and 2 location rows read and written, the bins written,
    # one ligand value read per inner update
    nbytes = n * (9 * 8 * 2 + 2 * 8 * 2 + 2 * 4 + SUBSTEPS * 8)
    res['a_algorithmic_bytes'] = nbytes
    res['a_achieved_TB_per_s'] = nbytes / (np.median(a) * 1e-3) / 1e12

    def device_route():
        col._occ_dev.sort(col.bin_lin, n, lat.rows_local * lat.ny, None)
        lat.exchange_ordered(col._occ_dev.order, col._occ_dev.sorted_bin, n, col.counts, col.map_exch_count,
                             col.map_exch_field)

    def host_route():
        col.refresh_bins()
        lat.exchange_sorted(col.occ, col.counts, col.map_exch_count, col.map_exch_field)

    res['b_device_rebin_exchange'] = summary(event_ms(device_route, args.reps))
    res['b_device_rebin_exchange_wall'] = summary(wall_ms(device_route, args.reps))
    res['c_host_rebin_exchange_wall'] = summary(wall_ms(host_route, args.reps))

    plain = build(dev, n, args.nx, False)
    plain.step(1.0)
    k = args.graph_steps
    replays = {'motile': col.capture(1.0, k), 'plain': plain.capture(1.0, k)}
    steps = {name: [] for name in replays}
    for name, r in replays.items():
        r()
    for _ in range(5):                                               # alternating
        for name, r in replays.items():
            steps[name] += [t / k for t in event_ms(r, 1, warmup=0)]
    res['step_ms_motile'] = summary(steps['motile'])
    res['step_ms_plain_three_planes'] = summary(steps['plain'])
    res['agents_with_status'] = int((col.status[:n] != 0).sum())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
