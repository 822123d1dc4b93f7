"""Timing of the motile-agent launches: the flagella launch against the coarse one.

    python scripts/flagella_timing.py [--parent-lib PATH] > profiles/flagella_timing.json

1M agents on a 4096 x 4096 plane, dt = 1 s.  Every figure is HIP events around the launch
(or the graph replay), after a warm-up, as the median of 20 with min and max, in ms:
  - the flagella launch at 10 and at 100 inner updates, for 5 flagella per agent, for 32,
    and for counts mixed 0..32 within every wave;
  - the coarse launch at 10 inner updates;
  - a colony step on three planes (glc__D_e, lcts_e, MeAsp; glc_lct kinetics, DP45)
    replayed from a graph, with the coarse motor and with the flagella motor.
With ``--parent-lib`` (the library built from the parent commit) the coarse launch and the
coarse step are also measured with that library, alternating with this tree's, each
measurement in a process of its own (two libraries with the same symbols do not share a
process).  Prints one JSON line.
"""

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N, NX, BOUND, DT, REPS, WARMUP = 1 << 20, 4096, 8192.0, 1.0, 20, 3


def summary(ms):
    ms = sorted(ms)
    return {'median_ms': round(0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]), 4), 'min_ms': round(ms[0], 4),
            'max_ms': round(ms[-1], 4)}


def timed(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return summary(out)


def load(lib):
    from lens_amd import native
    if lib:
        # the parent's library lacks this tree's newest export
        import ctypes
        have = ctypes.CDLL(lib)
        for name in [s for s in native._SIGS if not hasattr(have, s)]:
            native._SIGS.pop(name)
    native.load(lib or native.LIB_PATH)


def worker_launch(args):
    import numpy as np
    import torch
    load(args.lib)
    from lens_amd.lattice import Lattice
    from lens_amd.motility import FlagellaModel, MotilityModel, flagella_step, motility_step
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(1)
    x = np.linspace(0.0, 1.0, NX)
    lat = Lattice(['MeAsp'], (NX, NX), (BOUND, BOUND), 10.0, 5.0, device=dev,
                  initial={'MeAsp': 0.2 * x[:, None] + 0.05 * x[None, :] ** 2})
    loc0 = torch.from_numpy(rng.uniform(0.0, BOUND, (2, N))).to(dev)
    bins = torch.zeros(N, dtype=torch.int32, device=dev)
    out = {}

    def coarse():
        model = MotilityModel(initial_ligand=1e-2, substeps=10, seed=3)
        motil = torch.from_numpy(model.initial_rows(N, N)).to(dev)
        loc, counter = loc0.clone(), torch.zeros(1, dtype=torch.int64, device=dev)
        return timed(lambda: motility_step(model, lat, loc, motil, N, DT, counter, bin_lin=bins))

    out['coarse_10'] = coarse()
    for name, counts in (() if args.coarse_only else (('5', 5), ('32', 32), ('mixed', np.arange(N) % 33))):
        for substeps in (10, 100):
            model = MotilityModel(initial_ligand=1e-2, substeps=substeps, seed=3, flagella=FlagellaModel(counts))
            motil = torch.from_numpy(model.initial_rows(N, N)).to(dev)
            flag, flag_int = (torch.from_numpy(a).to(dev) for a in model.flagella.initial_rows(N, N, 3))
            loc, counter = loc0.clone(), torch.zeros(1, dtype=torch.int64, device=dev)
            out['flagella_%s_%d' % (name, substeps)] = timed(
                lambda: flagella_step(model, lat, loc, motil, flag, flag_int, N, DT, counter, bin_lin=bins))
    print(json.dumps(out), flush=True)


def worker_step(args):
    import numpy as np
    import torch
    load(args.lib)
    from lens_amd import configs
    from lens_amd.colony import Colony
    from lens_amd.lattice import Lattice
    from lens_amd.motility import FlagellaModel, MotilityModel
    from lens_amd.rate_law_compiler import compile_rate_laws
    dev = torch.device('cuda', 0)
    cfg = configs.glc_lct_config()
    t = compile_rate_laws(cfg['reactions'], cfg['kinetic_parameters'])
    rng = np.random.default_rng(1)
    x = np.linspace(0.0, 1.0, NX)
    start = {'glc__D_e': configs.gaussian_bump_field((NX, NX)), 'lcts_e': np.full((NX, NX), 10.0),
             'MeAsp': 0.2 * x[:, None] + 0.05 * x[None, :] ** 2}
    lat = Lattice(['glc__D_e', 'lcts_e', 'MeAsp'], (NX, NX), (BOUND, BOUND), 10.0, 5.0, device=dev, initial=start)
    flagella = FlagellaModel(5) if args.worker == 'step_flagella' else None
    model = MotilityModel(initial_ligand=1e-2, substeps=10, seed=3, flagella=flagella)
    params, conc = configs.heterogeneous_colony(t, cfg, N)
    col = Colony(cfg, N, device=dev, integrator='dopri5', environment=lat, table=t, motility=model)
    col.set_agents(params=params, conc=conc, location=rng.uniform(0.0, BOUND, (2, N)))
    col.gather_external()
    col.step(DT)
    replay = col.capture(DT, 1)
    print(json.dumps({args.worker: timed(replay)}), flush=True)


def child(*argv):
    res = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(argv), check=True, stdout=subprocess.PIPE,
                         timeout=600)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent-lib', default=None)
    p.add_argument('--rounds', type=int, default=3, help='alternations of tree and parent')
    p.add_argument('--worker', default=None, choices=['launch', 'step_coarse', 'step_flagella'])
    p.add_argument('--lib', default=None)
    p.add_argument('--coarse-only', action='store_true')
    args = p.parse_args()
    if args.worker == 'launch':
        return worker_launch(args)
    if args.worker:
        return worker_step(args)
    out = {'agents': N, 'bins': [NX, NX], 'dt': DT, 'reps': REPS, 'warmup': WARMUP,
           'tree': {'coarse_10': [], 'step_coarse': []}, 'parent': {'coarse_10': [], 'step_coarse': []}}
    out['tree'].update(child('--worker', 'launch'))
    out['tree']['coarse_10'] = [out['tree']['coarse_10']]
    rounds = args.rounds if args.parent_lib else 0
    for r in range(rounds):
        out['parent']['coarse_10'].append(child('--worker', 'launch', '--coarse-only', '--lib', args.parent_lib)['coarse_10'])
        if r + 1 < rounds:
            out['tree']['coarse_10'].append(child('--worker', 'launch', '--coarse-only')['coarse_10'])
    for r in range(max(rounds, 1)):
        out['tree']['step_coarse'].append(child('--worker', 'step_coarse')['step_coarse'])
        if args.parent_lib:
            out['parent']['step_coarse'].append(child('--worker', 'step_coarse', '--lib', args.parent_lib)['step_coarse'])
    out['tree'].update(child('--worker', 'step_flagella'))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
