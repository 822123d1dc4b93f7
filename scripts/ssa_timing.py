"""Timing of the batched Gillespie step, and of what it must leave alone.

    python scripts/ssa_timing.py [--parent-lib PATH] [--rounds 3] > profiles/ssa_timing.json

1M agents, dt = 1 s, one MI355X.  Every figure is HIP events around the launches (or the
graph replay), after a warm-up, as the median of 20 with min and max, in ms:
  (a) idle            a step of the reference's complexation network
                      (tests/golden/flagella_complexation.json) in which no agent fires: the
                      monomers are exhausted (the burst's end state).  The kernel reads the 37
                      count rows and writes the events row; beside it vk_copy_stream over the
                      2 x 37 x 4 B per agent a kernel that also wrote the counts would move;
  (b) burst           the step from 1000 of every monomer: 573 events per agent (the counts
                      are restored before every timed launch, outside the timing);
  (c) birth_death     0 -> X at 50 / s, X -> 0 at 0.5 / s per molecule from X = 100: about 100
                      events per agent-step, as events per second; and the mean over waves of
                      (mean events / max events within the wave) from events_out -- the share
                      of the wave's event loop an average lane uses, the cost of the
                      lane-per-agent shape;
  (d) step_flagella   the replayed step of a motile colony WITHOUT stochastic=; with
                      ``--parent-lib`` (the library built from the parent commit) also with
                      that library, alternating with this tree's, each measurement in a
                      process of its own.
Prints one JSON line.
"""

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N, NX, BOUND, DT, REPS, WARMUP = 1 << 20, 4096, 8192.0, 1.0, 20, 3
COPY_FLOOR_BYTES_PER_S = 6.3e12
FIXTURE = os.path.join(REPO, 'tests', 'golden', 'flagella_complexation.json')


def summary(ms):
    ms = sorted(ms)
    return {'median_ms': round(0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]), 4), 'min_ms': round(ms[0], 4),
            'max_ms': round(ms[-1], 4)}


def timed(fn, before=None):
    import torch
    for _ in range(WARMUP):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return summary(out)


def load(lib):
    import torch  # noqa: F401  -- before any library: both bind to the HIP runtime torch ships
    from lens_amd import native
    if lib:
        # the parent's library lacks this tree's newest exports
        import ctypes
        have = ctypes.CDLL(lib)
        for name in [s for s in native._SIGS if not hasattr(have, s)]:
            native._SIGS.pop(name)
    native.load(lib or native.LIB_PATH)


def colony():
    import numpy as np
    import torch
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
    model = MotilityModel(initial_ligand=1e-2, substeps=10, seed=3, flagella=FlagellaModel(5))
    params, conc = configs.heterogeneous_colony(t, cfg, N)
    col = Colony(cfg, N, device=dev, integrator='dopri5', environment=lat, table=t, motility=model)
    col.set_agents(params=params, conc=conc, location=rng.uniform(0.0, BOUND, (2, N)))
    col.gather_external()
    return col


def worker_step(args):
    load(args.lib)
    col = colony()
    col.step(DT)
    replay = col.capture(DT, 1)
    print(json.dumps({'step_flagella': timed(replay)}), flush=True)


def worker_ssa(args):
    import torch
    load(None)
    from lens_amd import native
    from lens_amd.stochastic import StochasticEngine, StochasticModel
    dev = torch.device('cuda', 0)
    with open(FIXTURE) as f:
        fx = json.load(f)
    species = fx['monomer_ids'] + fx['complex_ids']
    model = StochasticModel(species, fx['stoichiometry'], fx['rates'], initial={m: 1000 for m in fx['monomer_ids']},
                            seed=11)
    eng = StochasticEngine(model, dev)
    S = model.n_species
    start = torch.from_numpy(model.initial_counts(N, N)).to(dev)
    x = start.clone()
    keys = torch.arange(N, dtype=torch.int64, device=dev)
    events = torch.zeros(N, dtype=torch.int32, device=dev)
    status = torch.zeros(N, dtype=torch.int32, device=dev)
    step = lambda: eng.step(DT, x, keys, N, events=events, status=status)
    out = {}

    # (b) the burst, the counts restored before every launch
    burst = timed(step, before=lambda: x.copy_(start))
    per_agent = events.to(torch.int64).sum().item() / N
    burst.update(events_per_agent=per_agent, events_per_s=round(per_agent * N / (burst['median_ms'] * 1e-3), 1))
    out['burst'] = burst

    # (a) nothing fires from the burst's end state
    idle = timed(step)
    assert int(events.sum()) == 0 and int(status.sum()) == 0
    nbytes = N * 2 * S * 4
    src = x.view(torch.float64).reshape(-1)                  # the same bytes as doubles: S * N / 2 of them
    dst = torch.empty_like(src)
    copy = timed(lambda: native.check(native._lib.vk_copy_stream(native.ptr(src), native.ptr(dst), src.numel(),
                                                                 native.stream_handle()), 'vk_copy_stream'))
    idle.update(bytes_read=N * (S * 4 + 8), bytes_written=N * 4)
    out['idle'] = idle
    out['copy_2x37x4B'] = dict(copy, bytes=nbytes, floor_ms=round(nbytes / COPY_FLOOR_BYTES_PER_S * 1e3, 4))
    out['idle_over_copy'] = round(idle['median_ms'] / copy['median_ms'], 3)

    # (c) birth-death at its steady state: about 100 events per agent-step
    bd = StochasticEngine(StochasticModel(['X'], {'birth': {'X': 1}, 'death': {'X': -1}},
                                          {'birth': 50.0, 'death': 0.5}, seed=12), dev)
    xb = torch.full((1, N), 100, dtype=torch.int32, device=dev)
    total = []

    def bd_step():
        bd.step(DT, xb, keys, N, events=events, status=status)
        total.append(events.to(torch.int64).sum())

    t = timed(bd_step)
    per_agent = float(torch.stack(total[WARMUP:]).double().mean().item()) / N
    ev = events.reshape(-1, 64).double()
    t.update(events_per_agent=round(per_agent, 3), events_per_s=round(per_agent * N / (t['median_ms'] * 1e-3), 1),
             wave_efficiency=round(float((ev.mean(dim=1) / ev.max(dim=1).values.clamp(min=1.0)).mean().item()), 4))
    out['birth_death'] = t
    assert int(status.sum()) == 0
    print(json.dumps({'ssa': out}), flush=True)


def child(*argv):
    res = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(argv), check=True, stdout=subprocess.PIPE,
                         timeout=600)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent-lib', default=None)
    p.add_argument('--rounds', type=int, default=3, help='alternations of tree and parent (d)')
    p.add_argument('--worker', default=None, choices=['step', 'ssa'])
    p.add_argument('--lib', default=None)
    args = p.parse_args()
    if args.worker:
        return {'step': worker_step, 'ssa': worker_ssa}[args.worker](args)
    out = {'agents': N, 'bins': [NX, NX], 'dt': DT, 'reps': REPS, 'warmup': WARMUP,
           'tree': {'step_flagella': []}, 'parent': {'step_flagella': []}}
    out['tree'].update(child('--worker', 'ssa'))
    for r in range(args.rounds if args.parent_lib else 1):
        if args.parent_lib:
            out['parent']['step_flagella'].append(child('--worker', 'step', '--lib', args.parent_lib)['step_flagella'])
        out['tree']['step_flagella'].append(child('--worker', 'step')['step_flagella'])
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
