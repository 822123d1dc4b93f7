"""Timing of the translation step, and of what it must leave alone.

    python scripts/translation_timing.py [--parent-lib PATH] [--rounds 3] > profiles/translation_timing.json

1M agents, one MI355X.  Every figure is HIP events around the launch (or the graph replay),
after a warm-up, as the median of 20 with min and max, in ms:
  (a) flagella_1s     vk_translation_step of the flagella fixture
                      (tests/golden/flagella_translation.json without the fliE operon, so that
                      its species fit one StochasticModel: 51 templates, 20 monomers; sequences
                      synthesised at the estimated lengths), 100 ribosomes per agent at random
                      places, two transcripts per operon, pools that never run out, T = 1 s: 22
                      elongating sub-intervals.  The state is restored before every timed
                      launch, outside the timing.  Elongations per second from the ATP spent;
  (b) flagella_10s    the same at T = 10 s: 219 elongating sub-intervals and a partial one;
  (c) idle            empty lists, no transcripts: nothing is bound and nothing initiates;
  each beside vk_copy_stream over the bytes the launch must move (the list and its length in
  and out, the monomer rows in and out, the operon rows in, the free ribosomes in and out,
  keys in, events out), timed in the same run;
  (d) step_flagella   the replayed step of a motile colony with stochastic= and WITHOUT
                      translation=; with ``--parent-lib`` (the library built from the parent
                      commit) also with that library, alternating with this tree's, each
                      measurement in a process of its own.
Prints one JSON line.
"""

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'scripts'))

from ssa_timing import BOUND, DT, N, NX, load, timed  # noqa: E402

FIXTURE = os.path.join(REPO, 'tests', 'golden', 'flagella_translation.json')
SSA_FIXTURE = os.path.join(REPO, 'tests', 'golden', 'flagella_complexation.json')
RIBOSOMES, CAP = 100, 128


def child(*argv):
    import subprocess
    res = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(argv), check=True, stdout=subprocess.PIPE,
                         timeout=900)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def colony(stochastic):
    """ssa_timing's motile colony, with a stochastic network beside it."""
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
    col = Colony(cfg, N, device=dev, integrator='dopri5', environment=lat, table=t, motility=model,
                 stochastic=stochastic)
    col.set_agents(params=params, conc=conc, location=rng.uniform(0.0, BOUND, (2, N)))
    col.gather_external()
    return col


def worker_step(args):
    load(args.lib)
    from lens_amd.stochastic import StochasticModel
    with open(SSA_FIXTURE) as f:
        fx = json.load(f)
    model = StochasticModel(fx['monomer_ids'] + fx['complex_ids'], fx['stoichiometry'], fx['rates'],
                            initial={m: 100 for m in fx['monomer_ids']}, seed=11)
    col = colony(model)
    assert getattr(col, 'translation', None) is None
    col.step(DT)
    replay = col.capture(DT, 1)
    print(json.dumps({'step_flagella': timed(replay)}), flush=True)


def worker_translation(args):
    import numpy as np
    import torch
    load(None)
    from lens_amd import configs, native
    from lens_amd.stochastic import StochasticModel
    from lens_amd.translation import TranslationEngine
    dev = torch.device('cuda', 0)
    with open(FIXTURE) as f:
        data = json.load(f)
    operons = [o for o in dict.fromkeys(o for o, _ in data['transcripts']) if o != 'fliE']
    tm = configs.flagella_translation(data, operons=operons, max_ribosomes=CAP, seed=7)
    sm = StochasticModel(tm.species() + ['sink'], {'none': {'sink': 1}}, {'none': 0.0})
    eng = TranslationEngine(tm, sm, dev)
    T, M, S = tm.n_templates, tm.n_monomers, sm.n_species
    rng = np.random.default_rng(5)
    lengths = np.array([tm.length(t) for t in range(T)], dtype=np.int32)
    t = rng.integers(0, T, (RIBOSOMES, N), dtype=np.int32)
    p = (rng.random((RIBOSOMES, N), dtype=np.float32) * (lengths[t] - 1)).astype(np.int32)
    words = (p << 7) | (t << 1) | (p < tm.polymerase_occlusion)
    slots0 = torch.zeros((CAP, N), dtype=torch.int32, device=dev)
    slots0[:RIBOSOMES] = torch.from_numpy(words).to(dev)
    del t, p, words
    count0 = torch.full((N,), RIBOSOMES, dtype=torch.int32, device=dev)
    mol0 = torch.full((M + 2, N), 10 ** 6, dtype=torch.int32, device=dev)
    mol0[M], mol0[M + 1] = 10 ** 9, 0
    x0 = torch.zeros((S, N), dtype=torch.int32, device=dev)
    for o in operons:
        x0[sm.index(tm.transcript_species[o])] = 2
    slots, count, mol, x = slots0.clone(), count0.clone(), mol0.clone(), x0.clone()
    keys = torch.arange(N, dtype=torch.int64, device=dev)
    events = torch.zeros(N, dtype=torch.int32, device=dev)
    status = torch.zeros(N, dtype=torch.int32, device=dev)

    def restore():
        slots.copy_(slots0), count.copy_(count0), mol.copy_(mol0), x.copy_(x0)

    def copy_of(nbytes):
        src = torch.empty(nbytes // 16, dtype=torch.float64, device=dev)      # nbytes moved: half in, half out
        dst = torch.empty_like(src)
        c = timed(lambda: native.check(native._lib.vk_copy_stream(native.ptr(src), native.ptr(dst), src.numel(),
                                                                  native.stream_handle()), 'vk_copy_stream'))
        return dict(c, bytes=nbytes)

    out = {'templates': T, 'monomers': M, 'species': S, 'ribosomes_per_agent': RIBOSOMES, 'max_ribosomes': CAP,
           'residues': int(lengths.sum())}
    moved = N * (2 * 4 * (RIBOSOMES + 1 + M + 2) + 4 * len(operons) + 8 + 8 + 4)
    for name, dt in (('flagella_1s', 1.0), ('flagella_10s', 10.0)):
        eng.plan(dt)
        r = timed(lambda: eng.step(dt, slots, count, mol, x, keys, N, events=events, status=status), before=restore)
        torch.cuda.synchronize()
        assert int(status.sum()) == 0
        elongations = int((mol0[M].to(torch.int64) - mol[M].to(torch.int64)).sum().item()) // 2
        r.update(sub_intervals=len(tm.plan(dt)), elongations_per_agent=round(elongations / N, 2),
                 elongations_per_s=round(elongations / (r['median_ms'] * 1e-3), 1),
                 initiations_per_agent=round(events.to(torch.int64).sum().item() / N, 3),
                 ribosomes_left_per_agent=round(count.to(torch.int64).sum().item() / N, 2))
        out[name] = r
    out['copy_list'] = copy_of(moved)
    for name in ('flagella_1s', 'flagella_10s'):
        out[name]['over_copy'] = round(out[name]['median_ms'] / out['copy_list']['median_ms'], 2)
    # (c) nothing bound, nothing initiates
    slots.zero_(), count.zero_(), x.zero_(), mol.copy_(mol0)
    idle = timed(lambda: eng.step(1.0, slots, count, mol, x, keys, N, events=events, status=status))
    assert int(events.sum()) == 0 and int(status.sum()) == 0 and int(count.sum()) == 0
    out['idle'] = idle
    out['copy_idle'] = copy_of(N * (4 * (M + 1 + len(operons)) + 8 + 8 + 4 + 4))
    out['idle']['over_copy'] = round(idle['median_ms'] / out['copy_idle']['median_ms'], 2)
    print(json.dumps({'translation': out}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent-lib', default=None)
    p.add_argument('--rounds', type=int, default=3, help='alternations of tree and parent (d)')
    p.add_argument('--worker', default=None, choices=['step', 'translation'])
    p.add_argument('--lib', default=None)
    p.add_argument('--skip-step', action='store_true', help='(a)-(c) only')
    args = p.parse_args()
    if args.worker:
        return {'step': worker_step, 'translation': worker_translation}[args.worker](args)
    out = {'agents': N, 'dt': DT, 'tree': {'step_flagella': []}, 'parent': {'step_flagella': []}}
    out['tree'].update(child('--worker', 'translation'))
    for r in range(0 if args.skip_step else (args.rounds if args.parent_lib else 1)):
        if args.parent_lib:
            out['parent']['step_flagella'].append(child('--worker', 'step', '--lib', args.parent_lib)['step_flagella'])
        out['tree']['step_flagella'].append(child('--worker', 'step')['step_flagella'])
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
