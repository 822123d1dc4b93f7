"""Timing of the transcription step, and of what it must leave alone.

    python scripts/transcription_timing.py [--parent-lib PATH] [--rounds 3] > profiles/transcription_timing.json

1M agents, one MI355X.  Every figure is HIP events around the launch (or the graph replay),
after a warm-up, as the median of 20 with min and max, in ms:
  (a) flagella_1s     vk_transcription_step of the flagella fixture
                      (tests/golden/flagella_transcription.json: 15 promoters, 36 927 bases over
                      a seeded synthetic genome), 100 RNAPs per agent at random places, every
                      factor above its thresholds, 10 free RNAPs, pools that never run out,
                      T = 1 s: 50 elongating sub-intervals.  The state is restored before every
                      timed launch, outside the timing.  Elongations per second from the ADP made;
  (b) flagella_10s    the same at T = 10 s (the reference's compartment step): 500 elongating
                      sub-intervals;
  (a', b')            the same two with the sequence staged in LDS at 2 bits per base
                      (TranscriptionModel(sequence_path='lds')); (a) and (b) run sequence_path='auto', which
                      for this fixture reads the global byte table (the staged words would cost a
                      wave of occupancy);
  (c) idle            empty lists, no free RNAP: nothing is bound and nothing initiates;
  each beside vk_copy_stream over the bytes the launch must move (the list and its length in
  and out, the molecule rows in and out, the factor rows in, the free RNAPs in and out,
  mmol_to_counts and keys in, events out), timed in the same run;
  (d) translation     scripts/translation_timing.py's (a)-(c), vk_translation_step on its own
                      fixture, in the same run: the yardstick of the same dependent-chain structure;
  (e) step_flagella   the replayed step of a motile colony with stochastic= and translation= and
                      WITHOUT transcription=; with ``--parent-lib`` (the library built from the
                      parent commit) also with that library, alternating with this tree's, each
                      measurement in a process of its own.
``--worker once`` runs (b) once, for a counter run of its own.
Prints one JSON line.
"""

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'scripts'))

import translation_timing as tlt  # noqa: E402
from ssa_timing import DT, N, load, timed  # noqa: E402

FIXTURE = os.path.join(REPO, 'tests', 'golden', 'flagella_transcription.json')
RNAPS, CAP, FREE = 100, 128, 10


def child(*argv):
    import subprocess
    res = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(argv), check=True, stdout=subprocess.PIPE,
                         timeout=900)
    print('done:', ' '.join(argv), file=sys.stderr, flush=True)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def worker_step(args):
    """The motile colony of translation_timing with translation= beside the network, no transcription=."""
    load(args.lib)
    from lens_amd import configs
    from lens_amd.stochastic import StochasticModel
    with open(tlt.FIXTURE) as f:
        data = json.load(f)
    operons = [o for o in dict.fromkeys(o for o, _ in data['transcripts']) if o != 'fliE']
    tm = configs.flagella_translation(data, operons=operons, max_ribosomes=tlt.CAP, seed=7)
    sm = StochasticModel(tm.species() + ['sink'], {'none': {'sink': 1}}, {'none': 0.0}, seed=11)
    col = colony_with_translation(sm, tm)
    assert getattr(col, 'transcription', None) is None and col.translation is tm
    col.step(DT)
    replay = col.capture(DT, 1)
    print(json.dumps({'step_flagella': timed(replay)}), flush=True)


def colony_with_translation(sm, tm):
    import numpy as np
    import torch
    from lens_amd import configs
    from lens_amd.colony import Colony
    from lens_amd.lattice import Lattice
    from lens_amd.motility import FlagellaModel, MotilityModel
    from lens_amd.rate_law_compiler import compile_rate_laws
    from ssa_timing import BOUND, NX
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
    col = Colony(cfg, N, device=dev, integrator='dopri5', environment=lat, table=t, motility=model, stochastic=sm,
                 translation=tm)
    col.set_agents(params=params, conc=conc, location=rng.uniform(0.0, BOUND, (2, N)))
    col.gather_external()
    for o in tm.operons:
        col.ssa[sm.index(tm.transcript_species[o]), :N] = 2
    col.ssa[sm.index('Ribosome'), :N] = 20
    col.set_translation_molecules(ATP=10 ** 9, **{name: 10 ** 6 for name in tm.monomer_ids})
    return col


def worker_transcription(args):
    import numpy as np
    import torch
    load(None)
    from lens_amd import configs, native
    from lens_amd.stochastic import StochasticModel
    from lens_amd.transcription import TranscriptionEngine
    dev = torch.device('cuda', 0)
    with open(FIXTURE) as f:
        data = json.load(f)
    models = {mode: configs.flagella_transcription(data, max_rnaps=CAP, seed=7, sequence_path=mode)
              for mode in ('auto', 'lds')}
    tm = models['auto']
    sm = StochasticModel(tm.species() + ['sink'], {'none': {'sink': 1}}, {'none': 0.0})
    engines = {mode: TranscriptionEngine(m, sm, dev) for mode, m in models.items()}
    P, R, S = tm.n_templates, len(tm.molecule_ids), sm.n_species
    rng = np.random.default_rng(5)
    lengths = np.array([tm.length(t) for t in range(P)], dtype=np.int32)
    t = rng.integers(0, P, (RNAPS, N), dtype=np.int32)
    p = (rng.random((RNAPS, N), dtype=np.float32) * (lengths[t] - 1)).astype(np.int32)
    words = (p << 9) | (t << 1) | (p < tm.polymerase_occlusion)          # one terminator each: index 0
    slots0 = torch.zeros((CAP, N), dtype=torch.int32, device=dev)
    slots0[:RNAPS] = torch.from_numpy(words).to(dev)
    del t, p, words
    count0 = torch.full((N,), RNAPS, dtype=torch.int32, device=dev)
    mol0 = torch.full((R, N), 10 ** 7, dtype=torch.int32, device=dev)
    mol0[tm.atp_row], mol0[tm.adp_row] = 10 ** 9, 0
    x0 = torch.zeros((S, N), dtype=torch.int32, device=dev)
    for f in tm.factors_used():
        x0[sm.index(f)] = 100                                             # 1.4e-4 mM: over every threshold
    x0[sm.index('RNA Polymerase')] = FREE
    m2c = torch.full((N,), 7.33e5, dtype=torch.float64, device=dev)      # 1339 fg
    slots, count, mol, x = slots0.clone(), count0.clone(), mol0.clone(), x0.clone()
    keys = torch.arange(N, dtype=torch.int64, device=dev)
    events = torch.zeros(N, dtype=torch.int32, device=dev)
    status = torch.zeros(N, dtype=torch.int32, device=dev)

    def restore():
        slots.copy_(slots0), count.copy_(count0), mol.copy_(mol0), x.copy_(x0)

    if args.worker == 'once':
        engines['auto'].plan(10.0)
        engines['auto'].step(10.0, slots, count, mol, x, m2c, keys, N, events=events, status=status)
        torch.cuda.synchronize()
        return

    def copy_of(nbytes):
        src = torch.empty(nbytes // 16, dtype=torch.float64, device=dev)      # nbytes moved: half in, half out
        dst = torch.empty_like(src)
        c = timed(lambda: native.check(native._lib.vk_copy_stream(native.ptr(src), native.ptr(dst), src.numel(),
                                                                  native.stream_handle()), 'vk_copy_stream'))
        return dict(c, bytes=nbytes)

    out = {'promoters': P, 'molecule_rows': R, 'species': S, 'rnaps_per_agent': RNAPS, 'max_rnaps': CAP,
           'bases': int(lengths.sum()), 'affinity_entries': len(tm.affinity)}
    factors = len(tm.factors_used())
    moved = N * (2 * 4 * (RNAPS + 1 + R) + 4 * factors + 8 + 8 + 8 + 4)
    for name, dt, mode in (('flagella_1s', 1.0, 'auto'), ('flagella_10s', 10.0, 'auto'),
                           ('flagella_1s_lds_sequence', 1.0, 'lds'), ('flagella_10s_lds_sequence', 10.0, 'lds')):
        eng = engines[mode]
        eng.plan(dt)
        r = timed(lambda: eng.step(dt, slots, count, mol, x, m2c, keys, N, events=events, status=status), before=restore)
        torch.cuda.synchronize()
        assert int(status.sum()) == 0
        elongations = int(mol[tm.adp_row].to(torch.int64).sum().item())
        r.update(sub_intervals=len(tm.plan(dt)), elongations_per_agent=round(elongations / N, 2),
                 elongations_per_s=round(elongations / (r['median_ms'] * 1e-3), 1),
                 initiations_per_agent=round(events.to(torch.int64).sum().item() / N, 3),
                 rnaps_left_per_agent=round(count.to(torch.int64).sum().item() / N, 2))
        out[name] = r
    out['copy_list'] = copy_of(moved)
    for name in ('flagella_1s', 'flagella_10s', 'flagella_1s_lds_sequence', 'flagella_10s_lds_sequence'):
        out[name]['over_copy'] = round(out[name]['median_ms'] / out['copy_list']['median_ms'], 2)
    # (c) nothing bound, nothing initiates
    slots.zero_(), count.zero_(), x.zero_(), mol.copy_(mol0)
    idle = timed(lambda: engines['auto'].step(1.0, slots, count, mol, x, m2c, keys, N, events=events, status=status))
    assert int(events.sum()) == 0 and int(status.sum()) == 0 and int(count.sum()) == 0
    out['idle'] = idle
    out['copy_idle'] = copy_of(N * (4 * (R + 1 + factors) + 8 + 8 + 8 + 4 + 4))
    out['idle']['over_copy'] = round(idle['median_ms'] / out['copy_idle']['median_ms'], 2)
    print(json.dumps({'transcription': out}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent-lib', default=None)
    p.add_argument('--rounds', type=int, default=3, help='alternations of tree and parent (e)')
    p.add_argument('--worker', default=None, choices=['step', 'transcription', 'once'])
    p.add_argument('--lib', default=None)
    p.add_argument('--skip-step', action='store_true', help='(a)-(d) only')
    args = p.parse_args()
    if args.worker:
        return {'step': worker_step, 'transcription': worker_transcription, 'once': worker_transcription}[args.worker](
            args)
    out = {'agents': N, 'dt': DT, 'tree': {'step_flagella': []}, 'parent': {'step_flagella': []}}
    out['tree'].update(child('--worker', 'transcription'))
    out['tree'].update(tlt.child('--worker', 'translation'))
    for r in range(0 if args.skip_step else (args.rounds if args.parent_lib else 1)):
        if args.parent_lib:
            out['parent']['step_flagella'].append(child('--worker', 'step', '--lib', args.parent_lib)['step_flagella'])
        out['tree']['step_flagella'].append(child('--worker', 'step')['step_flagella'])
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
