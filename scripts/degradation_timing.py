"""Timing of the RNA degradation step, and of what it must leave alone.

    python scripts/degradation_timing.py [--parent-lib PATH] [--rounds 3] > profiles/degradation_timing.json

1M agents, one MI355X.  Every figure is HIP events around the launch (or the graph replay),
after a warm-up, as the median of 20 with min and max, in ms:
  (a) flagella        vk_rna_degradation_step of the whole flagella chromosome
                      (configs.flagella_gene_expression(operons=None): 15 transcripts, one
                      endoRNAse, 77 rows), 0..5 of every transcript and 0..40 endoRNAses per agent,
                      T = 1 s, carries that differ from agent to agent.  The state is restored
                      before every timed launch, outside the timing;
      copy            vk_copy_stream over the bytes the launch must move, counted here from the
                      shapes: in, the 15 transcript rows (int32), the 15 carries (FP64), the enzyme
                      row, mmol_to_counts and the 5 pool rows; out, the 15 carries, the 15
                      transcript rows and the 5 pool rows (an upper bound: a count or a pool is
                      stored only where it changed) and ``degraded``;
  (b) step_flagella   the replayed step of a motile colony with stochastic=, translation= and
                      transcription= and WITHOUT degradation= and without passive=; with
                      ``--parent-lib`` (the library built from the parent commit) also with that
                      library, alternating with this tree's, each measurement in a process of its
                      own.  "Unchanged" holds if each median lies inside the other's min-max.
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
from ssa_timing import BOUND, DT, N, NX, load, timed  # noqa: E402

GOLDEN = os.path.join(REPO, 'tests', 'golden')
# what fits the 64 species of a table without passive rows beside the free ribosome, the free RNAP and the factors
OPERONS = ['flhDC', 'fliA', 'fliC', 'fliD', 'flgK', 'flgM', 'motA', 'tar', 'fliE', 'flgE']


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def child(*argv):
    import subprocess
    res = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(argv), check=True, stdout=subprocess.PIPE,
                         timeout=900)
    print('done:', ' '.join(argv), file=sys.stderr, flush=True)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def worker_step(args):
    """A motile colony with the network, translation and transcription on one table of active rows."""
    import numpy as np
    import torch
    load(args.lib)
    from lens_amd import configs
    from lens_amd.colony import Colony
    from lens_amd.lattice import Lattice
    from lens_amd.motility import FlagellaModel, MotilityModel
    from lens_amd.rate_law_compiler import compile_rate_laws
    from lens_amd.stochastic import StochasticModel
    tm = configs.flagella_transcription(golden('flagella_transcription.json'), operons=OPERONS, max_rnaps=32, seed=7)
    lm = configs.flagella_translation(golden('flagella_translation.json'), operons=OPERONS, max_ribosomes=tlt.CAP, seed=7)
    species = list(dict.fromkeys(tm.species() + lm.species() + ['sink']))
    sm = StochasticModel(species, {'none': {'sink': 1}}, {'none': 0.0}, seed=11)
    assert sm.n_rows == sm.n_species <= 64
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
                 translation=lm, transcription=tm)
    assert getattr(col, 'degradation', None) is None
    col.set_agents(params=params, conc=conc, location=rng.uniform(0.0, BOUND, (2, N)))
    col.gather_external()
    for name in tm.products:
        col.ssa[sm.index(name), :N] = 2
    for f in tm.factors_used():
        col.ssa[sm.index(f), :N] = 100
    col.ssa[sm.index('Ribosome'), :N] = 20
    col.ssa[sm.index('RNA Polymerase'), :N] = 10
    col.set_translation_molecules(ATP=10 ** 9, **{name: 10 ** 6 for name in lm.monomer_ids})
    col.set_transcription_molecules(ATP=10 ** 9, GTP=10 ** 7, UTP=10 ** 7, CTP=10 ** 7)
    col.step(DT)
    replay = col.capture(DT, 1)
    print(json.dumps({'step_flagella': timed(replay)}), flush=True)


def worker_degradation(args):
    import torch
    load(None)
    from lens_amd import configs, native
    from lens_amd.degradation import DegradationEngine
    dev = torch.device('cuda', 0)
    cfg = configs.flagella_gene_expression(golden('flagella_transcription.json'), golden('flagella_translation.json'),
                                           golden('flagella_complexation.json'), golden('flagella_degradation.json'))
    sm, tm, dm = cfg['stochastic'], cfg['transcription'], cfg['degradation']
    eng = DegradationEngine(dm, sm, tm, dev)
    trow, erow = dm.bind(sm, tm)
    T, E, R = dm.n_transcripts, dm.n_enzymes, len(dm.molecule_ids)
    g = torch.Generator(device=dev).manual_seed(5)
    x0 = torch.zeros((sm.n_rows, N), dtype=torch.int32, device=dev)
    x0[torch.from_numpy(trow).long().to(dev)] = torch.randint(0, 6, (T, N), generator=g, device=dev, dtype=torch.int32)
    x0[int(erow[0])] = torch.randint(0, 41, (N,), generator=g, device=dev, dtype=torch.int32)
    p0 = torch.rand((T, N), generator=g, device=dev, dtype=torch.float64)
    mol0 = torch.full((R, N), 5 * 10 ** 6, dtype=torch.int32, device=dev)
    m2c = torch.full((N,), 7.33e5, dtype=torch.float64, device=dev) * (
        1.0 + torch.rand(N, generator=g, device=dev, dtype=torch.float64))          # 1339 fg and up to twice that
    x, p, mol = x0.clone(), p0.clone(), mol0.clone()
    degraded = torch.zeros(N, dtype=torch.int32, device=dev)
    status = torch.zeros(N, dtype=torch.int32, device=dev)

    def restore():
        x.copy_(x0), p.copy_(p0), mol.copy_(mol0)

    r = timed(lambda: eng.step(DT, x, p, mol, m2c, N, degraded=degraded, status=status), before=restore)
    torch.cuda.synchronize()
    assert int(status.sum()) == 0
    r['degraded_per_agent'] = round(int(degraded.to(torch.int64).sum().item()) / N, 3)
    bytes_in = N * (4 * T + 8 * T + 4 * E + 8 + 4 * R)
    bytes_out = N * (8 * T + 4 * T + 4 * R + 4)
    moved = bytes_in + bytes_out
    src = torch.empty(moved // 16, dtype=torch.float64, device=dev)          # moved bytes: half in, half out
    dst = torch.empty_like(src)
    c = timed(lambda: native.check(native._lib.vk_copy_stream(native.ptr(src), native.ptr(dst), src.numel(),
                                                              native.stream_handle()), 'vk_copy_stream'))
    c.update(bytes=moved, bytes_in=bytes_in, bytes_out=bytes_out)
    r['over_copy'] = round(r['median_ms'] / c['median_ms'], 2)
    r['bytes_per_s'] = round(moved / (r['median_ms'] * 1e-3), 1)
    print(json.dumps({'degradation': {'transcripts': T, 'enzymes': E, 'pairs': dm.n_pairs, 'rows': sm.n_rows,
                                      'molecule_rows': R, 'flagella': r, 'copy': c}}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent-lib', default=None)
    p.add_argument('--rounds', type=int, default=3, help='alternations of tree and parent (b)')
    p.add_argument('--worker', default=None, choices=['step', 'degradation'])
    p.add_argument('--lib', default=None)
    p.add_argument('--skip-step', action='store_true', help='(a) only')
    args = p.parse_args()
    if args.worker:
        return {'step': worker_step, 'degradation': worker_degradation}[args.worker](args)
    out = {'agents': N, 'dt': DT, 'tree': {'step_flagella': []}, 'parent': {'step_flagella': []}}
    out['tree'].update(child('--worker', 'degradation'))
    for r in range(0 if args.skip_step else (args.rounds if args.parent_lib else 1)):
        if args.parent_lib:
            out['parent']['step_flagella'].append(child('--worker', 'step', '--lib', args.parent_lib)['step_flagella'])
        out['tree']['step_flagella'].append(child('--worker', 'step')['step_flagella'])
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
