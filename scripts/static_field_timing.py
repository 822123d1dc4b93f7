"""Timing of the static-field launches, each against a floor or a twin timed
in the same run:

    python scripts/static_field_timing.py [--agents N] [--nx NX] [--reps R] [--out FILE]

  (a) the motile launches at the C4 size -- 1M agents on 4096^2 bins, 10 inner updates --
      sensing a plane (vk_motility_step, vk_flagella_step with 5 flagella) and sensing an
      analytic gradient (the _static launches; exponential and linear), alternating, every
      variant on its own copy of the same states;
  (b) vk_gradient_fill on one 4096^2 plane and vk_static_gather for 1M agents x 2 molecules,
      as a fraction of vk_copy_stream's rate over their written-plus-read bytes;
  (c) a whole step of a non-motile colony in a static field against the same colony on
      'held' (the difference is the gather), replayed from captured graphs, alternating;
  (d) one run of the reference experiment's shape: chemotaxis_static('exponential'), 4096
      agents, 60 s, the mean displacement along y -- beside the same colony in a flat field
      (base 1, so base ** d = 1, scaled to the same ligand at the start).  Recorded, not
      asserted: the kinematics are this engine's.

HIP-event times, median and min-max of R repetitions after a warmup.  Prints one JSON line
(and writes it to --out).  Needs a GPU: there is no fallback.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lens_amd import configs, native                                                 # noqa: E402
from lens_amd.colony import Colony                                                   # noqa: E402
from lens_amd.lattice import Lattice                                                 # noqa: E402
from lens_amd.motility import FlagellaModel, MotilityModel, flagella_step, motility_step   # noqa: E402
from lens_amd.static_field import StaticField                                        # noqa: E402

SUBSTEPS = 10


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternating(fns, reps, warmup=3):
    """{name: [ms]}: the variants in turn, `reps` rounds after `warmup` rounds."""
    out = {name: [] for name in fns}
    for r in range(warmup + reps):
        for name, fn in fns.items():
            t = event_ms(fn)
            if r >= warmup:
                out[name].append(t)
    return out


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms))}


def launches(dev, n, nx, reps):
    rng = np.random.default_rng(configs.SEED)
    bound = float(nx)
    x = np.linspace(0.0, 1.0, nx)
    lat = Lattice(['MeAsp'], (nx, nx), (bound, bound), 10.0, 5.0, device=dev,
                  initial={'MeAsp': 0.2 * x[:, None] + 0.05 * x[None, :] ** 2})
    center = [0.5, 0.5]
    fields = {
        'exponential': StaticField(['MeAsp'], (bound, bound), {'type': 'exponential', 'molecules': {
            'MeAsp': {'center': center, 'base': 1.3e2, 'scale': 0.1}}}, n_bins=(nx, nx)),
        'linear': StaticField(['MeAsp'], (bound, bound), {'type': 'linear', 'molecules': {
            'MeAsp': {'center': center, 'base': 0.1, 'slope': 0.1}}}, n_bins=(nx, nx))}
    coarse = MotilityModel(initial_ligand=0.1, substeps=SUBSTEPS, seed=configs.SEED)
    flagella = MotilityModel(initial_ligand=0.1, substeps=SUBSTEPS, seed=configs.SEED, flagella=FlagellaModel(5))
    loc0 = torch.from_numpy(rng.uniform(0.0, bound, (2, n))).to(dev)
    motil0 = torch.from_numpy(coarse.initial_rows(n, n)).to(dev)
    flag0, flagi0 = (torch.from_numpy(a).to(dev) for a in flagella.flagella.initial_rows(n, n, configs.SEED))
    fns = {}

    def add(name, model, field):
        loc, motil, counter = loc0.clone(), motil0.clone(), torch.zeros(1, dtype=torch.int64, device=dev)
        bins = torch.zeros(n, dtype=torch.int32, device=dev)
        if model.flagella is None:
            fns[name] = lambda: motility_step(model, field, loc, motil, n, 1.0, counter, bin_lin=bins)
        else:
            flag, flagi = flag0.clone(), flagi0.clone()
            fns[name] = lambda: flagella_step(model, field, loc, motil, flag, flagi, n, 1.0, counter, bin_lin=bins)

    add('motility_plane', coarse, lat)
    add('motility_static_exponential', coarse, fields['exponential'])
    add('motility_static_linear', coarse, fields['linear'])
    add('flagella_plane', flagella, lat)
    add('flagella_static_exponential', flagella, fields['exponential'])
    res = {name: summary(ms) for name, ms in alternating(fns, reps).items()}
    for name in ('motility_static_exponential', 'motility_static_linear'):
        res[name]['ratio_to_plane'] = res[name]['median_ms'] / res['motility_plane']['median_ms']
    res['flagella_static_exponential']['ratio_to_plane'] = (res['flagella_static_exponential']['median_ms'] /
                                                            res['flagella_plane']['median_ms'])
    res['exponential_minus_linear_ms'] = (res['motility_static_exponential']['median_ms'] -
                                          res['motility_static_linear']['median_ms'])
    return res


def small_kernels(dev, n, nx, reps):
    lib = native.load()
    gradient = {'type': 'exponential', 'molecules': {'a': {'center': [0.5, 0.0], 'base': 1.3e2, 'scale': 4.0},
                                                     'b': {'center': [0.2, 0.6], 'base': 0.7}}}
    field = StaticField(['a', 'b'], (1000, 3000), gradient)
    rng = np.random.default_rng(configs.SEED)
    loc = torch.from_numpy(np.stack([rng.uniform(0, 1000, n), rng.uniform(0, 3000, n)])).to(dev)
    conc = torch.zeros((2, n), dtype=torch.float64, device=dev)
    src = torch.zeros(nx * nx, dtype=torch.float64, device=dev)
    dst = torch.zeros(nx * nx, dtype=torch.float64, device=dev)
    copy = lambda count: native.check(lib.vk_copy_stream(native.ptr(src), native.ptr(dst), count,
                                                         native.stream_handle()), 'vk_copy_stream')
    # vk_copy_stream moves 16 B per element (8 read, 8 written): the same bytes are bytes / 16 elements
    fill_bytes, gather_bytes = nx * nx * 8, n * 8 * (2 + 2)
    even = lambda count: count - count % 2
    plane = torch.zeros((nx, nx), dtype=torch.float64, device=dev)
    spec = field.specs()
    ms = alternating({
        'gradient_fill': lambda: native.check(lib.vk_gradient_fill(spec, 1, native.ptr(plane), nx * nx, nx, nx, nx,
                                                                   1000.0, 3000.0, native.stream_handle()), 'fill'),
        'copy_same_bytes_as_fill': lambda: copy(even(fill_bytes // 16)),
        'static_gather': lambda: field.gather(loc, n, conc, {'a': 0, 'b': 1}),
        'copy_same_bytes_as_gather': lambda: copy(even(gather_bytes // 16)),
    }, reps)
    res = {name: summary(t) for name, t in ms.items()}
    res['gradient_fill'].update(bytes=fill_bytes, fraction_of_copy_rate=(
        res['copy_same_bytes_as_fill']['median_ms'] / res['gradient_fill']['median_ms']))
    res['static_gather'].update(bytes=gather_bytes, fraction_of_copy_rate=(
        res['copy_same_bytes_as_gather']['median_ms'] / res['static_gather']['median_ms']))
    return res


def non_motile_step(dev, n, reps, k=10):
    cfg = configs.glc_lct_config()
    c = configs.chemotaxis_static('exponential', n_agents=n)
    rng = np.random.default_rng(configs.SEED)
    loc = np.stack([rng.uniform(0, 1000, n), rng.uniform(0, 3000, n)])
    static = Colony(cfg, n, device=dev, integrator='dopri5', environment=c['field'], specialize=True)
    static.set_agents(location=loc)
    held = Colony(cfg, n, device=dev, integrator='dopri5', environment='held', specialize=True)
    held.set_agents(conc=static.conc)
    for col in (static, held):
        col.step(1.0)
    replays = {'static_step': static.capture(1.0, k), 'held_step': held.capture(1.0, k)}
    res = {name: summary([t / k for t in ms]) for name, ms in alternating(replays, reps).items()}
    res['gather_ms_by_difference'] = res['static_step']['median_ms'] - res['held_step']['median_ms']
    return res


def experiment(dev, n=4096, seconds=60):
    out = {}
    for name in ('exponential', 'flat'):
        c = configs.chemotaxis_static('exponential', n_agents=n, substeps=SUBSTEPS)
        field = c['field']
        if name == 'flat':
            field = StaticField(field.molecules, field.bounds, {'type': 'exponential', 'molecules': {
                'glc__D_e': {'center': [0.5, 0.0], 'base': 1.0, 'scale': c['motility'].initial_ligand}}})
        col = Colony(configs.glc_lct_config(), n, device=dev, integrator='euler', environment=field,
                     motility=c['motility'])
        col.set_agents(location=c['location'])
        for _ in range(seconds):
            col.step(1.0)
        dy = (col.location[1, :n].cpu().numpy() - c['location'][1])
        out[name] = {'mean_dy_um': float(dy.mean()), 'sem_um': float(dy.std() / np.sqrt(n)),
                     'mean_ligand_mM': float(col.conc[col.table.species.index(('external', 'glc__D_e')), :n].mean())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1_000_000)
    ap.add_argument('--nx', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('static_field_timing: needs a GPU')
    dev = torch.device('cuda', 0)
    res = {'agents': args.agents, 'bins': [args.nx, args.nx], 'dt': 1.0, 'substeps': SUBSTEPS, 'reps': args.reps,
           'device': torch.cuda.get_device_name(0)}
    res['launches'] = launches(dev, args.agents, args.nx, args.reps)
    res['small_kernels'] = small_kernels(dev, args.agents, args.nx, args.reps)
    res['non_motile_step'] = non_motile_step(dev, args.agents, args.reps)
    res['experiment_60s_4096_agents'] = experiment(dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
