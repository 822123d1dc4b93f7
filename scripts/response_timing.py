"""Timing of the antibiotic-response launches at the C4 size (the
response section): 1M agents on 4096^2 bins of 1 um with the antibiotic kinetics
(AntibioticTransport's export, Euler), uniform over the plane, exchange 'sorted'.

    python scripts/response_timing.py [--agents N] [--nx NX] [--reps R] [--out profiles/response_timing.json]

Reports, in ms per step (graph replays, alternating): a colony without
``response=`` and one with, the latter with no agent dead, about half, and all
dead -- the cost of running the existing launches on frozen agents and
discarding their work.  Per launch (HIP events, median of R after a warm-up):
vk_response_begin, vk_expression_step, vk_response_end, the device occupancy
sort and vk_exchange_ordered_mixed, with the bytes each moves per agent and the
fraction of the 6.3 TB/s copy floor that makes.  Prints one JSON line and
writes it to ``--out``.  Needs a GPU: there is no fallback.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lens_amd.colony import Colony                                # noqa: E402
from lens_amd.lattice import Lattice, stencil_depth, stencil_kernel, stencil_mode   # noqa: E402
from lens_amd.rate_law_compiler import compile_rate_laws          # noqa: E402
from lens_amd.response import from_antibiotics                    # noqa: E402

COPY_FLOOR_TB_S = 6.3
SEED = 20260419


def build(dev, n, nx, response, dead_fraction=0.0):
    kin, resp = from_antibiotics({'diffusion': {'permeabilities': {'porin': 0.1}}})
    table = compile_rate_laws(kin['reactions'], kin['kinetic_parameters'])
    rng = np.random.default_rng(SEED)
    lat = Lattice(['antibiotic'], (nx, nx), (float(nx), float(nx)), 10.0, 5.0, device=dev,
                  initial={'antibiotic': 1.0 + rng.uniform(0.0, 1.0, (nx, nx))})
    col = Colony(kin, n, device=dev, integrator='euler', environment=lat, table=table,
                 response=resp if response else None)
    loc = rng.uniform(0.0, float(nx), (2, n))
    if response:
        L = col._resp_layout
        conc = col.conc[:, :n].cpu().numpy()
        conc[L.row(('membrane', 'porin'))] = rng.uniform(1e-17, 1e-16, n)
        conc[L.row(('pump_port', 'AcrAB-TolC'))] = rng.uniform(0.0, 0.5, n)
        col.set_agents(conc=conc, location=loc)
        k = int(round(dead_fraction * n))
        if k:
            # dead and frozen from the start: every other agent first, then the rest
            idx = torch.arange(n, device=dev)
            mask = (idx % 2 == 0) if k < n else torch.ones(n, dtype=torch.bool, device=dev)
            col.dead[:n] = mask.to(torch.int32)
            col.frozen[:n] = mask.to(torch.int32)
    else:
        col.set_agents(location=loc)
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


def bytes_per_agent(col, frozen_fraction):
    """Algorithmic bytes each launch moves per agent (antibiotics layout: 1 molecule, 1 porin,
    1 detector, 1 saved row, 1 flux row, 2 expression outputs, 1 exchange row)."""
    L, t = col._resp_layout, col.table
    nm, npn, nd, ns, nf, ne, nx = len(L.molecules), len(L.porins), len(L.det_row), L.n_dyn, t.n_reactions, \
        len(L.expr_rows), t.n_ext
    f = frozen_fraction
    begin = 4 + 8 * nd + 8 * npn + 8 * (2 * nm) + 4 + 16 * nm + f * (16 * ns + 16 * nf + 16)
    end = 4 + 4 + f * (16 * ns + 16 * nf + 16 + 8 * nx) + (1 - f) * 24 * ne + 24 * nm
    expression = 8 * 3 + 8 * ne                      # RNA twice and the pump read, two updates written
    exchange = 4 + 4 + 8 + 8 + 16                    # sorted_bin, order, int count, float count, the bin's value
    return {'vk_response_begin': begin, 'vk_expression_step': expression, 'vk_response_end': end,
            'vk_exchange_ordered_mixed': exchange}


def launches(col):
    lat = col.lattice
    return {
        'vk_response_begin': lambda: col._resp.begin(1.0, col.n, col.conc, None, col.frozen, col._resp_buf, col.flux,
                                                     col.status, col.nsteps, expression=False),
        'vk_expression_step': lambda: col._resp.expression.step(1.0, col.conc, col.n, update=col._resp_buf.expr_update,
                                                               accumulate=False),
        'vk_response_end': lambda: col._response_end(),
        'vk_occupancy_sort': lambda: col._occ_dev.sort(col.bin_lin, col.n, lat.rows_local * lat.ny, None),
        'vk_exchange_ordered_mixed': lambda: col._step_exchange(),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1_000_000)
    ap.add_argument('--nx', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--graph-steps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'response_timing.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('response_timing: needs a GPU')
    dev = torch.device('cuda', 0)
    stencil_mode('fma'), stencil_depth(10), stencil_kernel(70, 64)     # the bench's C4 settings
    n, nx, k = args.agents, args.nx, args.graph_steps
    res = {'agents': n, 'bins': [nx, nx], 'kinetics': 'antibiotic_transport (euler)', 'exchange': 'sorted',
           'reps': args.reps, 'device': torch.cuda.get_device_name(0), 'copy_floor_TB_per_s': COPY_FLOOR_TB_S}

    arms = {'plain': build(dev, n, nx, False), 'response_none_dead': build(dev, n, nx, True, 0.0),
            'response_half_dead': build(dev, n, nx, True, 0.5), 'response_all_dead': build(dev, n, nx, True, 1.0)}
    replays = {}
    for name, col in arms.items():
        col.step(1.0)                                                # loads every kernel
        replays[name] = col.capture(1.0, k)
        replays[name]()
    steps = {name: [] for name in arms}
    for _ in range(5):                                               # alternating
        for name, r in replays.items():
            steps[name] += [t / k for t in event_ms(r, 1, warmup=0)]
    res['step_ms'] = {name: summary(ms) for name, ms in steps.items()}
    res['dead_fraction_at_end'] = {name: float(col.dead[:n].double().mean()) for name, col in arms.items()
                                   if col.response is not None}

    res['launches'] = {}
    for arm, frac in (('response_none_dead', 0.0), ('response_half_dead', 0.5), ('response_all_dead', 1.0)):
        col = arms[arm]
        frac = float(col.frozen[:n].double().mean())
        per_agent = bytes_per_agent(col, frac)
        entry = {'frozen_fraction': frac}
        for name, fn in launches(col).items():
            s = summary(event_ms(fn, args.reps))
            if name in per_agent:
                s['bytes_per_agent'] = per_agent[name]
                s['achieved_TB_per_s'] = per_agent[name] * n / (s['median_ms'] * 1e-3) / 1e12
                s['fraction_of_copy_floor'] = s['achieved_TB_per_s'] / COPY_FLOOR_TB_S
            entry[name] = s
        res['launches'][arm] = entry
    for col in arms.values():
        col.check_status()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
