"""Timing of the mother machine's launches at the C4 size (the mother
machine section): 1M capsules of 2 x 1 um in channels on 4096^2 bins of 1 um --
channel space 4 um (1024 lines), channel height 0.7 of the plane, the agents
uniform over the channels' interiors up to the plane's top (so three in ten are
above the channels), axis angles within 0.3 rad of the channel axis.

    python scripts/mother_machine_timing.py [--agents N] [--nx NX] [--reps R] [--out PATH]

HIP-event times (median, min and max of R repetitions after a warm-up), the two
sides of each comparison alternating:
  * vk_contact_step_channels against vk_contact_step, 4 iterations, from the same
    state (restored before every launch);
  * vk_population_plan (divide and remove flags at 0.05 each) plus the gathers of
    a colony's per-agent arrays, against vk_divide_plan (the same divide flags)
    plus the same gathers.
Writes profiles/mother_machine_timing.json and prints it as one JSON line.
Needs a GPU: there is no fallback.
"""

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from lens_amd import configs, native                              # noqa: E402
from lens_amd.lattice import Lattice                              # noqa: E402
from lens_amd.mechanics import ContactBuffers, ContactModel, contact_step   # noqa: E402

SPACE, SPACER, WIDTH, LENGTH = 4.0, 0.1, 1.0, 2.0


def model(nx, channels):
    ch = {'channel_height': 0.7 * nx, 'channel_space': SPACE, 'spacer_thickness': SPACER} if channels else None
    return ContactModel(iterations=4, jitter=0.01, jitter_angle=0.02, seed=configs.SEED, channels=ch)


def state(n, nx, seed=configs.SEED):
    rng = np.random.default_rng(seed)
    edge = WIDTH / 2 + SPACER
    c = rng.integers(0, int(nx // SPACE), n)
    x = c * SPACE + edge + rng.uniform(0.0, SPACE - 2 * edge, n)
    y = rng.uniform(0.0, float(nx), n)
    angle = math.pi / 2 + rng.uniform(-0.3, 0.3, n)
    return np.stack([x, y]), angle


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms))}


def alternate(sides, reps, warmup=2):
    """{name: [ms]}: ``reps`` timed runs of every side, the sides alternating.  A side is
    (prepare, run): prepare is not timed."""
    out = {name: [] for name in sides}
    for r in range(warmup + reps):
        for name, (prepare, run) in sides.items():
            prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                out[name].append(e0.elapsed_time(e1))
    return out


def contact_sides(dev, n, nx):
    lat = Lattice(['glc__D_e'], (nx, nx), (float(nx), float(nx)), 10.0, 5.0, device=dev)
    loc0, angle0 = state(n, nx)
    loc0, angle0 = torch.from_numpy(loc0).to(dev), torch.from_numpy(angle0).to(dev)
    loc, angle = loc0.clone(), angle0.clone()
    bins, ix = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    outflow = torch.zeros(n, dtype=torch.int32, device=dev)
    m = {name: model(nx, name == 'channels') for name in ('channels', 'plain')}
    gx, gy = m['plain'].grid(lat.bounds)
    buf = ContactBuffers(n, gx * gy, dev)

    def restore():
        loc.copy_(loc0)
        angle.copy_(angle0)
        buf.counter.zero_()

    def launch(name):
        return lambda: contact_step(m[name], lat, loc, angle, n, buf, bin_lin=bins, bin_ix=ix,
                                    outflow=outflow if name == 'channels' else None)

    return {name: (restore, launch(name)) for name in m}, lambda: (int(outflow.sum()), int(buf.flags[0]))


def plan_sides(dev, n):
    lib = native.load()
    rng = np.random.default_rng(configs.SEED + 1)
    divide = torch.from_numpy((rng.random(n) < 0.05).astype(np.int32)).to(dev)
    remove = torch.from_numpy((rng.random(n) < 0.05).astype(np.int32)).to(dev)
    ld = 2 * n
    # a colony's per-agent arrays (glc_ac at C4: 11 parameter rows, 7 species, 2 fluxes, 2 counts, ...)
    arrays = [torch.zeros((rows, n), dtype=dt, device=dev) for rows, dt in (
        (11, torch.float64), (7, torch.float64), (1, torch.float64), (2, torch.float64), (2, torch.int64),
        (1, torch.int32), (1, torch.int32), (1, torch.float64), (2, torch.float64))]
    dst = [torch.zeros((a.shape[0], ld), dtype=a.dtype, device=dev) for a in arrays]
    src = torch.zeros(ld, dtype=torch.int32, device=dev)
    kind = torch.zeros(ld, dtype=torch.int32, device=dev)
    n_out = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(int(lib.vk_population_scratch_bytes(n)) + int(lib.vk_divide_scratch_bytes(n)),
                          dtype=torch.uint8, device=dev)
    st = native.stream_handle()

    def gathers(count):
        for a, d in zip(arrays, dst):
            native.check(lib.vk_divide_gather(count, native.ptr(src), native.ptr(kind), native.ptr(a), n,
                                              native.ptr(d), ld, a.shape[0], a.element_size(),
                                              native.VK_DIVIDE_SET, st), 'vk_divide_gather')

    counts = {}

    def population():
        native.check(lib.vk_population_plan(native.ptr(divide), native.ptr(remove), n, native.ptr(src),
                                            native.ptr(kind), native.ptr(n_out), native.ptr(scratch), st),
                     'vk_population_plan')
        counts['population'] = int(n_out.item())          # the host read a colony pays too
        gathers(counts['population'])

    def division():
        native.check(lib.vk_divide_plan(native.ptr(divide), n, native.ptr(src), native.ptr(kind), native.ptr(n_out),
                                        native.ptr(scratch), st), 'vk_divide_plan')
        counts['division'] = int(n_out.item())
        gathers(counts['division'])

    nothing = lambda: None
    return {'population_plan_and_gathers': (nothing, population), 'divide_plan_and_gathers': (nothing, division)}, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1_000_000)
    ap.add_argument('--nx', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mother_machine_timing.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mother_machine_timing: needs a GPU')
    dev = torch.device('cuda', 0)
    n, nx = args.agents, args.nx
    res = {'agents': n, 'bins': [nx, nx], 'capsule_um': [LENGTH, WIDTH], 'channel_space_um': SPACE,
           'channel_height_um': 0.7 * nx, 'lines': int(nx // SPACE), 'iterations': 4, 'reps': args.reps,
           'device': torch.cuda.get_device_name(0)}
    sides, flags = contact_sides(dev, n, nx)
    ms = alternate(sides, args.reps)
    res['contact_step_channels'] = summary(ms['channels'])
    res['contact_step_plain'] = summary(ms['plain'])
    sides['channels'][0]()
    sides['channels'][1]()
    res['agents_flagged'], res['flag_word'] = flags()
    sides, counts = plan_sides(dev, n)
    ms = alternate(sides, args.reps)
    for name in sides:
        res[name] = summary(ms[name])
    res['n_out'] = counts
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
