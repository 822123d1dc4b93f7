"""Timing of what motile division adds, and of what it must leave alone.

    python scripts/motile_division_timing.py [--parent-lib PATH] [--parent-tree DIR --bench-rounds 3]
        > profiles/motile_division_timing.json

1M agents on a 4096 x 4096 plane, dt = 1 s, one MI355X.  Every figure is HIP events around
the launches (or the graph replay), after a warm-up, as the median of 20 with min and max,
in ms:
  (a) step_flagella   a flagella colony's step without cells, replayed from a graph; with
                      ``--parent-lib`` (the library built from the parent commit) also with
                      that library, alternating with this tree's, each measurement in a
                      process of its own (two libraries with the same symbols do not share
                      a process);
  (b) expression      the expression launch plus vk_flagella_counts of one step, with the
                      bytes they must move (every expression row read and written, one
                      mmol_to_counts row read, one int row written) and that traffic's time
                      at 6.3 TB/s;
  (c) divide          one division event with 10 % mothers: vk_divide_flagella beside
                      vk_divide_gather (set) over the same three int rows and the key row;
  (d) bench           ``bench.py --gpus 1 --steps 20 --warmup 5`` of this tree and of a built
                      checkout of the parent commit (``--parent-tree``), alternating,
                      ``--bench-rounds`` times each.
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
    import torch  # noqa: F401  -- before any library: both bind to the HIP runtime torch ships
    from lens_amd import native
    if lib:
        # the parent's library lacks this tree's newest exports
        import ctypes
        have = ctypes.CDLL(lib)
        for name in [s for s in native._SIGS if not hasattr(have, s)]:
            native._SIGS.pop(name)
    native.load(lib or native.LIB_PATH)


def colony(expression):
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
    flagella = FlagellaModel(5, expression=configs.flagella_expression()) if expression else FlagellaModel(5)
    model = MotilityModel(initial_ligand=1e-2, substeps=10, seed=3, flagella=flagella)
    params, conc = configs.heterogeneous_colony(t, cfg, N)
    col = Colony(cfg, N, device=dev, integrator='dopri5', environment=lat, table=t, motility=model)
    col.set_agents(params=params, conc=conc, location=rng.uniform(0.0, BOUND, (2, N)))
    col.gather_external()
    return col


def worker_step(args):
    load(args.lib)
    col = colony(False)
    col.step(DT)
    replay = col.capture(DT, 1)
    print(json.dumps({'step_flagella': timed(replay)}), flush=True)


def worker_expression(args):
    load(None)
    col = colony(True)
    col.step(DT)

    def launches():
        col._flag_expression.step(DT, col.flag_expr, col.n, update=col._flag_expr_update, accumulate=True)
        col._flagella_counts()

    keys = col.flag_expr.shape[0]
    nbytes = N * (2 * 8 * keys + 8 + 4)
    out = timed(launches)
    out.update(bytes=nbytes, floor_ms=round(nbytes / COPY_FLOOR_BYTES_PER_S * 1e3, 4))
    out['share_of_floor'] = round(out['floor_ms'] / out['median_ms'], 4)
    print(json.dumps({'expression': out}), flush=True)


def worker_divide(args):
    import numpy as np
    import torch
    load(None)
    from lens_amd import native
    dev, st = torch.device('cuda', 0), native.stream_handle
    rng = np.random.default_rng(2)
    divide = torch.from_numpy((rng.random(N) < 0.1).astype(np.int32)).to(dev)
    src = torch.empty(2 * N, dtype=torch.int32, device=dev)
    kind = torch.empty(2 * N, dtype=torch.int32, device=dev)
    n_out_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(int(native._lib.vk_divide_scratch_bytes(N)), dtype=torch.uint8, device=dev)
    native.check(native._lib.vk_divide_plan(native.ptr(divide), N, native.ptr(src), native.ptr(kind),
                                            native.ptr(n_out_dev), native.ptr(scratch), st()), 'vk_divide_plan')
    n_out = int(n_out_dev.item())
    n_keep, ld = 2 * N - n_out, n_out
    have = rng.integers(0, 33, N)
    mask = rng.integers(0, 2 ** 32, N, dtype=np.uint64) & ((np.uint64(1) << have.astype(np.uint64)) - np.uint64(1))
    flag_int = torch.from_numpy(np.stack([rng.integers(0, 33, N).astype(np.int32), have.astype(np.int32),
                                          mask.astype(np.uint32).view(np.int32)])).to(dev).contiguous()
    key = torch.arange(N, dtype=torch.int64, device=dev)
    root = torch.arange(N, dtype=torch.int32, device=dev)
    depth = torch.zeros(N, dtype=torch.int32, device=dev)
    path = torch.zeros(N, dtype=torch.int64, device=dev)
    fi_dst = torch.empty((3, ld), dtype=torch.int32, device=dev)
    key_dst = torch.empty(ld, dtype=torch.int64, device=dev)

    def flagella(mode):
        native.check(native._lib.vk_divide_flagella(
            n_out, n_keep, N, native.ptr(src), native.ptr(kind), native.ptr(flag_int), N, native.ptr(key),
            native.ptr(root), native.ptr(depth), native.ptr(path), native.ptr(fi_dst), ld, native.ptr(key_dst), mode, 3,
            7, N, st()), 'vk_divide_flagella')

    def gathers():
        native.check(native._lib.vk_divide_gather(n_out, native.ptr(src), native.ptr(kind), native.ptr(flag_int), N,
                                                  native.ptr(fi_dst), ld, 3, 4, native.VK_DIVIDE_SET, st()), 'gather')
        native.check(native._lib.vk_divide_gather(n_out, native.ptr(src), native.ptr(kind), native.ptr(key), N,
                                                  native.ptr(key_dst), ld, 1, 8, native.VK_DIVIDE_SET, st()), 'gather')

    out = {'agents_out': n_out, 'mothers': N - n_keep,
           'vk_divide_flagella_merged': timed(lambda: flagella(native.VK_FLAGELLA_MERGED)),
           'vk_divide_flagella_split_dict': timed(lambda: flagella(native.VK_FLAGELLA_SPLIT_DICT)),
           'vk_divide_gather_set_int_rows_and_keys': timed(gathers)}
    print(json.dumps({'divide': out}), flush=True)


def child(*argv):
    res = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(argv), check=True, stdout=subprocess.PIPE,
                         timeout=600)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def bench(tree):
    res = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'],
                         check=True, stdout=subprocess.PIPE, timeout=900, cwd=tree)
    line = json.loads(res.stdout.decode().strip().splitlines()[-1])
    return {'ms_per_step': round(line['ms_per_step'], 5), 'value': round(line['value'], 1)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent-lib', default=None)
    p.add_argument('--rounds', type=int, default=3, help='alternations of tree and parent (a)')
    p.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit (d)')
    p.add_argument('--bench-rounds', type=int, default=0, help='alternations of tree and parent (d); 0: skip')
    p.add_argument('--worker', default=None, choices=['step', 'expression', 'divide'])
    p.add_argument('--lib', default=None)
    args = p.parse_args()
    if args.worker:
        return {'step': worker_step, 'expression': worker_expression, 'divide': worker_divide}[args.worker](args)
    out = {'agents': N, 'bins': [NX, NX], 'dt': DT, 'reps': REPS, 'warmup': WARMUP,
           'tree': {'step_flagella': [], 'bench': []}, 'parent': {'step_flagella': [], 'bench': []}}
    for r in range(args.rounds if args.parent_lib else 1):
        if args.parent_lib:
            out['parent']['step_flagella'].append(child('--worker', 'step', '--lib', args.parent_lib)['step_flagella'])
        out['tree']['step_flagella'].append(child('--worker', 'step')['step_flagella'])
    out['tree'].update(child('--worker', 'expression'))
    out['tree'].update(child('--worker', 'divide'))
    for r in range(args.bench_rounds):
        if args.parent_tree:
            out['parent']['bench'].append(bench(os.path.abspath(args.parent_tree)))
        out['tree']['bench'].append(bench(REPO))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
