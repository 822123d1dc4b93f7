"""Timing of the cell step with TreeMass over the count table, and of what it must leave alone.

    python scripts/tree_mass_timing.py [--parent-lib PATH] [--rounds 3] > profiles/tree_mass_timing.json

1M agents, one MI355X, ld = ld_counts = the agent count (as a colony without spare capacity has
it).  Every figure is HIP events around the launch, after a warm-up, as the median of 20 with
min and max, in ms.  The state is restored before every timed launch, outside the timing.
  (a) tree            vk_cell_step_tree in the VK_GROWTH_TREE model over the 77-row table of the
                      whole flagella chromosome (configs.flagella_gene_expression(operons=None))
                      with the weights of configs.gene_expression_cell (69 weighted rows), counts
                      of 0..999 per row and agent;
      cell_step       vk_cell_step (VK_GROWTH_MASS: the same rows read and written, no table) on
                      the same cell rows;
      copy            vk_copy_stream over the bytes the tree launch must move, counted here from
                      the shapes: in, 4 B per weighted row, the step-start volume and
                      initial_mass; out, the mass, volume, length and surface-area rows,
                      mmol_to_counts and divide;
  (b) plain           vk_cell_step alone (VK_GROWTH_PROTEIN with Philox draws, and VK_GROWTH_MASS);
                      with ``--parent-lib`` (the library built from the parent commit) also with
                      that library, alternating with this tree's, each measurement in a process of
                      its own.  "Unchanged" holds if each median lies inside the other's min-max.
Prints one JSON line.
"""

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'scripts'))

from ssa_timing import N, load, timed  # noqa: E402

GOLDEN = os.path.join(REPO, 'tests', 'golden')


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def child(*argv):
    import subprocess
    res = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(argv), check=True, stdout=subprocess.PIPE,
                         timeout=600)
    print('done:', ' '.join(argv), file=sys.stderr, flush=True)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def _cell_state(cm, dev):
    """Cell rows of N agents around the division threshold, m2c, divide and the lineage."""
    import torch
    from lens_amd import native
    g = torch.Generator(device=dev).manual_seed(5)
    spread = 1.0 + torch.rand(N, generator=g, device=dev, dtype=torch.float64)          # 1 .. 2 times the start
    rows, m2c = cm.initial_rows(1)
    cell = torch.from_numpy(rows).to(dev).repeat(1, N).contiguous()
    for r in (native.VK_CELL_MASS, native.VK_CELL_VOLUME, native.VK_CELL_PROTEIN):
        cell[r] *= spread
    i32 = lambda: torch.zeros(N, dtype=torch.int32, device=dev)
    lineage = (torch.arange(N, dtype=torch.int32, device=dev), i32(), torch.zeros(N, dtype=torch.int64, device=dev))
    return cell, torch.full((N,), float(m2c[0]), dtype=torch.float64, device=dev), i32(), lineage


def _plain(cm, dev):
    """vk_cell_step of ``cm`` on state restored before every launch."""
    import ctypes
    from lens_amd import native
    cell0, m2c, divide, (root, depth, path) = _cell_state(cm, dev)
    cell = cell0.clone()
    p = cm.vk_params(1.0, 3)
    launch = lambda: native.check(native._lib.vk_cell_step(
        ctypes.byref(p), N, N, native.ptr(cell), native.ptr(m2c), None, native.ptr(root), native.ptr(depth),
        native.ptr(path), native.ptr(divide), native.stream_handle()), 'vk_cell_step')
    return timed(launch, before=lambda: cell.copy_(cell0))


def worker_plain(args):
    import torch
    load(args.lib)
    from lens_amd.cells import CellModel
    dev = torch.device('cuda', 0)
    print(json.dumps({'growth_protein': _plain(CellModel(rng='philox', seed=7), dev),
                      'growth': _plain(CellModel(model='growth', growth_rate=0.0006), dev)}), flush=True)


def worker_tree(args):
    import torch
    load(None)
    from lens_amd import configs, native
    from lens_amd.cells import CellModel, cell_step_tree
    dev = torch.device('cuda', 0)
    tl = golden('flagella_translation.json')
    cfg = configs.flagella_gene_expression(golden('flagella_transcription.json'), tl,
                                           golden('flagella_complexation.json'), golden('flagella_degradation.json'))
    sm = cfg['stochastic']
    cm = configs.gene_expression_cell(tl, cfg['transcription'], golden('flagella_complex_weights.json')['molecular_weight'])
    tree = cm.bind(sm).upload(dev)
    W = len(tree)
    g = torch.Generator(device=dev).manual_seed(6)
    counts = torch.randint(0, 1000, (sm.n_rows, N), generator=g, device=dev, dtype=torch.int32)
    cell0, m2c, divide, (root, depth, path) = _cell_state(CellModel(model='growth'), dev)
    cell = cell0.clone()
    initial_mass = cell0[native.VK_CELL_MASS].clone()
    p = cm.vk_params(1.0, 3)
    launch = lambda: native.check(cell_step_tree(p, N, N, cell, m2c, None, root, depth, path, divide, counts, tree,
                                                 initial_mass), 'vk_cell_step_tree')
    r = timed(launch, before=lambda: cell.copy_(cell0))
    torch.cuda.synchronize()
    r['dividing'] = round(int(divide.sum().item()) / N, 3)
    plain = _plain(CellModel(model='growth', growth_rate=0.0006), dev)
    bytes_in, bytes_out = N * (4 * W + 8 + 8), N * (4 * 8 + 8 + 4)
    moved = bytes_in + bytes_out
    src = torch.empty(moved // 16, dtype=torch.float64, device=dev)          # moved bytes: half in, half out
    dst = torch.empty_like(src)
    c = timed(lambda: native.check(native._lib.vk_copy_stream(native.ptr(src), native.ptr(dst), src.numel(),
                                                              native.stream_handle()), 'vk_copy_stream'))
    c.update(bytes=moved, bytes_in=bytes_in, bytes_out=bytes_out)
    r['over_copy'] = round(r['median_ms'] / c['median_ms'], 2)
    r['bytes_per_s'] = round(moved / (r['median_ms'] * 1e-3), 1)
    print(json.dumps({'rows': sm.n_rows, 'weighted': W, 'tree': r, 'cell_step': plain, 'copy': c}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent-lib', default=None)
    p.add_argument('--rounds', type=int, default=3, help='alternations of tree and parent (b)')
    p.add_argument('--worker', default=None, choices=['plain', 'tree'])
    p.add_argument('--lib', default=None)
    args = p.parse_args()
    if args.worker:
        return {'plain': worker_plain, 'tree': worker_tree}[args.worker](args)
    out = {'agents': N, 'tree': {'plain': []}, 'parent': {'plain': []}}
    out['tree'].update(child('--worker', 'tree'))
    for r in range(args.rounds if args.parent_lib else 1):
        if args.parent_lib:
            out['parent']['plain'].append(child('--worker', 'plain', '--lib', args.parent_lib))
        out['tree']['plain'].append(child('--worker', 'plain'))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
