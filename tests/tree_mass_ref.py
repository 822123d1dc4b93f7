"""vk_cell_step_tree and the ``set`` divider of count rows, restated as Python loops.

The step is the one include/vk_kinetics.h states above vk_cell_step_tree: per agent, growth as
vk_cell_step has it (GrowthProtein) or none (the tree model), then the fold of the weighted
rows in ascending row order, one ``numpy.float64`` operation at a time, then the deriver tail
by CellModel's own formulas.  Nothing here imports the library."""

import numpy as np

from lens_amd import native
from lens_amd.cells import FG_PER_G, CellModel
from oracle.colony import philox_uniform

F = np.float64
TREE, PROTEIN = 'tree_mass', 'growth_protein'


def fold(cm, m, rows, weights, column):
    """m + the weighted rows of one agent's ``column`` of the table, k ascending."""
    m = F(m)
    for row, w in zip(rows, weights):
        count = np.int32(column[int(row)])
        m = m + (F(w) * (F(count) / F(cm.avogadro))) * F(FG_PER_G)
    return m


def derive(cm, m):
    """(volume, mmol_to_counts, length, surface area) of the mass ``m``."""
    return tuple(F(v) for v in cm.derive(F(m)))


def cell_step(cm, dt, step, n, cell, m2c, counts, rows, weights, u=None, lineage=None, initial_mass=None):
    """One step of agents [0, n) in place on ``cell`` [6, ld], ``m2c`` [ld]; ``counts``
    [n_rows, ld_counts] int32; ``u`` [n] (rng='stream') or ``lineage`` = (root, depth, path)
    (rng='philox').  Returns divide [n] int32."""
    p = cm.vk_params(dt, step)
    divide = np.zeros(n, dtype=np.int32)
    for a in range(n):
        if cm.model == PROTEIN:
            pr = F(cell[native.VK_CELL_PROTEIN, a])
            total = pr * F(p.factor)
            added = np.trunc(total - pr)
            extra = total - np.trunc(total)
            if cm.rng == 'philox':
                root, depth, path = lineage
                draw = philox_uniform(cm.seed, step, int(root[a]), int(depth[a]), int(path[a]))
            else:
                draw = u[a]
            if draw < extra:
                added = added + F(1.0)
            divide[a] = pr >= F(p.divide_protein)
            pn = pr + added
            cell[native.VK_CELL_PROTEIN, a] = pn
            m = F(0.0) + (F(cm.protein_mw) * (pn / F(cm.avogadro))) * F(FG_PER_G)
        else:
            assert cm.model == TREE
            divide[a] = F(cell[native.VK_CELL_VOLUME, a]) >= F(cm.division_volume)
            m = F(initial_mass[a])
        m = fold(cm, m, rows, weights, counts[:, a])
        volume, mc, length, area = derive(cm, m)
        cell[native.VK_CELL_MASS, a], cell[native.VK_CELL_VOLUME, a] = m, volume
        cell[native.VK_CELL_LENGTH, a], cell[native.VK_CELL_SURFACE_AREA, a] = length, area
        m2c[a] = mc
    return divide


def plan(divide):
    """(src, kind, n_keep): survivors in order, then the daughters 0, 1 of each mother in order."""
    keep = [a for a, d in enumerate(divide) if not d]
    mothers = [a for a, d in enumerate(divide) if d]
    src = keep + [a for a in mothers for _ in (0, 1)]
    kind = [-1] * len(keep) + [0, 1] * len(mothers)
    return np.array(src, dtype=np.int64), np.array(kind, dtype=np.int64), len(keep)


def divide_float(x, src, kind, split):
    """Rows of float64 over a plan: daughters halve (``split``) or copy."""
    out = np.array(x[..., src], dtype=np.float64)
    if split:
        out[..., kind >= 0] = out[..., kind >= 0] / F(2)
    return out


def set_rows(split_counts, x, src, set_rows_):
    """The ``set`` divider on top of the split restatement (ssa_ref.divide_counts): every slot
    of a ``set`` row holds its source's count, daughters included."""
    out = np.array(split_counts)
    for r in set_rows_:
        out[r] = np.asarray(x)[r, src]
    return out
