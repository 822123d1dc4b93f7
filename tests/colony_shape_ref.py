"""NumPy restatement of the colony metrics (vk_colony_metrics,
lens_amd/csrc/vk_colonies.hip) for the tests, over all N x N pairs.

The distance d of every ordered pair is ``mechanics_ref.pairs``' arithmetic (the
contact kernel's closest-point solve); the partition comes from
``scipy.sparse.csgraph.connected_components``, not from a union-find; the sums are
``math.fsum`` (correctly rounded), not the kernel's order.  Neighbours are not found
through a grid: the grid cell is computed only for the (cell, key) order that numbers
the colonies.
"""

import math

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import mechanics_ref

ROWS = ('mass', 'cell_area', 'cx', 'cy', 'sxx', 'syy', 'sxy', 'angle', 'major', 'minor')
SUM_TOL = 1e-12           # (n - 1) 2^-53 for a sum of n <= 1000 terms in any order, against fsum


def grid(bounds, max_length, gap):
    """(gx, gy, edge_x, edge_y): cell edges >= max_length + gap."""
    gx = max(1, int(math.floor(bounds[0] / (max_length + gap))))
    gy = max(1, int(math.floor(bounds[1] / (max_length + gap))))
    return gx, gy, bounds[0] / gx, bounds[1] / gy


def cell_axis(x, edge, g):
    """min(g - 1, floor(x / edge)); anything else (outside, NaN) in an end cell."""
    with np.errstate(invalid='ignore'):
        v = np.floor(x / edge)
        return np.where(v >= 0.0, np.minimum(v, g - 1.0), 0.0).astype(np.int64)


def cells(x, y, bounds, max_length, gap):
    gx, gy, ex, ey = grid(bounds, max_length, gap)
    return cell_axis(x, ex, gx) * gy + cell_axis(y, ey, gy)


def links(x, y, th, L, w, gap):
    """(link [N, N] bool, margin [N, N]): margin = (2 r + gap) - d of the ordered pair;
    a pair is linked when either ordered evaluation is >= 0.  Agents with a non-finite
    location link to nobody."""
    n = x.shape[0]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        q = mechanics_ref.pairs(x, y, th, L, w)
        r = w / 2.0
        margin = ((r + r) + gap) - q['d']
        finite = np.isfinite(x) & np.isfinite(y)
        ok = finite[:, None] & finite[None, :] & ~np.eye(n, dtype=bool)
        link = ok & (margin >= 0.0)
    return link | link.T, np.where(ok, margin, np.inf)


def tie_margin(margin):
    """The smallest |margin| over all ordered pairs of finite agents (inf for none)."""
    return float(np.abs(margin).min()) if margin.size else math.inf


def analyse(x, y, th, L, keys, bounds, *, width=1.0, gap=0.5, min_cells=3, max_length=4.0, mass=None,
            mass_const=1.0):
    """dict: colony [N] (-1: none), n_colonies, cells, key, the ROWS per colony (fsum),
    'abs_moments' (sum of |terms| of sxx, syy, sxy per colony), 'residual' (|sum dx| + |sum dy|
    about the rounded centroid), 'anisotropy' ((lambda_1 - lambda_2) / lambda_1 of the moment
    matrix), 'radius' (the farthest capsule end from the centroid) and 'tie' (the smallest
    |margin|)."""
    n = x.shape[0]
    out = {'colony': np.full(n, -1, dtype=np.int64), 'n_colonies': 0, 'cells': [], 'key': [], 'tie': math.inf,
           'abs_moments': [], 'anisotropy': [], 'radius': [], 'residual': []}
    for name in ROWS:
        out[name] = []
    if n == 0:
        return out
    link, margin = links(x, y, th, L, width, gap)
    out['tie'] = tie_margin(margin)
    _, comp = connected_components(csr_matrix(link), directed=False)
    finite = np.isfinite(x) & np.isfinite(y)
    cell = cells(x, y, bounds, max_length, gap)
    order = np.lexsort((keys, cell))                 # ascending (cell, key)
    position = np.empty(n, dtype=np.int64)
    position[order] = np.arange(n)
    groups = {}
    for a in range(n):
        groups.setdefault(comp[a], []).append(a)
    found = []
    for members in groups.values():
        if len(members) >= min_cells and all(finite[a] for a in members):
            members.sort(key=lambda a: position[a])
            found.append(members)
    found.sort(key=lambda m: position[m[0]])         # by first member in (cell, key) order
    mass = np.full(n, mass_const) if mass is None else mass
    r = width / 2.0
    h = np.maximum(L - width, 0.0) / 2.0
    for c, m in enumerate(found):
        m = np.array(m)
        out['colony'][m] = c
        out['cells'].append(len(m))
        out['key'].append(int(keys[m].min()))
        xs, ys = x[m], y[m]
        out['mass'].append(math.fsum(mass[m]))
        out['cell_area'].append(math.fsum(width * np.maximum(L[m] - width, 0.0) + math.pi * width * width / 4.0))
        cx, cy = math.fsum(xs) / len(m), math.fsum(ys) / len(m)
        dx, dy = xs - cx, ys - cy
        sxx, syy, sxy = math.fsum(dx * dx), math.fsum(dy * dy), math.fsum(dx * dy)
        phi = 0.5 * math.atan2(2.0 * sxy, sxx - syy)
        ext = []
        for ex, ey in ((math.cos(phi), math.sin(phi)), (-math.sin(phi), math.cos(phi))):
            p = dx * ex + dy * ey
            q = h[m] * np.abs(np.cos(th[m]) * ex + np.sin(th[m]) * ey)
            ext.append(float((p + q + r).max() - (p - q - r).min()))
        for name, v in zip(ROWS, (out['mass'][-1], out['cell_area'][-1], cx, cy, sxx, syy, sxy, phi,
                                  max(ext), min(ext))):
            if name not in ('mass', 'cell_area'):
                out[name].append(v)
        out['abs_moments'].append((math.fsum(dx * dx), math.fsum(dy * dy), math.fsum(np.abs(dx * dy))))
        out['residual'].append(abs(math.fsum(dx)) + abs(math.fsum(dy)))
        lam = math.hypot(2.0 * sxy, sxx - syy)       # lambda_1 - lambda_2
        lam1 = 0.5 * ((sxx + syy) + lam)
        out['anisotropy'].append(lam / lam1 if lam1 > 0.0 else 0.0)
        out['radius'].append(float(np.sqrt(dx * dx + dy * dy).max() + h[m].max() + r))
    out['n_colonies'] = len(found)
    for name in ('cells', 'key') + ROWS + ('anisotropy', 'radius', 'residual'):
        out[name] = np.array(out[name])
    out['abs_moments'] = np.array(out['abs_moments']).reshape(-1, 3)
    return out


def bounds(want):
    """The bounds a device result must meet against ``analyse``'s values, per colony, all from
    the restatement alone:
      'sum'      SUM_TOL, relative, for mass, cell_area, cx, cy (sums of positive terms);
      'moments'  [C, 3]: SUM_TOL times the sum of |terms| of sxx, syy, sxy;
      'angle'    dphi <= |dS| / (lambda_1 - lambda_2), |dS| the sum of the three moment bounds;
      'extent'   radius * dphi, for major and minor;
      'conditioned'  where angle and extents may be compared: anisotropy >= 0.05, radius <= 64 um
                 and |phi| < pi / 2 - 1e-3 (phi jumps by pi across the cut at +-pi / 2)."""
    tol_s = SUM_TOL * want['abs_moments']
    lam = np.hypot(2.0 * want['sxy'], want['sxx'] - want['syy'])
    with np.errstate(divide='ignore', invalid='ignore'):
        dphi = tol_s.sum(axis=1) / lam
    ok = (want['anisotropy'] >= 0.05) & (want['radius'] <= 64.0) & (np.abs(want['angle']) < math.pi / 2 - 1e-3)
    return {'sum': SUM_TOL, 'moments': tol_s, 'angle': dphi, 'extent': want['radius'] * dphi, 'conditioned': ok}
