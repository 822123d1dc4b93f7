"""NumPy restatement of one relaxation iteration of the contact kernel
(vk_contact_step, lens_amd/csrc/vk_contact.hip) for the tests: the same
operations in the same order, elementwise over all N x N pairs.

Neighbours are NOT found through the kernel's grid tables: every agent visits
every other agent, in ascending (grid cell, key) order.  Pairs that do not
overlap contribute an exact 0.0, which leaves a floating-point sum unchanged, so
the result is the kernel's whenever no capsule is longer than a grid cell's edge
(the kernel then misses no contact among its 3 x 3 cells).  The cell index is
needed only for that order.  Jitter draws are oracle.colony.philox_uniform
(seed, iteration, key, 1, j), j = 0..3.
"""

import math

import numpy as np

from oracle.colony import philox_uniform

TWO_PI = 6.283185307179586


def grid(bounds, max_length):
    """(gx, gy, edge_x, edge_y) of the neighbour grid."""
    gx = max(1, int(math.floor(bounds[0] / max_length)))
    gy = max(1, int(math.floor(bounds[1] / max_length)))
    return gx, gy, bounds[0] / gx, bounds[1] / gy


def cells(x, y, bounds, max_length):
    gx, gy, ex, ey = grid(bounds, max_length)
    cx = np.minimum(gx - 1, np.floor(x / ex).astype(np.int64))
    cy = np.minimum(gy - 1, np.floor(y / ey).astype(np.int64))
    return cx * gy + cy


def bin_axis(loc, n, bound):
    return np.floor(loc * n / bound).astype(np.int64) % n


def bins(x, y, n_bins, bounds):
    """(bin_lin, ix) as vk_bin_sites gives them."""
    ix = bin_axis(x, n_bins[0], bounds[0])
    return (ix * n_bins[1] + bin_axis(y, n_bins[1], bounds[1])).astype(np.int32), ix.astype(np.int32)


def pairs(x, y, th, L, w):
    """Closest spine points of every ordered pair (i, j) = [row, column]:
    dict of N x N arrays (the diagonal is meaningless)."""
    ux, uy = np.cos(th), np.sin(th)
    h = np.maximum(L - w, 0.0) / 2.0
    hi, hj = h[:, None], h[None, :]
    uxi, uyi, uxj, uyj = ux[:, None], uy[:, None], ux[None, :], uy[None, :]
    rx, ry = x[:, None] - x[None, :], y[:, None] - y[None, :]
    b = uxi * uxj + uyi * uyj
    c = uxi * rx + uyi * ry
    f = uxj * rx + uyj * ry
    den = 1.0 - b * b
    clamp = lambda v: np.minimum(np.maximum(v, -hi), hi)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(den > 1e-12, clamp((b * f - c) / den), 0.0)
    t = b * s + f
    lo, up = t < -hj, t > hj
    s = np.where(lo, clamp(-b * hj - c), np.where(up, clamp(b * hj - c), s))
    t = np.where(lo, -hj, np.where(up, hj, t))
    vx = (x[:, None] + s * uxi) - (x[None, :] + t * uxj)
    vy = (y[:, None] + s * uyi) - (y[None, :] + t * uyj)
    d = np.sqrt(vx * vx + vy * vy)
    r = w / 2.0
    return dict(s=s, t=t, vx=vx, vy=vy, d=d, delta=(r + r) - d, den=den, rx=rx, ry=ry, ux=ux, uy=uy, h=h, L=L)


def pushes(x, y, th, L, keys, w, stiffness):
    """(px, py, dtheta) [i, j]: what neighbour j adds to agent i; zero where the
    pair does not overlap and on the diagonal.  Also the pair dict."""
    q = pairs(x, y, th, L, w)
    n = x.shape[0]
    d, delta = q['d'], q['delta']
    rho = np.sqrt(q['rx'] * q['rx'] + q['ry'] * q['ry'])
    first = np.where(keys[:, None] < keys[None, :], 1.0, -1.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        nx = np.where(d > 1e-9, q['vx'] / d, np.where(rho > 1e-9, q['rx'] / rho, first))
        ny = np.where(d > 1e-9, q['vy'] / d, np.where(rho > 1e-9, q['ry'] / rho, 0.0))
    contact = (delta > 0.0) & ~np.eye(n, dtype=bool)
    mag = 0.5 * stiffness * delta
    px = np.where(contact, mag * nx, 0.0)
    py = np.where(contact, mag * ny, 0.0)
    s, uxi, uyi = q['s'], q['ux'][:, None], q['uy'][:, None]
    dth = np.where(contact, ((s * uxi) * py - (s * uyi) * px) * 12.0 / (L[:, None] * L[:, None]), 0.0)
    q['contact'] = contact
    return px, py, dth, q


def crossing(q):
    """Touching pairs whose closest points are interior to both spines."""
    return (q['contact'] & (q['den'] > 1e-12) & (np.abs(q['s']) < q['h'][:, None]) &
            (np.abs(q['t']) < q['h'][None, :]))


def margins(q):
    """How far the reference's own branch decisions are from a tie: the smallest
    |delta|, |den - 1e-12| (pairs of two true capsules: with h = 0 on either side
    the branch does not matter) and |d - 1e-9| (overlapping pairs), off the diagonal.
    'den_near' is the den margin over the pairs within reach of each other (centres
    closer than (L_i + L_j) / 2: no other pair can touch, whichever branch it takes),
    'den_cross' the smallest den itself over touching pairs whose closest points are
    both interior (the spines cross: only there does s keep the 1 / den of the
    solve), 'd_small' the smallest d above 1e-9 over touching pairs (the normal
    v / d amplifies rounding by 1 / d)."""
    n = q['d'].shape[0]
    off = ~np.eye(n, dtype=bool)
    out = {'delta': 1.0, 'den': 1.0, 'den_near': 1.0, 'd': 1.0, 'den_cross': 1.0, 'd_small': 1.0}
    if n < 2:
        return out
    out['delta'] = float(np.abs(q['delta'][off]).min())
    both = off & (q['h'][:, None] > 0.0) & (q['h'][None, :] > 0.0)
    if both.any():
        out['den'] = float(np.abs(q['den'][both] - 1e-12).min())
    near = both & (np.sqrt(q['rx'] * q['rx'] + q['ry'] * q['ry']) < (q['L'][:, None] + q['L'][None, :]) / 2.0)
    if near.any():
        out['den_near'] = float(np.abs(q['den'][near] - 1e-12).min())
    if q['contact'].any():
        out['d'] = float(np.abs(q['d'][q['contact']] - 1e-9).min())
    cross = crossing(q)
    if cross.any():
        out['den_cross'] = float(q['den'][cross].min())
    apart = q['contact'] & (q['d'] > 1e-9)
    if apart.any():
        out['d_small'] = float(q['d'][apart].min())
    return out


def draws(seed, s, keys):
    return np.array([[philox_uniform(seed, s, int(k), 1, j) for k in keys] for j in range(4)])


def iterate(x, y, th, L, keys, bounds, s_global, *, stiffness=0.5, max_length=4.0, width=1.0, max_push=None,
            max_turn=0.5, jitter=0.0, jitter_angle=0.0, seed=0, clamp=True, info=None):
    """One iteration: new (x, y, theta).  ``max_push`` None: width / 2; math.inf:
    no cap.  ``clamp`` False leaves the walls out (the self-checks).  ``info``
    (optional dict) receives the margins, the push matrices and the visit order."""
    n = x.shape[0]
    max_push = width / 2.0 if max_push is None else max_push
    cell = cells(x, y, bounds, max_length)
    order = np.lexsort((keys, cell))                 # ascending (cell, key)
    xs, ys, ts, Ls, ks = x[order], y[order], th[order], L[order], keys[order]
    px, py, dth, q = pushes(xs, ys, ts, Ls, ks, width, stiffness)
    dcx, dcy, dt_ = np.zeros(n), np.zeros(n), np.zeros(n)
    for j in range(n):                               # the kernel's summation order
        dcx = dcx + px[:, j]
        dcy = dcy + py[:, j]
        dt_ = dt_ + dth[:, j]
    m = np.sqrt(dcx * dcx + dcy * dcy)
    capped = m > max_push
    scale = np.where(capped, max_push / np.where(capped, m, 1.0), 1.0)
    dcx = np.where(capped, dcx * scale, dcx)
    dcy = np.where(capped, dcy * scale, dcy)
    dt_ = np.minimum(np.maximum(dt_, -max_turn), max_turn)
    nxs, nys, nts = xs + dcx, ys + dcy, ts + dt_
    if jitter != 0.0 or jitter_angle != 0.0:
        u = draws(seed, s_global, ks)
        r0, r1 = np.sqrt(-2.0 * np.log(1.0 - u[0])), np.sqrt(-2.0 * np.log(1.0 - u[2]))
        nxs = nxs + jitter * (r0 * np.cos(TWO_PI * u[1]))
        nys = nys + jitter * (r0 * np.sin(TWO_PI * u[1]))
        nts = nts + jitter_angle * (r1 * np.cos(TWO_PI * u[3]))
    if clamp:
        nxs = np.minimum(np.maximum(nxs, 0.0), np.nextafter(bounds[0], 0.0))
        nys = np.minimum(np.maximum(nys, 0.0), np.nextafter(bounds[1], 0.0))
    if info is not None:
        info.update(margins=margins(q), px=px, py=py, order=order, contact=q['contact'], capped=capped,
                    cell=cell)
    out = [np.empty(n), np.empty(n), np.empty(n)]
    for dst, src in zip(out, (nxs, nys, nts)):
        dst[order] = src
    return out


def overlap_sum(x, y, th, L, w):
    """Summed overlap delta over the unordered pairs that touch."""
    q = pairs(x, y, th, L, w)
    n = x.shape[0]
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    delta = q['delta'][upper]
    return float(delta[delta > 0.0].sum())
