"""NumPy restatement of the motility kernel (vk_motility_step) for the tests:
the reference's receptor (chemoreceptor_cluster.py:166-209) and motor
(coarse_motor.py:134-164) arithmetic, vectorised over agents in the same
operation order, and this engine's run-and-tumble kinematics (which are NOT the
reference's pymunk multibody).  Random draws are oracle.colony.philox_uniform
(seed, inner update, agent key, 0, j).
"""

import math

import numpy as np

from oracle.colony import philox_uniform

ROWS = ('n_methyl', 'chemoreceptor_activity', 'CheY_P', 'ccw_motor_bias', 'ccw_to_cw', 'motor_state', 'angle',
        'thrust', 'torque')
R = {name: i for i, name in enumerate(ROWS)}


def receptor(p, n_methyl, P_on, L, h):
    """(n_methyl, P_on) after one update; arrays.  The quirk: an out-of-range
    n_methyl is clamped and not advanced in that update."""
    CheR, CheB = p['CheR'] * 1e3, p['CheB'] * 1e3     # mM -> uM (pint's factor, unpinned)
    low, high = n_methyl < 0, n_methyl > 8
    d = p['adapt_rate'] * (p['k_meth'] * CheR * (1.0 - P_on) - p['k_demeth'] * CheB * P_on) * h
    nm = np.where(low, 0.0, np.where(high, 8.0, n_methyl + d))
    eps = np.select(
        [nm < 0, nm < 2, nm < 4, nm < 6, nm < 7, nm < 8],
        [np.full_like(nm, 1.0), 1.0 - 0.5 * nm, -0.3 * (nm - 2.0), -0.6 - 0.25 * (nm - 4.0),
         -1.1 - 0.9 * (nm - 6.0), -2.0 - (nm - 7.0)], -3.0)
    tar = float(p['n_Tar']) * (eps + np.log((1.0 + L / p['K_Tar_off']) / (1.0 + L / p['K_Tar_on'])))
    tsr = float(p['n_Tsr']) * (eps + np.log((1.0 + L / p['K_Tsr_off']) / (1.0 + L / p['K_Tsr_on'])))
    with np.errstate(over='ignore'):
        return nm, 1.0 / (1.0 + np.exp(tar + tsr))


def motor_rates(m, P_on):
    """(CheY_P, ccw_motor_bias, ccw_to_cw) of an activity (array)."""
    CheY_P = float(m['adapt_precision']) * m['k_y'] * m['k_s'] * P_on / (m['k_y'] * m['k_s'] * P_on + m['k_z'] + m['gamma_Y'])
    bias = m['mb_0'] / (CheY_P * (1.0 - m['mb_0']) + m['mb_0'])
    ccw_to_cw = m['cw_to_ccw'] * (1.0 / bias - 1.0)
    return CheY_P, bias, np.maximum(ccw_to_cw, m['cw_to_ccw_leak'])


def switch_probability(r, h):
    with np.errstate(divide='ignore', invalid='ignore'):
        p = 1.0 - np.exp(-(-np.log(1.0 - r)) * h)
    return np.where(r >= 1.0, 1.0, p)


def bin_axis(loc, n, bound):
    return np.floor(loc * n / bound).astype(np.int64) % n


def draws(seed, s, keys):
    return np.array([[philox_uniform(seed, s, int(k), 0, j) for k in keys] for j in range(3)])


def step(model, motil, loc, field, bounds, dt, substeps, counter, keys=None, margins=None):
    """``substeps`` inner updates in place on motil [9, n] and loc [2, n]; field
    is the ligand plane [nx, ny].  Returns the linear bins.  ``margins``
    (optional dict) collects the smallest |u0 - p| and the smallest distance of
    a moved coordinate to a bin edge or wall in units of the bin width -- the
    conditions under which the device must agree exactly on the discrete results."""
    rp, mp = model.receptor, model.motor
    n = motil.shape[1]
    nx, ny = field.shape
    bx, by = bounds
    keys = np.arange(n) if keys is None else keys
    h = dt / substeps
    x, y = loc[0], loc[1]
    ix, iy = bin_axis(x, nx, bx), bin_axis(y, ny, by)
    for s in range(substeps):
        L = field[ix, iy]
        nm, P_on = receptor(rp, motil[R['n_methyl']], motil[R['chemoreceptor_activity']], L, h)
        CheY_P, bias, c2c = motor_rates(mp, P_on)
        tumbling = motil[R['motor_state']] != 0
        p = switch_probability(np.where(tumbling, mp['cw_to_ccw'], c2c), h)
        u = draws(model.seed, counter + s, keys)
        tumbling = np.where(u[0] <= p, ~tumbling, tumbling)
        z = np.sqrt(-2.0 * np.log(1.0 - u[1])) * np.cos(6.283185307179586 * u[2])
        d_angle = np.where(tumbling, model.tumble_sigma * h * z, 0.0)
        angle = np.where(tumbling, motil[R['angle']] + d_angle, motil[R['angle']])
        speed = np.where(tumbling, model.run_speed * 100.0 / 250.0, model.run_speed)
        x = x + speed * h * np.cos(angle)
        y = y + speed * h * np.sin(angle)
        if margins is not None:
            margins['switch'] = min(margins.get('switch', 1.0), float(np.abs(u[0] - p).min()))
        # walls
        lo, hi = x < 0.0, x >= bx
        x = np.where(lo, -x, np.where(hi, 2.0 * bx - x, x))
        angle = np.where(lo | hi, math.pi - angle, angle)
        lo, hi = y < 0.0, y >= by
        y = np.where(lo, -y, np.where(hi, 2.0 * by - y, y))
        angle = np.where(lo | hi, -angle, angle)
        x = np.minimum(np.maximum(x, 0.0), np.nextafter(bx, 0.0))
        y = np.minimum(np.maximum(y, 0.0), np.nextafter(by, 0.0))
        if margins is not None:
            for c, nb, b in ((x, nx, bx), (y, ny, by)):
                t = c * nb / b                       # in bin widths; walls are the edges 0 and nb
                edge = float(np.abs(t - np.round(t)).min())
                margins['edge'] = min(margins.get('edge', 1.0), edge)
        ix, iy = bin_axis(x, nx, bx), bin_axis(y, ny, by)
        motil[R['n_methyl']], motil[R['chemoreceptor_activity']] = nm, P_on
        motil[R['CheY_P']], motil[R['ccw_motor_bias']], motil[R['ccw_to_cw']] = CheY_P, bias, c2c
        motil[R['motor_state']] = tumbling.astype(np.float64)
        motil[R['angle']] = angle
        motil[R['thrust']] = np.where(tumbling, 100.0, 250.0)
        motil[R['torque']] = np.where(tumbling, d_angle / h, 0.0)
    loc[0], loc[1] = x, y
    return (ix * ny + iy).astype(np.int32)
