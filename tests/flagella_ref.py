"""NumPy restatement of the flagella kernel (vk_flagella_step) for the tests:
the reference's FlagellaActivity.next_update (flagella_activity.py:135-261) in
its operation order, vectorised over agents, between the receptor of
tests/motility_ref.py and this engine's run-and-tumble move (which is NOT the
reference's pymunk multibody).  Random draws are oracle.colony.philox_uniform
(seed, inner update, agent key, 0, path) with the kernel's paths: 1, 2 the tumble
heading, 3, 4 the CheY-P noise, 16 + i flagellum i's switch, 64 + r the r-th
structural draw (a removal index, or a new flagellum's state).

Scalars go through ``math`` (the reference's own functions: the known answers of
tests/test_flagella_host.py are to the last bit), arrays through NumPy.
"""

import math

import numpy as np

from oracle.colony import philox_uniform

import motility_ref as mref

FLAG_ROWS = ('CheY', 'CheY_P', 'cw_bias', 'motile_state', 'PMF')
FLAGI_ROWS = ('target', 'have', 'mask')
F = {name: i for i, name in enumerate(FLAG_ROWS)}
FI = {name: i for i, name in enumerate(FLAGI_ROWS)}
R = mref.R
MAX_FLAGELLA = 32


def _exp(x):
    return math.exp(x) if np.ndim(x) == 0 else np.exp(x)


def _pow(x, y):
    return float(x) ** y if np.ndim(x) == 0 else np.power(x, y)


def uniforms(seed, s, keys, path):
    """philox_uniform for every key at once: the scalar function's integer
    arithmetic carries over to uint64 arrays unchanged (every product of two
    32-bit words fits 64 bits)."""
    keys = np.asarray(keys, dtype=np.int64).astype(np.uint64)
    return np.asarray(philox_uniform(int(seed), int(s), keys, 0, int(path)), dtype=np.float64)


def normal(seed, s, keys, path):
    u1, u2 = uniforms(seed, s, keys, path), uniforms(seed, s, keys, path + 1)
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(6.283185307179586 * u2)


def switch_rates(f, CheY_P):
    """(delta_g, CW_to_CCW, CCW_to_CW) of update_flagellum (:229-233)."""
    delta_g = f['g_0'] / 4 - f['g_1'] / 2 * (CheY_P / (CheY_P + f['K_D']))
    return delta_g, f['omega'] * _exp(delta_g), f['omega'] * _exp(-delta_g)


def cw_bias(f, CheY_P):
    return _pow(CheY_P, f['H']) / (_pow(f['K_d'], f['H']) + _pow(CheY_P, f['H']))


def thrust(f, scaling, PMF, n_flagella):
    """run() / tumble() (:253-261), multiplied left to right."""
    return f[scaling] * PMF * f['flagellum_thrust'] * n_flagella


def noise_amplitude(f, h):
    """sigma * (2 * timestep / tau) ** 0.5 with both square roots correctly rounded."""
    return math.sqrt(f['sigma2_Y']) * math.sqrt(2.0 * h / f['tau'])


def remove_bit(mask, j):
    """Delete bit j of the uint64 mask(s) and close the gap."""
    j = np.asarray(j, dtype=np.uint64)
    one = np.uint64(1)
    return (mask & ((one << j) - one)) | ((mask >> (j + one)) << j)


def _margin(margins, name, values):
    if margins is not None and np.size(values):
        margins[name] = min(margins.get(name, 1.0), float(np.min(values)))


def step(model, motil, flag, flag_int, loc, field, bounds, dt, substeps, counter, keys=None, margins=None):
    """``substeps`` inner updates in place on motil [9, n], flag [5, n] (float64),
    flag_int [3, n] (int32) and loc [2, n]; field is the ligand plane [nx, ny].
    Returns the linear bins.  ``margins`` (optional dict) collects the smallest
    |u - prob| over all switch draws ('switch'), the smallest distance of a
    structural draw to its threshold ('structural': to j / remaining for a removal,
    to 1/2 for a new flagellum) and the smallest distance of a moved coordinate to
    a bin edge or wall in bin widths ('edge') -- the conditions under which the
    device must agree exactly on the discrete results."""
    rp, f = model.receptor, model.flagella.parameters
    n = motil.shape[1]
    nx, ny = field.shape
    bx, by = bounds
    keys = np.arange(n) if keys is None else np.asarray(keys)
    h = dt / substeps
    amp = noise_amplitude(f, h)
    one = np.uint64(1)
    target = np.clip(flag_int[FI['target']].astype(np.int64), 0, MAX_FLAGELLA)
    have = np.clip(flag_int[FI['have']].astype(np.int64), 0, MAX_FLAGELLA)
    mask = flag_int[FI['mask']].astype(np.int32).view(np.uint32).astype(np.uint64)
    mask &= (one << have.astype(np.uint64)) - one
    PMF = flag[F['PMF']]
    x, y = loc[0].copy(), loc[1].copy()
    ix, iy = mref.bin_axis(x, nx, bx), mref.bin_axis(y, ny, by)
    for s in range(substeps):
        st = counter + s
        L = field[ix, iy]
        nm, P_on = mref.receptor(rp, motil[R['n_methyl']], motil[R['chemoreceptor_activity']], L, h)
        # 2. CheY-P
        dYP = -(1 / f['tau']) * (flag[F['CheY_P']] - f['YP_ss']) * h + amp * normal(model.seed, st, keys, 3)
        CheY_P = np.maximum(flag[F['CheY_P']] + dYP, 0.0)
        CheY = np.maximum(flag[F['CheY']] - dYP, 0.0)
        # 3. the existing flagella
        _, cw_to_ccw, ccw_to_cw = switch_rates(f, CheY_P)
        p_cw, p_ccw = cw_to_ccw * h, ccw_to_cw * h
        for i in range(int(have.max()) if n else 0):
            alive = i < have
            u = uniforms(model.seed, st, keys, 16 + i)
            prob = np.where((mask >> np.uint64(i)) & one != 0, p_cw, p_ccw)
            _margin(margins, 'switch', np.abs(u - prob)[alive])
            mask ^= (alive & (u <= prob)).astype(np.uint64) << np.uint64(i)
        # 4. motile state and thrust
        change = target - have
        tumble = mask != 0
        run = ~tumble & ((have > 0) | (change > 0))
        motile = np.where(tumble, 1.0, np.where(run, -1.0, 0.0))
        push = np.where(tumble, thrust(f, 'tumble_scaling', PMF, target.astype(np.float64)),
                        np.where(run, thrust(f, 'run_scaling', PMF, target.astype(np.float64)), 0.0))
        # 1. the count change takes effect
        for r in range(int(np.abs(change).max()) if n else 0):
            u = uniforms(model.seed, st, keys, 64 + r)
            gone = -change > r
            remaining = np.where(gone, have - r, 1)
            t = u * remaining
            j = np.minimum(np.floor(t), remaining - 1)
            _margin(margins, 'structural', (np.abs(t - np.round(t)) / remaining)[gone])
            mask = np.where(gone, remove_bit(mask, np.where(gone, j, 0)), mask)
            new = change > r
            _margin(margins, 'structural', np.abs(u - 0.5)[new])
            mask |= (new & (u < 0.5)).astype(np.uint64) << np.where(new, have + r, 0).astype(np.uint64)
        have = target.copy()
        # kinematics
        z = normal(model.seed, st, keys, 1)
        d_angle = np.where(tumble, model.tumble_sigma * h * z, 0.0)
        angle = np.where(tumble, motil[R['angle']] + d_angle, motil[R['angle']])
        speed = model.run_speed * push / 250.0
        x = x + speed * h * np.cos(angle)
        y = y + speed * h * np.sin(angle)
        lo, hi = x < 0.0, x >= bx
        x = np.where(lo, -x, np.where(hi, 2.0 * bx - x, x))
        angle = np.where(lo | hi, math.pi - angle, angle)
        lo, hi = y < 0.0, y >= by
        y = np.where(lo, -y, np.where(hi, 2.0 * by - y, y))
        angle = np.where(lo | hi, -angle, angle)
        x = np.minimum(np.maximum(x, 0.0), np.nextafter(bx, 0.0))
        y = np.minimum(np.maximum(y, 0.0), np.nextafter(by, 0.0))
        for c, nb, b in ((x, nx, bx), (y, ny, by)):
            t = c * nb / b                       # in bin widths; walls are the edges 0 and nb
            _margin(margins, 'edge', np.abs(t - np.round(t)))
        ix, iy = mref.bin_axis(x, nx, bx), mref.bin_axis(y, ny, by)
        motil[R['n_methyl']], motil[R['chemoreceptor_activity']] = nm, P_on
        motil[R['motor_state']] = tumble.astype(np.float64)
        motil[R['angle']] = angle
        motil[R['thrust']] = push
        motil[R['torque']] = np.where(tumble, d_angle / h, 0.0)
        flag[F['CheY']], flag[F['CheY_P']] = CheY, CheY_P
        flag[F['cw_bias']] = cw_bias(f, CheY_P)
        flag[F['motile_state']] = motile
    flag_int[FI['have']] = have
    flag_int[FI['mask']] = mask.astype(np.uint32).view(np.int32)
    loc[0], loc[1] = x, y
    return (ix * ny + iy).astype(np.int32)
