"""Motile agents: the reference's chemotaxis processes, batched.

:class:`MotilityModel` holds what the reference's ``ReceptorCluster``
(vivarium/processes/chemoreceptor_cluster.py) and ``MotorActivity``
(vivarium/processes/coarse_motor.py) hold -- their default parameters and
initial states, the receptor run to its steady state at the initial ligand
concentration -- and the two constants of this engine's kinematics.  A
``Colony(..., motility=model)`` then moves its agents every step on the
device (vk_motility_step) and re-bins them there (vk_occupancy_sort,
vk_exchange_ordered): no host read, no re-layout, so the step can be captured.

Receptor and motor follow the reference's arithmetic.  The move itself does
NOT: the reference hands thrust and torque to pymunk (multibody), which this
engine does not have.  Agents run at ``run_speed`` along their heading, drift
at 100/250 of it while tumbling with a Gaussian heading change of
``tumble_sigma`` rad/s, and reflect off the lattice bounds.

``MotilityModel(..., flagella=FlagellaModel(n_flagella))`` swaps the coarse
motor for the reference's ``FlagellaActivity``
(vivarium/processes/flagella_activity.py): up to 32 flagella per agent that
switch on their own, CheY-P as an Ornstein-Uhlenbeck process, a tumble when
any flagellum turns CW, thrust from the flagella count and the proton motive
force (vk_flagella_step).  The speed then is ``run_speed * thrust / 250``.

``MotilityModel(..., division='merged' | 'split_dict')`` lets such a colony grow and
divide (``Colony(..., cells=CellModel(...), motility=model)``), and
``FlagellaModel(0, expression=...)`` derives the flagella count from an expressed
protein: together the reference's ChemotaxisODEExpressionFlagella agent
(vk_flagella_counts, vk_divide_flagella).
"""

from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np

from lens_amd import native

STEADY_STATE_DELTA = 1e-6

# ReceptorCluster.defaults + INITIAL_INTERNAL_STATE (chemoreceptor_cluster.py:22-28, :98-114)
RECEPTOR_DEFAULTS = {
    'n_Tar': 6, 'n_Tsr': 12,
    'K_Tar_off': 0.02, 'K_Tar_on': 0.5, 'K_Tsr_off': 100.0, 'K_Tsr_on': 10e6,
    'k_meth': 0.0625, 'k_demeth': 0.0714, 'adapt_rate': 1.2,
    'CheR': 0.00016, 'CheB': 0.00028,               # mM
    'n_methyl': 2.0, 'chemoreceptor_activity': 1. / 3.,
}
# MotorActivity.defaults (coarse_motor.py:51-86)
MOTOR_DEFAULTS = {
    'k_y': 100.0, 'k_z': 30.0, 'gamma_Y': 0.1, 'k_s': 0.45, 'adapt_precision': 3,
    'mb_0': 0.65, 'cw_to_ccw': 0.83, 'cw_to_ccw_leak': 0.25,
    'CheY_P': 0.5, 'ccw_motor_bias': 0.5, 'ccw_to_cw': 0.5, 'motor_state': 1, 'thrust': 0, 'torque': 0,
}

ROW_NAMES = ('n_methyl', 'chemoreceptor_activity', 'CheY_P', 'ccw_motor_bias', 'ccw_to_cw', 'motor_state',
             'angle', 'thrust', 'torque')          # vk_motil_row order


# FlagellaActivity.defaults (flagella_activity.py:48-86), verbatim; next_update reads YP_ss,
# sigma2_Y, tau, K_d, H, omega, g_0, g_1, K_D, flagellum_thrust and the two scalings
FLAGELLA_INITIAL_PMF = 170
FLAGELLA_DEFAULTS = {
    'n_flagella': 5,
    'initial_state': {'CheY': 2.59, 'CheY_P': 2.59, 'cw_bias': 0.5, 'motile_state': 0, 'PMF': FLAGELLA_INITIAL_PMF},
    'ccw_to_cw': 0.26, 'cw_to_ccw': 1.7, 'CB': 0.13, 'lambda': 0.68,
    'YP_ss': 2.59, 'sigma2_Y': 1.0, 'tau': 0.2,
    'K_d': 3.1, 'H': 10.3,
    'omega': 1.3, 'g_0': 40, 'g_1': 40, 'K_D': 3.06,
    'flagellum_thrust': 25, 'tumble_jitter': 120.0,
    'tumble_scaling': 1 / FLAGELLA_INITIAL_PMF, 'run_scaling': 1 / FLAGELLA_INITIAL_PMF,
    'time_step': 0.01,
}
FLAG_ROW_NAMES = ('CheY', 'CheY_P', 'cw_bias', 'motile_state', 'PMF')      # vk_flag_row order
FLAGI_ROW_NAMES = ('target', 'have', 'mask')                                # vk_flagi_row order
MAX_FLAGELLA = 32
DIVISION_MODES = {None: None, 'merged': native.VK_FLAGELLA_MERGED, 'split_dict': native.VK_FLAGELLA_SPLIT_DICT}


def check_flagella_counts(counts):
    """``counts`` (an int or an array of ints) as an int64 array, every value in 0..32."""
    c = np.asarray(counts)
    if c.dtype.kind not in 'iu' and not (c.dtype.kind == 'f' and np.all(c == np.floor(c))):
        raise ValueError('flagella counts must be whole numbers')
    c = c.astype(np.int64)
    if c.ndim > 1 or (c.size and (c.min() < 0 or c.max() > MAX_FLAGELLA)):
        raise ValueError('flagella counts must lie in 0..%d (one value, or one per agent)' % MAX_FLAGELLA)
    return c


class FlagellaModel:
    """The reference's ``FlagellaActivity`` (vivarium/processes/flagella_activity.py):
    its default parameters and initial state.  ``n_flagella`` is one count for
    every agent or one per agent, 0..32.  ``MotilityModel(flagella=FlagellaModel())``
    runs it in the place of the coarse motor (vk_flagella_step).

    ``expression`` (an ``ODE_expression`` configuration dict, e.g.
    ``configs.flagella_expression()``) makes the count a derived quantity, as in the
    reference's ChemotaxisODEExpressionFlagella (chemotaxis_flagella.py:94-173): the
    colony keeps the configuration's transcripts and proteins per agent
    (``flag_expr``), advances them every step (vk_expression_step) and sets the count
    to ``int(concentration of count_of * mmol_to_counts)`` (vk_flagella_counts).
    ``n_flagella`` then is only the number of flagella the agents start with (the
    reference's agent: 0).  The configuration's states all live under ``'internal'``;
    regulators on other ports and a transcription leak (host draws that cannot be
    replayed) are refused.

    ``complexes`` (a species id, e.g. ``'flagella'``) takes the count from the colony's
    stochastic network instead (``Colony(stochastic=StochasticModel(...))``), as in the
    reference's ChemotaxisExpressionFlagella (chemotaxis_flagella.py:176-291), where
    ``Complexation`` assembles the ``'flagella'`` complex: after every stochastic step, and
    once at t = 0, the count is the agent's int count of that species, 0..32
    (vk_ssa_flagella_target).  It does not combine with ``expression``."""

    def __init__(self, n_flagella=5, expression=None, count_of='flagella', complexes=None, **parameters):
        self.expression, self.count_of, self.expression_table = None, count_of, None
        if complexes is not None and expression is not None:
            raise ValueError('flagella: the count follows either an expressed protein (expression=) or a complex '
                             'of the stochastic network (complexes=), not both')
        if complexes is not None and not isinstance(complexes, str):
            raise ValueError('flagella: complexes must be the id of a species of the colony\'s stochastic network')
        self.complexes = complexes
        if expression is not None:
            self._compile_expression(expression, count_of)
        unknown = set(parameters) - set(FLAGELLA_DEFAULTS)
        if unknown:
            raise ValueError('unknown flagella parameters: %s' % sorted(unknown))
        initial = parameters.pop('initial_state', None) or {}
        unknown = set(initial) - set(FLAGELLA_DEFAULTS['initial_state'])
        if unknown:
            raise ValueError('unknown flagella initial states: %s' % sorted(unknown))
        self.n_flagella = check_flagella_counts(n_flagella)
        self.parameters = dict(FLAGELLA_DEFAULTS, **parameters)
        self.parameters['n_flagella'] = n_flagella
        self.parameters['initial_state'] = dict(FLAGELLA_DEFAULTS['initial_state'], **initial)
        if not self.parameters['tau'] > 0 or self.parameters['sigma2_Y'] < 0:
            raise ValueError('flagella: tau > 0 and sigma2_Y >= 0')

    def _compile_expression(self, config, count_of):
        from lens_amd.expression import ExpressionTable, RuleSyntaxError
        if not isinstance(config, dict):
            raise ValueError('flagella expression must be an ODE_expression configuration dict')
        leak = config.get('transcription_leak') or {}
        if leak.get('rate', 0.0) != 0 or leak.get('magnitude', 0.0) != 0:
            raise ValueError('flagella expression: a transcription_leak draws on the host and cannot be replayed '
                             '(rate and magnitude must be 0)')
        for port, name in config.get('regulators', []):
            if port != 'internal':
                raise ValueError('flagella expression: regulator (%r, %r) is not on the internal port' % (port, name))
        initial = (config.get('initial_state') or {}).get('internal', {})
        names = list(dict.fromkeys(list(config.get('transcription_rates', {})) +
                                   list(config.get('translation_rates', {})) + list(initial) +
                                   [name for _, name in config.get('regulators', [])]))
        if count_of not in names:
            raise ValueError('flagella expression: count_of=%r is not one of its states %s' % (count_of, names))
        try:
            self.expression_table = ExpressionTable(config, [('internal', s) for s in names])
        except (KeyError, RuleSyntaxError) as e:
            raise ValueError('flagella expression: %s' % (e.args[0] if e.args else e))
        self.expression = config
        self.expression_names = names
        self.count_row = names.index(count_of)
        self.expression_initial = np.array([float(initial.get(s, 0.0)) for s in names], dtype=np.float64)

    def counts(self, n: int) -> np.ndarray:
        c = self.n_flagella
        if c.ndim == 0:
            return np.full(n, int(c), dtype=np.int64)
        if c.shape[0] < n:
            raise ValueError('n_flagella must give every agent a count (%d < %d)' % (c.shape[0], n))
        return c[:n]

    def initial_rows(self, n: int, ld: int, seed: int = 0):
        """(flag [VK_FLAG_ROWS, ld] float64, flag_int [VK_FLAGI_ROWS, ld] int32): the
        reference's initial_state; have = target = n_flagella, and each flagellum CW
        with probability 1/2 from a numpy generator seeded with ``seed``."""
        flag = np.zeros((native.VK_FLAG_ROWS, ld))
        for row, name in enumerate(FLAG_ROW_NAMES):
            flag[row, :n] = self.parameters['initial_state'][name]
        flag_int = np.zeros((native.VK_FLAGI_ROWS, ld), dtype=np.int32)
        have = self.counts(n)
        cw = np.random.default_rng(seed).random((n, MAX_FLAGELLA)) < 0.5
        cw &= np.arange(MAX_FLAGELLA)[None, :] < have[:, None]
        mask = (cw.astype(np.uint64) << np.arange(MAX_FLAGELLA, dtype=np.uint64)[None, :]).sum(axis=1)
        flag_int[native.VK_FLAGI_TARGET, :n] = have
        flag_int[native.VK_FLAGI_HAVE, :n] = have
        flag_int[native.VK_FLAGI_MASK, :n] = mask.astype(np.uint32).view(np.int32)
        return flag, flag_int

    def vk_params(self) -> native.VkFlagellaParams:
        f = native.VkFlagellaParams()
        for name, _ in native.VkFlagellaParams._fields_:
            setattr(f, name, float(self.parameters[name]))
        return f


def receptor_update(p, n_methyl, P_on, ligand, timestep):
    """ReceptorCluster.next_update (chemoreceptor_cluster.py:166-209) on plain
    floats; CheR / CheB mM -> uM as x * 1e3 (the reference converts through
    pint, which this restatement is not pinned against)."""
    CheR, CheB = p['CheR'] * 1e3, p['CheB'] * 1e3
    if n_methyl < 0:
        n_methyl = 0
    elif n_methyl > 8:
        n_methyl = 8
    else:
        n_methyl += p['adapt_rate'] * (p['k_meth'] * CheR * (1.0 - P_on) - p['k_demeth'] * CheB * P_on) * timestep
    if n_methyl < 0:
        eps = 1.0
    elif n_methyl < 2:
        eps = 1.0 - 0.5 * n_methyl
    elif n_methyl < 4:
        eps = -0.3 * (n_methyl - 2.0)
    elif n_methyl < 6:
        eps = -0.6 - 0.25 * (n_methyl - 4.0)
    elif n_methyl < 7:
        eps = -1.1 - 0.9 * (n_methyl - 6.0)
    elif n_methyl < 8:
        eps = -2.0 - (n_methyl - 7.0)
    else:
        eps = -3.0
    tar = p['n_Tar'] * (eps + math.log((1 + ligand / p['K_Tar_off']) / (1 + ligand / p['K_Tar_on'])))
    tsr = p['n_Tsr'] * (eps + math.log((1 + ligand / p['K_Tsr_off']) / (1 + ligand / p['K_Tsr_on'])))
    return n_methyl, 1.0 / (1.0 + math.exp(tar + tsr))


class MotilityModel:
    def __init__(self, ligand_id: str = 'MeAsp', initial_ligand: float = 5.0, receptor: Optional[dict] = None,
                 motor: Optional[dict] = None, run_speed: float = 14.0, tumble_sigma: float = math.radians(120.0),
                 substeps: int = 1, seed: int = 0, angles=None, flagella: Optional[FlagellaModel] = None,
                 division: Optional[str] = None):
        if flagella is not None and not isinstance(flagella, FlagellaModel):
            raise ValueError('flagella must be a FlagellaModel')
        if division not in DIVISION_MODES:
            raise ValueError('division must be None, \'merged\' or \'split_dict\' (got %r)' % (division,))
        for given, known, what in ((receptor, RECEPTOR_DEFAULTS, 'receptor'), (motor, MOTOR_DEFAULTS, 'motor')):
            unknown = set(given or {}) - set(known)
            if unknown:
                raise ValueError('unknown %s parameters: %s' % (what, sorted(unknown)))
        if int(substeps) < 1:
            raise ValueError('substeps >= 1')
        self.ligand_id = ligand_id
        self.initial_ligand = float(initial_ligand)
        self.receptor = dict(RECEPTOR_DEFAULTS, **(receptor or {}))
        self.motor = dict(MOTOR_DEFAULTS, **(motor or {}))
        self.run_speed = float(run_speed)        # um/s: the speed the reference's timelines assume
        self.tumble_sigma = float(tumble_sigma)  # rad/s
        self.substeps = int(substeps)
        self.seed = int(seed)
        self.angles = angles                     # initial headings (rad) per agent; None: seeded uniform
        self.flagella = flagella                 # None: the coarse motor (vk_motility_step)
        # how the motile state divides in a colony with cells=: None refuses such a colony;
        # 'merged' is what the reference's Store does (both daughters keep every flagellum),
        # 'split_dict' the divider FlagellaActivity declares.  No effect without cells
        self.division = division
        # run_to_steady_state(self, initial_state, 1.0) (chemoreceptor_cluster.py:36-46, :126)
        n_methyl, P_on = self.receptor['n_methyl'], self.receptor['chemoreceptor_activity']
        delta, self.steady_iterations = 1, 0
        while delta > STEADY_STATE_DELTA:
            nm, po = receptor_update(self.receptor, n_methyl, P_on, self.initial_ligand, 1.0)
            delta = ((P_on - po) ** 2 + (n_methyl - nm) ** 2) ** 0.5
            n_methyl, P_on = nm, po
            self.steady_iterations += 1
        self.n_methyl, self.chemoreceptor_activity = n_methyl, P_on

    def initial_rows(self, n: int, ld: int, angles=None) -> np.ndarray:
        """motil[VK_MOTIL_ROWS][ld]: the receptor at its steady state, the motor
        rows from MotorActivity's initial_state, headings from ``angles`` or
        uniform in [0, 2 pi) from a numpy generator seeded with the model's seed."""
        rows = np.zeros((native.VK_MOTIL_ROWS, ld))
        m = self.motor
        for name, value in (('n_methyl', self.n_methyl), ('chemoreceptor_activity', self.chemoreceptor_activity),
                            ('CheY_P', m['CheY_P']), ('ccw_motor_bias', m['ccw_motor_bias']),
                            ('ccw_to_cw', m['ccw_to_cw']), ('motor_state', m['motor_state']),
                            ('thrust', m['thrust']), ('torque', m['torque'])):
            rows[ROW_NAMES.index(name), :n] = value
        if angles is None:
            angles = self.angles
        if angles is None:
            angles = np.random.default_rng(self.seed).uniform(0.0, 2.0 * math.pi, n)
        angles = np.asarray(angles, dtype=np.float64)
        if angles.shape[0] < n:
            raise ValueError('angles must give every agent a heading (%d < %d)' % (angles.shape[0], n))
        rows[native.VK_MOTIL_ANGLE, :n] = angles[:n]
        return rows

    def vk_params(self) -> native.VkMotilityParams:
        p = native.VkMotilityParams()
        for name in ('n_Tar', 'n_Tsr', 'K_Tar_off', 'K_Tar_on', 'K_Tsr_off', 'K_Tsr_on', 'k_meth', 'k_demeth',
                     'adapt_rate', 'CheR', 'CheB'):
            setattr(p, name, float(self.receptor[name]))
        for name in ('k_y', 'k_s', 'k_z', 'gamma_Y', 'adapt_precision', 'mb_0', 'cw_to_ccw', 'cw_to_ccw_leak'):
            setattr(p, name, float(self.motor[name]))
        p.run_speed, p.tumble_sigma, p.seed = self.run_speed, self.tumble_sigma, self.seed
        return p


def motility_step(model: MotilityModel, lattice, location, motil, n: int, dt: float, counter, key=None,
                  bin_lin=None, bin_ix=None, substeps: Optional[int] = None):
    """One vk_motility_step launch on the current stream: ``model.substeps``
    inner updates of ``dt / substeps`` for agents [0, n) of ``location`` [2, ld]
    and ``motil`` [VK_MOTIL_ROWS, ld]; ``counter`` (one device int64) supplies
    the inner-update index and is advanced.  ``bin_lin`` / ``bin_ix`` (int32
    [ld]) receive the bins.  The lattice must hold whole, unbanded planes; a
    :class:`lens_amd.static_field.StaticField` in its place senses the analytic
    gradient at each agent's own position (vk_motility_step_static)."""
    import torch
    from lens_amd.lattice import whole_plane
    from lens_amd.static_field import StaticField
    static = isinstance(lattice, StaticField)
    if not static and not whole_plane(lattice):
        raise ValueError('motility_step: a whole, unbanded plane')
    ld = location.shape[1]
    if motil.shape != (native.VK_MOTIL_ROWS, ld) or not (motil.is_contiguous() and location.is_contiguous()):
        raise ValueError('motility_step: motil must be [VK_MOTIL_ROWS, ld] beside location [2, ld], contiguous')
    if bin_lin is None:
        bin_lin = torch.zeros(ld, dtype=torch.int32, device=location.device)
    p = model.vk_params()
    if static:
        launch, ligand = native._lib.vk_motility_step_static, ctypes.byref(lattice.spec(model.ligand_id))
    else:
        launch = native._lib.vk_motility_step
        ligand = native.ptr(lattice.fields[lattice.molecules.index(model.ligand_id)])
    native.check(launch(
        ctypes.byref(p), n, ld, float(dt), int(model.substeps if substeps is None else substeps), native.ptr(motil),
        native.ptr(location), native.ptr(key), ligand, lattice.n_bins[0], lattice.n_bins[1],
        lattice.bounds[0], lattice.bounds[1], native.ptr(counter), native.ptr(bin_lin), native.ptr(bin_ix),
        native.stream_handle()), 'vk_motility_step_static' if static else 'vk_motility_step')
    return bin_lin


def flagella_step(model: MotilityModel, lattice, location, motil, flag, flag_int, n: int, dt: float, counter,
                  key=None, bin_lin=None, bin_ix=None, substeps: Optional[int] = None):
    """One vk_flagella_step launch on the current stream: :func:`motility_step` with
    ``model.flagella``'s motor in the place of the coarse one, on ``flag``
    [VK_FLAG_ROWS, ld] (float64) and ``flag_int`` [VK_FLAGI_ROWS, ld] (int32).  A
    ``StaticField`` in the lattice's place: vk_flagella_step_static."""
    import torch
    from lens_amd.lattice import whole_plane
    from lens_amd.static_field import StaticField
    static = isinstance(lattice, StaticField)
    if model.flagella is None:
        raise ValueError('flagella_step: the model has no FlagellaModel')
    if not static and not whole_plane(lattice):
        raise ValueError('flagella_step: a whole, unbanded plane')
    ld = location.shape[1]
    if motil.shape != (native.VK_MOTIL_ROWS, ld) or not (motil.is_contiguous() and location.is_contiguous()):
        raise ValueError('flagella_step: motil must be [VK_MOTIL_ROWS, ld] beside location [2, ld], contiguous')
    if (flag.shape != (native.VK_FLAG_ROWS, ld) or flag.dtype != torch.float64 or not flag.is_contiguous() or
            flag_int.shape != (native.VK_FLAGI_ROWS, ld) or flag_int.dtype != torch.int32 or
            not flag_int.is_contiguous()):
        raise ValueError('flagella_step: flag must be float64 [VK_FLAG_ROWS, ld] and flag_int int32 '
                         '[VK_FLAGI_ROWS, ld], contiguous')
    if bin_lin is None:
        bin_lin = torch.zeros(ld, dtype=torch.int32, device=location.device)
    p, f = model.vk_params(), model.flagella.vk_params()
    if static:
        launch, ligand = native._lib.vk_flagella_step_static, ctypes.byref(lattice.spec(model.ligand_id))
    else:
        launch = native._lib.vk_flagella_step
        ligand = native.ptr(lattice.fields[lattice.molecules.index(model.ligand_id)])
    native.check(launch(
        ctypes.byref(p), ctypes.byref(f), n, ld, float(dt), int(model.substeps if substeps is None else substeps),
        native.ptr(motil), native.ptr(flag), native.ptr(flag_int), native.ptr(location), native.ptr(key),
        ligand, lattice.n_bins[0], lattice.n_bins[1], lattice.bounds[0], lattice.bounds[1],
        native.ptr(counter), native.ptr(bin_lin), native.ptr(bin_ix), native.stream_handle()),
        'vk_flagella_step_static' if static else 'vk_flagella_step')
    return bin_lin


class DeviceOccupancy:
    """Buffers of vk_occupancy_sort for up to ``ld`` agents: ``order`` and
    ``sorted_bin`` (int32 [ld]) and the sort's scratch, allocated once so that
    a captured graph keeps valid pointers."""

    def __init__(self, ld: int, device):
        import torch
        self.order = torch.zeros(ld, dtype=torch.int32, device=device)
        self.sorted_bin = torch.zeros(ld, dtype=torch.int32, device=device)
        nbytes = int(native._lib.vk_occupancy_scratch_bytes(ld))
        self.scratch = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
        self._off = (-self.scratch.data_ptr()) % 256     # the sort wants a 256-B aligned base
        self._bytes = nbytes

    def sort(self, bin_lin, n: int, n_bins: int, key=None):
        """order / sorted_bin [:n] := the agents by (bin, key) -- what
        lattice.occupancy computes on the host, without a host read."""
        if n > self.order.numel():
            raise ValueError('DeviceOccupancy: more agents than the buffers hold')
        native.check(native._lib.vk_occupancy_sort(
            native.ptr(bin_lin), native.ptr(key), n, int(n_bins), native.ptr(self.order),
            native.ptr(self.sorted_bin), self.scratch.data_ptr() + self._off, self._bytes,
            native.stream_handle()), 'vk_occupancy_sort')
        return self.order, self.sorted_bin
