"""NumPy restatement of a motile colony that grows and divides, for the tests: the
counts deriver of the flagella protein (vk_flagella_counts), the motile state's dividers
(vk_divide_flagella) and a whole-colony loop in the reference's order

    receptor + flagella motor + move   (tests/flagella_ref.py; motility_ref.py for the coarse motor)
    expression                         (ODE_expression.next_update, ode_expression.py:265-303)
    counts deriver                     (derive_counts.py:42-51, with the step-start mmol_to_counts)
    growth + mass / globals derivers   (oracle.colony.soa_step)
    division                           (Store.apply_update's _divide branch, experiment.py:664-697)

Random draws are oracle.colony.philox_uniform: the motor's by (motility seed, inner
update, agent key, 0, path), the growth remainder by (cell seed, step, root, depth,
path), the odd flagellum of a split count by (motility seed ^ DOMAIN, step, the mother's
root, depth, path).  The kinematics are this engine's, not the reference's multibody.
"""

import numpy as np

from oracle import colony as oc
from oracle.colony import philox_uniform

import flagella_ref as fref
import motility_ref as mref

DOMAIN = 0x666c6167656c6c61            # VK_DIVIDE_FLAGELLA_DOMAIN
MAX_FLAGELLA = 32
MERGED, SPLIT_DICT = 'merged', 'split_dict'
FI = fref.FI


def flagella_counts(conc, m2c):
    """(target int32 [n], flag): int(concentration * mmol_to_counts) clamped into 0..32;
    NaN and negative products give 0.  flag: some product lay outside [0, 33)."""
    with np.errstate(invalid='ignore', over='ignore'):
        counts = np.asarray(conc, dtype=np.float64) * np.asarray(m2c, dtype=np.float64)
        inside = (counts >= 0.0) & (counts < 33.0)
        t = np.trunc(counts)                             # int() truncates toward zero
        t = np.where(np.isnan(t) | (t < 0.0), 0.0, np.minimum(t, float(MAX_FLAGELLA)))
    return t.astype(np.int32), bool(np.any(~inside))


def split_int(t, u):
    """divide_split on ints (registry.py:205-227): (daughter 0, daughter 1); the remainder
    goes to daughter 0 exactly when u < 0.5."""
    t = np.asarray(t, dtype=np.int64)
    half = np.trunc(t / 2).astype(np.int64)              # int(state / 2)
    rest = t - 2 * half
    first = np.asarray(u) < 0.5
    return half + np.where(first, rest, 0), half + np.where(first, 0, rest)


def divide_draw(seed, step, root, depth, path):
    """The mother's coin: one draw for both daughters."""
    return philox_uniform(int(seed) ^ DOMAIN, int(step), int(root), int(depth), int(path))


def _clean(have, mask):
    """have in 0..32 and the uint64 mask without bits at and above it, as the motor reads them."""
    have = np.clip(np.asarray(have, dtype=np.int64), 0, MAX_FLAGELLA)
    mask = np.asarray(mask).astype(np.int32).view(np.uint32).astype(np.uint64)
    return have, mask & ((np.uint64(1) << have.astype(np.uint64)) - np.uint64(1))


def divide_have_mask(have, mask, mode):
    """((have0, mask0), (have1, mask1)) of mothers' have / int32 mask arrays.  'merged':
    deep_merge into a copy of the mother keeps every flagellum in both daughters (experiment.py:
    664-697, dict_utils.py:51-66).  'split_dict' (registry.py:246-262): daughter 0 gets the
    items [len // 2:], daughter 1 the items [:len // 2]."""
    have, mask = np.asarray(have, dtype=np.int32), np.asarray(mask, dtype=np.int32)
    if mode == MERGED:
        return (have.copy(), mask.copy()), (have.copy(), mask.copy())
    if mode != SPLIT_DICT:
        raise ValueError(mode)
    hv, m = _clean(have, mask)
    h = hv // 2
    hu = h.astype(np.uint64)
    m0, m1 = m >> hu, m & ((np.uint64(1) << hu) - np.uint64(1))
    as_i32 = lambda x: x.astype(np.uint32).view(np.int32)
    return ((hv - h).astype(np.int32), as_i32(m0)), (h.astype(np.int32), as_i32(m1))


def divide_flagella(flag_int, keys, order, n_keep, mode, seed, step, lineage, key_base, margins=None):
    """(flag_int', keys') in the layout ``order`` (oracle.colony.soa_step: survivors, then
    both daughters of each mother in mother order).  ``lineage`` = (root, depth, path) arrays
    of the agents BEFORE the division.  flag_int may be None (the coarse motor): keys only.
    Daughters get the keys key_base, key_base + 1, ... in slot order."""
    order = np.asarray(order, dtype=np.int64)
    n_out = len(order)
    new_keys = np.asarray(keys, dtype=np.int64)[order].copy()
    new_keys[n_keep:] = key_base + np.arange(n_out - n_keep)
    if flag_int is None:
        return None, new_keys
    out = np.asarray(flag_int, dtype=np.int32)[:, order].copy()
    mothers = order[n_keep::2]
    root, depth, path = lineage
    u = np.array([divide_draw(seed, step, root[a], depth[a], path[a]) for a in mothers], dtype=np.float64)
    t = flag_int[FI['target'], mothers]
    if margins is not None and (t % 2 != 0).any():
        margins['split'] = min(margins.get('split', 1.0), float(np.abs(u - 0.5)[t % 2 != 0].min()))
    t0, t1 = split_int(t, u)
    (h0, m0), (h1, m1) = divide_have_mask(flag_int[FI['have'], mothers], flag_int[FI['mask'], mothers], mode)
    out[FI['target'], n_keep::2], out[FI['target'], n_keep + 1::2] = t0, t1
    out[FI['have'], n_keep::2], out[FI['have'], n_keep + 1::2] = h0, h1
    out[FI['mask'], n_keep::2], out[FI['mask'], n_keep + 1::2] = m0, m1
    return out, new_keys


def expression_step(table, expr, dt):
    """ODE_expression.next_update without regulation, accumulated: every delta from the
    step-start state.  ``table``: a lens_amd.expression.ExpressionTable over expr's rows."""
    new = expr.copy()
    for j in range(len(table.transcripts)):
        r = table.tx_row[j]
        new[r] = expr[r] + (table.tx_rate[j] - table.tx_deg[j] * expr[r]) * dt
    for j in range(len(table.proteins)):
        r = table.tl_row[j]
        new[r] = expr[r] + (table.tl_rate[j] * expr[table.tl_mrna_row[j]] - table.tl_deg[j] * expr[r]) * dt
    return new


# The whole-colony case of the tests: 24 agents on 16 x 16 bins of 2 um, steps of 1 s in 10
# inner updates, GrowthProtein at rate 0.05 (a division every 14 s).  The expression runs at
# the reference's rates except the transcription rate, with the transcript started at its
# steady state rate / degradation: the protein then grows linearly, the count passes 0..9
# before the first division and stays below 33 through the second one.  (From a transcript
# of zero the protein grows quadratically: a rate that shows 8 flagella by the first
# division passes 33 at the second, where the colony must raise.)  SEED: the restatement's
# margins are all >= 1e-9 in both modes and an odd count is split (chosen on the CPU).
CASE_SEED = 20261020
CASE_N, CASE_BINS, CASE_BOUNDS, CASE_SUBSTEPS, CASE_GROWTH = 24, (16, 16), (32.0, 32.0), 10, 0.05
CASE_TRANSCRIPTION = 1.25e-4


def colony_case(mode, expression=True, flagella=True):
    """(MotilityModel, CellModel, n, locations, bounds) of the whole-colony case;
    ``expression=False``: five flagella set by hand, ``flagella=False``: the coarse motor."""
    from lens_amd import configs
    from lens_amd.cells import CellModel
    from lens_amd.motility import FlagellaModel, MotilityModel
    e = configs.flagella_expression()
    e['transcription_rates']['flag_RNA'] = CASE_TRANSCRIPTION
    e['initial_state']['internal']['flag_RNA'] = CASE_TRANSCRIPTION / e['degradation_rates']['flag_RNA']
    fm = None if not flagella else FlagellaModel(0, expression=e) if expression else FlagellaModel(5)
    model = MotilityModel(ligand_id='MeAsp', initial_ligand=1e-2, substeps=CASE_SUBSTEPS, seed=CASE_SEED,
                          division=mode, flagella=fm)
    cells = CellModel(rng='philox', growth_rate=CASE_GROWTH, seed=CASE_SEED + 1)
    loc = np.random.default_rng(CASE_SEED).uniform(0.0, CASE_BOUNDS[0], (2, CASE_N))
    return model, cells, CASE_N, loc, CASE_BOUNDS


class MotileColony:
    """The whole-colony loop.  State (host arrays over the n agents): ``motil`` [9, n],
    ``flag`` [5, n], ``flag_int`` [3, n] (None with the coarse motor), ``expr`` [keys, n] (None
    without expression), ``loc`` [2, n], ``cell`` (oracle.colony.soa_step's dict, or None
    without cells), ``m2c``, ``ids``, lineage ``root`` / ``depth`` / ``path``, ``keys``, ``bins``."""

    def __init__(self, model, cells, n, loc, bounds, mass_fg=1339.0):
        self.model, self.cells, self.bounds = model, cells, bounds
        self.n = n
        self.motil = model.initial_rows(n, n)
        self.flag = self.flag_int = self.expr = None
        fm = model.flagella
        if fm is not None:
            self.flag, self.flag_int = fm.initial_rows(n, n, model.seed)
            if fm.expression is not None:
                self.expr = np.repeat(fm.expression_initial[:, None], n, axis=1)
        self.loc = np.array(loc, dtype=np.float64)[:, :n].copy()
        self.keys = np.arange(n, dtype=np.int64)
        self.key_base = n
        self.counter = 0
        self.step_index = 0
        self.ids = [str(a) for a in range(n)]
        self.root = np.arange(n, dtype=np.int64)
        self.depth = np.zeros(n, dtype=np.int64)
        self.path = np.zeros(n, dtype=np.int64)
        self.cell = None
        if cells is not None:
            rows, m2c = cells.initial_rows(n)
            self.cell = {'mass': rows[0], 'volume': rows[1], 'length': rows[2], 'surface_area': rows[3],
                         'protein': rows[4], 'angle': self.motil[mref.R['angle']].copy(), 'm2c': m2c}
            self.m2c = m2c
        else:
            self.m2c = np.full(n, oc.N_A * (mass_fg / 1100.0 * 1e-15) * 1e-3)
        self.flagged = False
        if self.expr is not None:                        # the derivers run once at t = 0
            self.flag_int[FI['target']], bad = flagella_counts(self.expr[fm.count_row], self.m2c)
            self.flagged |= bad
        self.bins = None

    def step(self, field, dt, margins=None):
        """One colony step on the pre-step ligand plane ``field`` [nx, ny].  Returns the
        number of mothers that divided."""
        m, fm = self.model, self.model.flagella
        nx, ny = field.shape
        if fm is not None:
            self.bins = fref.step(m, self.motil, self.flag, self.flag_int, self.loc, field, self.bounds, dt,
                                  m.substeps, self.counter, keys=self.keys, margins=margins)
        else:
            self.bins = mref.step(m, self.motil, self.loc, field, self.bounds, dt, m.substeps, self.counter,
                                  keys=self.keys, margins=margins)
        self.counter += m.substeps
        if self.expr is not None:
            # the process from the step-start state, then its counts deriver, in front of
            # DeriveGlobals: the mmol_to_counts of the previous step
            self.expr = expression_step(fm.expression_table, self.expr, dt)
            self.flag_int[FI['target']], bad = flagella_counts(self.expr[fm.count_row], self.m2c)
            self.flagged |= bad
        mothers = 0
        if self.cell is not None:
            mothers = self._grow_and_divide(dt, (nx, ny), margins)
        self.step_index += 1
        return mothers

    def _grow_and_divide(self, dt, n_bins, margins):
        cm, n = self.cells, self.n
        self.cell['angle'] = self.motil[mref.R['angle']].copy()          # one heading
        u = np.array([philox_uniform(cm.seed, self.step_index, int(r), int(d), int(p))
                      for r, d, p in zip(self.root, self.depth, self.path)], dtype=np.float64)
        cell = dict(self.cell, x=self.loc[0], y=self.loc[1])
        cell, ids, order = oc.soa_step(cell, self.ids, cm.model, dt, u=u, rate=cm.growth_rate,
                                       division_volume=cm.division_volume, divide_protein=cm.initial_protein() * 2,
                                       width=float(cm.width))
        n_out = len(order)
        self.loc = np.stack([cell.pop('x'), cell.pop('y')])
        self.cell, self.m2c = cell, cell['m2c']
        if n_out == n:
            return 0
        n_keep = 2 * n - n_out
        self.motil = self.motil[:, order].copy()                         # no divider: the mother's values
        if self.flag is not None:
            self.flag = self.flag[:, order].copy()
        if self.expr is not None:
            self.expr = self.expr[:, order].copy()
        self.flag_int, self.keys = divide_flagella(self.flag_int, self.keys, order, n_keep, self.model.division,
                                                   self.model.seed, self.step_index,
                                                   (self.root, self.depth, self.path), self.key_base, margins)
        self.key_base += n_out - n_keep
        daughter = np.arange(n_out) >= n_keep
        k = np.where(daughter, (np.arange(n_out) - n_keep) % 2, 0)
        self.root = self.root[order]
        self.path = np.where(daughter, self.path[order] * 2 + k, self.path[order])
        self.depth = self.depth[order] + daughter
        self.ids, self.n = ids, n_out
        nx, ny = n_bins
        ix, iy = mref.bin_axis(self.loc[0], nx, self.bounds[0]), mref.bin_axis(self.loc[1], ny, self.bounds[1])
        self.bins = (ix * ny + iy).astype(np.int32)
        return n_out - n
