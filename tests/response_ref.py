"""Test helper: the antibiotic response restated in NumPy, one agent at a time in
store order.  Not product code; it is the comparison for every response test.

Per step, every process computes from the step-start state S, and the updates
are applied in the Antibiotics compartment's process order: kinetics, growth,
expression, death, division trigger, then the membrane diffusion last.

  membrane, per molecule m:   rate = 0 + porin_0 * perm_0 + porin_1 * perm_1 ...
                              flux_mmol = (int_m - ext_m) * rate * dt
                              delta_int = -(flux_mmol / volume_fL * 1e15)
                              counts    = flux_mmol * 1e-3 * N_A          (a float)
  death:                      dying = not frozen and any(S[key] > threshold)
  a frozen agent:             only the membrane term runs; its kinetic counts are 0
  application:                conc[int_m] = (conc + delta_kinetics) + delta_membrane
                              per agent: v = v + mM(int counts); v = v + mM(float counts)
"""

import numpy as np

from table_eval import table_euler

VOLUME_TO_FL = 1e-18 / 1e-3 * 1e18 * 1e-3


def mM(count, bva):
    return (float(count) / bva) * 1000.0


def membrane_terms(col, volume_fl, dt, avogadro, mol_int_row, mol_ext_row, porin_row, porin_perm):
    """(delta_int[m], counts[m]) of one agent from its state column."""
    rate = 0
    for r, perm in zip(porin_row, porin_perm):
        rate = rate + col[r] * perm
    delta, counts = [], []
    for ri, re in zip(mol_int_row, mol_ext_row):
        flux_mmol = (col[ri] - col[re]) * rate * dt
        delta.append(-(flux_mmol / volume_fl * 1e15))
        counts.append(flux_mmol * 1e-3 * avogadro)
    return delta, counts


def expression_update(col, ex, dt):
    """ODE_expression without regulation: [(row, delta)] transcripts then proteins."""
    out = []
    for j in range(len(ex.transcripts)):
        out.append((int(ex.tx_row[j]), (ex.tx_rate[j] - ex.tx_deg[j] * col[ex.tx_row[j]]) * dt))
    for j in range(len(ex.proteins)):
        out.append((int(ex.tl_row[j]), (ex.tl_rate[j] * col[ex.tl_mrna_row[j]] - ex.tl_deg[j] * col[ex.tl_row[j]]) * dt))
    return out


class RefColony:
    """State of n agents and one step of the response, agent after agent.

    conc [rows, n], params [P, n], m2c [n]; ``volume``: a float (no cells) or
    None with ``cells=(CellModel, cell rows [VK_CELL_ROWS, n])``.
    ``fields`` [n_planes, n_bins], ``bins`` [n]: the agent's bin (a nonspatial
    colony: bin a for agent a).  ``gather`` [(plane, row)], ``exch_int``
    [(count row e, plane)], ``exch_float`` [(molecule index m, plane)]."""

    def __init__(self, table, layout, conc, params, m2c, *, avogadro, bva, fields, bins, gather, exch_int,
                 exch_float, volume=None, cells=None, nonspatial=True):
        self.t, self.L = table, layout
        self.conc = np.array(conc, dtype=np.float64)
        self.params = np.array(params, dtype=np.float64)
        self.m2c = np.array(m2c, dtype=np.float64)
        self.n = self.conc.shape[1]
        self.avogadro, self.bva = avogadro, bva
        self.fields = np.array(fields, dtype=np.float64)
        self.bins = np.array(bins, dtype=np.int64)
        self.gather, self.exch_int, self.exch_float = list(gather), list(exch_int), list(exch_float)
        self.volume = volume
        self.cm, self.cell = (cells[0], np.array(cells[1], dtype=np.float64)) if cells is not None else (None, None)
        self.nonspatial = nonspatial
        self.dead = np.zeros(self.n, dtype=np.int32)
        self.frozen = np.zeros(self.n, dtype=np.int32)
        self.divide = np.zeros(self.n, dtype=np.int32)
        self.flux = np.zeros((table.n_reactions, self.n))
        self.counts = np.zeros((table.n_ext, self.n), dtype=np.int64)
        self.fcounts = np.zeros((len(layout.molecules), self.n))

    def gather_external(self, fields=None):
        f = self.fields if fields is None else fields
        for a in range(self.n):
            for plane, row in self.gather:
                self.conc[row, a] = f[plane, self.bins[a]]

    def step(self, dt=1.0, between=None):
        """One step.  ``between(self)`` (lattice colonies) runs after the per-agent
        updates were computed and the externals gathered, before the exchange: the
        diffusion of the planes."""
        t, L = self.t, self.L
        S = self.conc.copy()
        cell0 = None if self.cell is None else self.cell.copy()
        exchanges = []
        for a in range(self.n):
            col = S[:, a]
            vol = self.volume if self.cell is None else cell0[1, a]
            fr = bool(self.frozen[a])
            dying = (not fr) and any(col[r] > thr for r, thr in zip(L.det_row, L.det_thr))
            kcounts = np.zeros(t.n_ext, dtype=np.int64)
            if not fr:
                new, flux, kcounts = table_euler(t, col[:t.n_species], self.params[:, a], dt, self.m2c[a])
                self.conc[:t.n_dyn, a] = new[:t.n_dyn]
                self.flux[:, a] = flux
                if self.cell is not None:
                    self._grow(a, dt)
                if L.expression is not None:
                    for row, d in expression_update(col, L.expression, dt):
                        self.conc[row, a] = self.conc[row, a] + d
            self.counts[:, a] = kcounts
            fcounts = []
            if len(L.molecules):
                delta, fcounts = membrane_terms(col, vol, dt, self.avogadro, L.mol_int_row, L.mol_ext_row,
                                                L.porin_row, L.porin_perm)
                for m, ri in enumerate(L.mol_int_row):
                    self.conc[ri, a] = self.conc[ri, a] + delta[m]
                self.fcounts[:, a] = fcounts
            if dying:
                self.dead[a] = 1
                self.frozen[a] = 1
            exchanges.append((kcounts, fcounts))
        if not self.nonspatial:
            self.gather_external()          # the pre-step field (one-step lag)
        if between is not None:
            between(self)
        for a in range(self.n):
            kcounts, fcounts = exchanges[a]
            b = self.bins[a]
            planes = []
            for e, plane in self.exch_int:
                planes.append(plane)
            for m, plane in self.exch_float:
                if plane not in planes:
                    planes.append(plane)
            for plane in planes:
                v = self.fields[plane, b]
                for e, p in self.exch_int:
                    if p == plane:
                        v = v + mM(kcounts[e], self.bva)
                for m, p in self.exch_float:
                    if p == plane:
                        v = v + mM(fcounts[m], self.bva)
                self.fields[plane, b] = v
        if self.nonspatial:
            self.gather_external()

    def _grow(self, a, dt):
        """Growth + DivisionVolume + DeriveGlobals (growth.py:101-107, division_volume.py:39-45,
        derive_globals.py:131-152), model='growth'."""
        cm, c = self.cm, self.cell
        cap = cm.capsule()
        self.divide[a] = int(c[1, a] >= cm.division_volume)
        m = c[0, a] * float(np.exp(cm.growth_rate * dt))
        raw = m / cm.density
        length = (raw - cap['cap_volume']) / cap['cap_area'] + cap['two_r']
        c[0, a], c[1, a], c[2, a] = m, raw * VOLUME_TO_FL, length
        c[3, a] = cap['sa_const'] + cap['sa_lin'] * (length - cm.width)
        self.m2c[a] = cm.avogadro * (raw * 1e-15) * 1e-3

    def apply_division(self):
        """MetaDivision as the colony lays it out: survivors keep their order, the two
        daughters of each mother follow in mother order.  Concentrations, parameters,
        mmol_to_counts, fluxes, counts and ``dead`` are copied (the set divider),
        mass .. protein are halved, ``frozen`` and ``divide`` are 0 for daughters.
        Returns the source column of every new column (bins are the caller's)."""
        n = self.n
        mothers = [a for a in range(n) if self.divide[a]]
        if not mothers:
            return None
        src = [a for a in range(n) if not self.divide[a]] + [m for m in mothers for _ in (0, 1)]
        daughter = np.array([False] * (n - len(mothers)) + [True] * (2 * len(mothers)))
        for name in ('conc', 'params', 'flux', 'counts', 'fcounts', 'cell'):
            setattr(self, name, getattr(self, name)[:, src].copy())
        for name in ('m2c', 'dead', 'frozen', 'divide'):
            setattr(self, name, getattr(self, name)[src].copy())
        self.cell[:5, daughter] = self.cell[:5, daughter] / 2
        self.frozen[daughter] = 0
        self.divide[daughter] = 0
        self.n = len(src)
        return src

    def cell_counts(self, row):
        """counts deriver (derive_counts.py:42-51): int(conc * mmol_to_counts), post-step."""
        return np.trunc(self.conc[row] * self.m2c)


def two_pass_exchange(v, int_counts, float_counts, bva):
    """The order the colony must NOT use: all int counts of a bin, then all float counts."""
    for k in int_counts:
        v = v + mM(k, bva)
    for d in float_counts:
        v = v + mM(d, bva)
    return v


def interleaved_exchange(v, int_counts, float_counts, bva):
    for k, d in zip(int_counts, float_counts):
        v = v + mM(k, bva)
        v = v + mM(d, bva)
    return v


def initial_state(table, layout, kin, n):
    """conc [rows, n] as Colony allocates it: the kinetics' initial_state on the table's
    rows, the response's defaults on the rows it appended."""
    conc = np.zeros((layout.n_rows, n))
    for s, (port, name) in enumerate(table.species):
        conc[s, :] = float(kin.get('initial_state', {}).get(port, {}).get(name, 0.0))
    for row, value in layout.initial.items():
        conc[row, :] = value
    return conc


def nonspatial_ref(table, layout, kin, n, *, env_volume_L, avogadro, mass_fg=1339.0, cells=None, conc=None,
                   environment=None):
    """A RefColony set up as Colony(environment='nonspatial') sets itself up: each agent
    owns a 1 x 1 field of every molecule (1.0 at the start, or ``environment`` [mols, n]),
    copied into its external rows."""
    mols = []
    for e in list(table.external_ids) + [k[1] for k in table.species if k[0] == 'external'] + list(layout.molecules):
        if e not in mols:
            mols.append(e)
    gather = [(f, table.species.index(('external', mol))) for f, mol in enumerate(mols) if ('external', mol) in table.species]
    for m, mol in enumerate(layout.molecules):
        if int(layout.mol_ext_row[m]) not in [r for _, r in gather]:
            gather.append((mols.index(mol), int(layout.mol_ext_row[m])))
    exch_int = [(e, mols.index(mol)) for e, mol in enumerate(table.external_ids) if mol in mols]
    exch_float = [(m, mols.index(mol)) for m, mol in enumerate(layout.molecules)]
    bva = ((env_volume_L * 1e15 * 1.0 * 1.0) * 1e-15 / 1) * avogadro
    raw = mass_fg / 1100.0
    if cells is not None:
        rows, m2c = cells.initial_rows(n)
        cells = (cells, rows)
    else:
        m2c = np.full(n, avogadro * (raw * 1e-15) * 1e-3)
    fields = np.ones((len(mols), n)) if environment is None else np.array(environment, dtype=np.float64)
    rc = RefColony(table, layout, initial_state(table, layout, kin, n) if conc is None else conc,
                   np.repeat(table.param_defaults[:, None], n, axis=1), m2c, avogadro=avogadro, bva=bva, fields=fields,
                   bins=np.arange(n), gather=gather, exch_int=exch_int, exch_float=exch_float,
                   volume=raw * VOLUME_TO_FL, cells=cells)
    rc.molecules = mols
    rc.gather_external()
    return rc


# the death known answers: (porin, external mM) -> first row with dead == 1 (None: never in 64 steps)
DEATH_CASES = [(1.2e-16, 2.0, 38), (2.4e-16, 2.0, 19), (4.8e-16, 2.0, 10), (2.4e-15, 2.0, 3), (1e-20, 2.0, None)] + \
    [(p, 0.9, None) for p in (1.2e-16, 2.4e-16, 4.8e-16, 2.4e-15, 1e-20, 6e-17)]
