"""Antibiotic response of a device-resident colony: pump expression, porin
diffusion across the membrane, death.

The reference's ``Antibiotics`` compartment (vivarium/compartments/
antibiotics.py:35-159) composes, per cell, ``AntibioticTransport`` (a
ConvenienceKinetics export through the AcrAB-TolC pump), ``Growth``,
``ODE_expression`` (which makes the pump), ``DeathFreezeState``,
``DivisionVolume`` and ``CellEnvironmentDiffusion``.  Kinetics, growth and
division are the colony's own; a :class:`CellResponse` carries the other three
and ``Colony(..., response=...)`` runs them on the device:

expression
    ``vk_expression_step`` (lens_amd/expression.py) from the step-start state
    into an update buffer, applied at the end of the step.
membrane (diffusion_cell_environment.py:92-138)
    ``rate = sum(porin * permeability)``; ``flux_mmol = (int - ext) * rate * dt``;
    the internal concentration takes ``-(flux_mmol / volume_fL * 1e15)`` and the
    field takes the *float* count ``flux_mmol * 1e-3 * N_A`` at the agent's bin.
    The process reads ``parameters['permeabilities']`` (default ``{'porin':
    1e-1}``); the compartment passes ``permeability_per_porin``, which the process
    never looks at -- the config reader keeps that quirk.
death (death.py:105-118, 197-219)
    ``dying = not frozen and any(state[key] > threshold)`` from the step-start
    state; the step of detection still applies every update; from the next step
    on the cell's kinetics, growth, expression, division trigger and detector do
    nothing, while the membrane keeps leaking.

Ports: in the Antibiotics topology ``internal``, ``pump_port`` and ``membrane``
are all the store ``('cell',)``, so a name under any of ``cell_ports`` is one
state row.  A name resolves to the kinetics table's species row whose port is in
that set, otherwise it gets a new row after the table's ``n_species`` rows.
"""

from __future__ import annotations

import copy
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from lens_amd.expression import ExpressionTable, parse_rule
from lens_amd.process import ProcessBase, deep_merge

CELL_PORTS = ('internal', 'pump_port', 'membrane')

# CellEnvironmentDiffusion.defaults (diffusion_cell_environment.py:17-28)
MEMBRANE_DEFAULTS = {
    'molecules_to_diffuse': [],
    'default_state': {},
    'default_default': 0,
    'permeabilities': {'porin': 1e-1},
}

# AntibioticTransport.defaults (antibiotic_transport.py:31-39)
ANTIBIOTIC_TRANSPORT_DEFAULTS = {
    'pump_kcat': 2e-4, 'pump_km': 0.6, 'pump_key': 'AcrAB-TolC', 'antibiotic_key': 'antibiotic',
    'initial_internal_antibiotic': 0, 'initial_external_antibiotic': 1, 'initial_pump': 1,
}

# Antibiotics.defaults (antibiotics.py:37-98), the compartment's overrides of its processes
ANTIBIOTICS_DEFAULTS = {
    'ode_expression': {
        'transcription_rates': {'AcrAB-TolC_RNA': 1e-3},
        'translation_rates': {'AcrAB-TolC': 1.0},
        'degradation_rates': {'AcrAB-TolC_RNA': 1.0, 'AcrAB-TolC': 1e-3},
        'protein_map': {'AcrAB-TolC': 'AcrAB-TolC_RNA'},
    },
    'antibiotic_transport': {
        'initial_pump': 0.0, 'initial_internal_antibiotic': 0.5, 'initial_external_antibiotic': 1,
        'pump_kcat': 5e-4,
    },
    'death': {
        'detectors': {'antibiotic': {'antibiotic_threshold': 0.95}},
        'targets': ['antibiotic_transport', 'growth', 'expression', 'death', 'division'],
    },
    'growth': {'growth_rate': math.log(2) / 2400},
    'division': {},
    'diffusion': {
        'default_state': {
            'membrane': {'porin': 1e-20},
            'external': {'antibiotic': 1},
            'internal': {'antibiotic': 0.5},
        },
        'molecules_to_diffuse': ['antibiotic'],
        'permeability_per_porin': {'porin': 5e-3},      # never read by the process
    },
}

# AntibioticDetector's arguments (death.py:85-87)
DETECTOR_DEFAULTS = {'antibiotic': {'antibiotic_threshold': 0.9, 'antibiotic_key': 'antibiotic'}}


def antibiotic_transport_config(parameters=None):
    """The ConvenienceKinetics configuration AntibioticTransport builds
    (antibiotic_transport.py:50-89)."""
    p = dict(ANTIBIOTIC_TRANSPORT_DEFAULTS)
    p.update(parameters or {})
    pump, drug = ('pump_port', p['pump_key']), p['antibiotic_key']
    return {
        'reactions': {
            'export': {
                'stoichiometry': {('internal', drug): -1, ('external', drug): 1},
                'is_reversible': False,
                'catalyzed by': [pump],
            },
        },
        'kinetic_parameters': {
            'export': {pump: {'kcat_f': p['pump_kcat'], ('internal', drug): p['pump_km']}},
        },
        'initial_state': {
            'fluxes': {'import': 0.0, 'export': 0.0},
            'internal': {drug: p['initial_internal_antibiotic']},
            'external': {drug: p['initial_external_antibiotic']},
            'pump_port': {p['pump_key']: p['initial_pump']},
        },
        'port_ids': ['internal', 'external', 'pump_port'],
    }


def _rule_keys(tree, out):
    if tree[0] in ('and', 'or'):
        _rule_keys(tree[1], out)
        _rule_keys(tree[2], out)
    elif tree[0] == 'not':
        _rule_keys(tree[1], out)
    elif tree[1][0] == 'key':
        out.append(tuple(tree[1][1]))


class ResponseLayout:
    """A :class:`CellResponse` bound to a kinetics table: the rows of ``conc``
    (the table's species, then the appended ones) and every index the kernels walk."""

    def __init__(self, response: 'CellResponse', table):
        r = response
        self.cell_ports = r.cell_ports
        self.keys: List[Tuple[str, str]] = [tuple(k) for k in table.species]
        self.n_table = len(self.keys)
        self.n_dyn = table.n_dyn
        self.initial: Dict[int, float] = {}

        # expression: every key the configuration names gets a row
        self.expression = None
        self.expr_rows = np.zeros(0, dtype=np.int32)
        if r.expression is not None:
            e = r.expression
            names = list(e.get('transcription_rates', {})) + list(e.get('translation_rates', {}))
            names += list(e.get('protein_map', {}).values())
            wanted = [('internal', s) for s in names]
            for rule in e.get('regulation', {}).values():
                _rule_keys(parse_rule(rule), wanted)
            wanted += [tuple(k) for k in e.get('regulators', [])]
            for key in wanted:
                self.row(key, create=True)
            for port, states in e.get('initial_state', {}).items():
                for name, value in states.items():
                    row = self.row((port, name), create=True)
                    if row >= self.n_table:
                        self.initial[row] = float(value)

        # membrane
        self.molecules: List[str] = []
        self.porins: List[str] = []
        self.mol_int_row = self.mol_ext_row = self.porin_row = np.zeros(0, dtype=np.int32)
        self.porin_perm = np.zeros(0, dtype=np.float64)
        if r.membrane is not None:
            m = r.membrane
            self.molecules = list(m['molecules_to_diffuse'])
            self.mol_int_row = np.array([self.row(('internal', s), create=True) for s in self.molecules], dtype=np.int32)
            # the agent's ('external', m) row, added even when no rate law mentions it
            self.mol_ext_row = np.array([self.row(('external', s), create=True) for s in self.molecules], dtype=np.int32)
            for port, states in m['default_state'].items():
                if port == 'global':
                    continue
                for name, value in states.items():
                    row = self.row((port, name), create=True)
                    if row >= self.n_table:
                        self.initial[row] = float(getattr(value, 'magnitude', value))
            self.porins = list(m['permeabilities'])
            self.porin_row = np.array([self.row(('membrane', p), create=False, what='porin') for p in self.porins],
                                      dtype=np.int32)
            self.porin_perm = np.array([float(m['permeabilities'][p]) for p in self.porins], dtype=np.float64)

        # death
        self.det_row = np.zeros(0, dtype=np.int32)
        self.det_thr = np.zeros(0, dtype=np.float64)
        if r.death is not None:
            rows, thr = [], []
            for name, conf in r.death['detectors'].items():
                d = dict(DETECTOR_DEFAULTS[name])
                d.update(conf)
                rows.append(self.row(('internal', d['antibiotic_key']), create=False, what='detector key'))
                thr.append(float(d['antibiotic_threshold']))
            self.det_row = np.array(rows, dtype=np.int32)
            self.det_thr = np.array(thr, dtype=np.float64)

        if r.expression is not None:
            # the expression table looks its keys up under 'internal': every cell-store row
            # goes by that port (a second row of the same name keeps its own port)
            seen, ekeys = set(), []
            for port, name in self.keys:
                k = ('internal', name) if port in self.cell_ports else (port, name)
                if k in seen:
                    k = ('%s#%d' % (port, len(ekeys)), name)
                seen.add(k)
                ekeys.append(k)
            self.expression = ExpressionTable(r.expression, ekeys)
            self.expr_rows = np.concatenate([self.expression.tx_row, self.expression.tl_row]).astype(np.int32)

    @property
    def n_rows(self):
        return len(self.keys)

    def find(self, key):
        port, name = key
        for row, (p, s) in enumerate(self.keys):
            if s == name and (p == port or (port in self.cell_ports and p in self.cell_ports)):
                return row
        return None

    def row(self, key, create=False, what='key'):
        row = self.find(tuple(key))
        if row is None:
            if not create:
                raise ValueError('response: %s %r resolves to no state row (rows: %s)' % (what, tuple(key), self.keys))
            self.keys.append(tuple(key))
            row = len(self.keys) - 1
        return row

    def external_molecules(self):
        return list(self.molecules)


class CellResponse:
    """Expression, membrane diffusion and death of one cell type.

    ``expression``: an ``ODE_expression`` configuration or None.
    ``membrane``: a ``CellEnvironmentDiffusion`` configuration or None.
    ``death``: ``{'detectors': {'antibiotic': {...}}}`` or None.  The set of
    processes a dead cell loses is fixed (the reference compartment's).
    """

    def __init__(self, expression=None, membrane=None, death=None, cell_ports: Sequence[str] = CELL_PORTS):
        self.cell_ports = tuple(cell_ports)
        if not self.cell_ports or any(not isinstance(p, str) for p in self.cell_ports):
            raise ValueError('cell_ports: a non-empty sequence of port names')
        if 'external' in self.cell_ports:
            raise ValueError('cell_ports: the external port is the environment\'s, not the cell store')
        if expression is None and membrane is None and death is None:
            raise ValueError('CellResponse: give expression, membrane or death')
        self.expression = None
        if expression is not None:
            e = copy.deepcopy(dict(expression))
            for k in ('transcription_rates', 'translation_rates', 'degradation_rates', 'protein_map', 'regulation'):
                if not isinstance(e.setdefault(k, {}), dict):
                    raise ValueError('expression: %s must be a dict' % k)
            for p in e['translation_rates']:
                if p not in e['protein_map']:
                    raise ValueError('expression: protein %r has no protein_map entry' % p)
            for p, t in e['protein_map'].items():
                if t not in e['transcription_rates']:
                    raise ValueError('expression: protein_map sends %r to %r, which has no transcription rate' % (p, t))
            leak = e.get('transcription_leak', {'rate': 0.0, 'magnitude': 0.0})
            if float(leak.get('rate', 0.0)) != 0.0:
                raise ValueError('expression: a transcription leak draws random numbers; a colony response takes none')
            for rule in e['regulation'].values():
                parse_rule(rule)
            self.expression = e
        self.membrane = None
        if membrane is not None:
            m = deep_merge(copy.deepcopy(MEMBRANE_DEFAULTS), copy.deepcopy(dict(membrane)))
            mols = m['molecules_to_diffuse']
            if not isinstance(mols, (list, tuple)) or not mols or len(set(mols)) != len(mols):
                raise ValueError('membrane: molecules_to_diffuse must list distinct molecules')
            if not isinstance(m['permeabilities'], dict) or not m['permeabilities']:
                raise ValueError('membrane: permeabilities must map a porin to its permeability')
            for p, v in m['permeabilities'].items():
                if not math.isfinite(float(v)):
                    raise ValueError('membrane: permeability of %r is not finite' % p)
            self.membrane = m
        self.death = None
        if death is not None:
            d = copy.deepcopy(dict(death))
            if 'targets' in d and sorted(d['targets']) != sorted(ANTIBIOTICS_DEFAULTS['death']['targets']):
                raise ValueError('death: the freeze set is fixed (the Antibiotics compartment\'s targets)')
            det = d.get('detectors')
            if not isinstance(det, dict) or not det:
                raise ValueError('death: detectors must name at least one detector')
            for name, conf in det.items():
                if name not in DETECTOR_DEFAULTS:
                    raise ValueError('death: unknown detector %r (known: %s)' % (name, sorted(DETECTOR_DEFAULTS)))
                for k in conf:
                    if k not in DETECTOR_DEFAULTS[name]:
                        raise ValueError('death: detector %r takes no %r' % (name, k))
                thr = dict(DETECTOR_DEFAULTS[name], **conf)['antibiotic_threshold']
                if math.isnan(float(thr)):
                    raise ValueError('death: detector %r has a NaN threshold' % name)
            self.death = d

    def bind(self, table) -> ResponseLayout:
        return ResponseLayout(self, table)

    @staticmethod
    def from_antibiotics(config=None):
        return from_antibiotics(config)


def from_antibiotics(config=None):
    """``(kinetics_config, response)`` as the Antibiotics compartment configures its
    processes (antibiotics.py:37-122): AntibioticTransport's ConvenienceKinetics
    configuration for ``Colony(config, ...)`` and the :class:`CellResponse` for
    ``response=``.  ``config`` is deep-merged over the compartment's defaults; its
    growth rate is ``ANTIBIOTICS_DEFAULTS['growth']['growth_rate']``."""
    merged = deep_merge(copy.deepcopy(ANTIBIOTICS_DEFAULTS), copy.deepcopy(config or {}))
    kinetics = antibiotic_transport_config(merged['antibiotic_transport'])
    response = CellResponse(expression=merged['ode_expression'], membrane=merged['diffusion'],
                            death={'detectors': merged['death']['detectors']})
    return kinetics, response


class ResponseBuffers:
    """Per-agent scratch of one response step for ``ld`` agents (not gathered by
    division: every value is written before it is read within a step)."""

    def __init__(self, layout: ResponseLayout, ld: int, n_flux: int, device, cells: bool):
        import torch
        from lens_amd import native
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=device)
        self.dying = z(ld, dtype=torch.int32)
        self.delta = z(max(len(layout.molecules), 1), ld)
        self.fcounts = z(max(len(layout.molecules), 1), ld)
        self.save_conc = z(max(layout.n_dyn, 1), ld)
        self.save_flux = z(max(n_flux, 1), ld)
        self.save_status = z(ld, dtype=torch.int32)
        self.save_nsteps = z(ld, dtype=torch.int32)
        self.expr_update = z(len(layout.expr_rows), ld) if layout.expression is not None else None
        if cells:
            self.save_cell = z(native.VK_CELL_ROWS, ld)
            self.save_m2c = z(ld)
            self.save_divide = z(ld, dtype=torch.int32)


class ResponseEngine:
    """A :class:`ResponseLayout` resident on one GPU: the descriptor arrays and the
    launches of vk_response_begin / vk_response_end / vk_response_cells."""

    def __init__(self, layout: ResponseLayout, device, avogadro: float, volume_fl: float, n_flux: int, n_ext: int):
        import torch
        from lens_amd import native
        from lens_amd.expression import ExpressionEngine
        native.load()
        self.layout, self.device = layout, native.resolve_device(device)
        self.avogadro, self.volume_fl, self.n_flux, self.n_ext = float(avogadro), float(volume_fl), int(n_flux), int(n_ext)
        save_row = np.arange(layout.n_dyn, dtype=np.int32)     # the kinetics' dynamic rows
        self._dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(self.device) for k, v in (
            ('mol_int_row', layout.mol_int_row), ('mol_ext_row', layout.mol_ext_row),
            ('porin_row', layout.porin_row), ('porin_perm', layout.porin_perm), ('det_row', layout.det_row),
            ('det_thr', layout.det_thr), ('save_row', save_row), ('expr_row', layout.expr_rows))}
        self.expression = ExpressionEngine(layout.expression, self.device) if layout.expression is not None else None

    def table(self):
        from lens_amd import native
        t, L = native.VkResponseTable(), self.layout
        t.n_mol, t.n_porin, t.n_det = len(L.molecules), len(L.porins), len(L.det_row)
        t.n_save, t.n_expr, t.n_flux, t.n_ext = L.n_dyn, len(L.expr_rows), self.n_flux, self.n_ext
        for k, v in self._dev.items():
            setattr(t, k, v.data_ptr() if v.numel() else None)
        t.avogadro, t.volume_fl = self.avogadro, self.volume_fl
        return t

    def begin(self, dt, n, conc, volume, frozen, buf: ResponseBuffers, flux, status, nsteps, expression=True):
        """Detector, membrane terms and the frozen agents' saved columns; then the
        expression update from the same step-start state (accumulate = 0;
        ``expression=False``: the first launch alone, for timing)."""
        import ctypes
        from lens_amd import native
        t, ld = self.table(), conc.shape[1]
        native.check(native._lib.vk_response_begin(
            ctypes.byref(t), n, ld, float(dt), native.ptr(conc), native.ptr(volume), native.ptr(frozen),
            native.ptr(buf.dying), native.ptr(buf.delta), native.ptr(buf.fcounts), native.ptr(buf.save_conc),
            native.ptr(flux), native.ptr(buf.save_flux), native.ptr(status), native.ptr(buf.save_status),
            native.ptr(nsteps), native.ptr(buf.save_nsteps), native.stream_handle()), 'vk_response_begin')
        if expression and self.expression is not None:
            self.expression.step(dt, conc, n, update=buf.expr_update, accumulate=False)

    def end(self, n, conc, frozen, dead, buf: ResponseBuffers, flux, status, nsteps, counts):
        import ctypes
        from lens_amd import native
        t, ld = self.table(), conc.shape[1]
        native.check(native._lib.vk_response_end(
            ctypes.byref(t), n, ld, native.ptr(conc), native.ptr(buf.delta), native.ptr(buf.expr_update),
            native.ptr(frozen), native.ptr(buf.dying), native.ptr(dead), native.ptr(buf.save_conc), native.ptr(flux),
            native.ptr(buf.save_flux), native.ptr(status), native.ptr(buf.save_status), native.ptr(nsteps),
            native.ptr(buf.save_nsteps), native.ptr(counts), native.stream_handle()), 'vk_response_end')

    def cells(self, restore, n, frozen, cell, m2c, divide, buf: ResponseBuffers):
        from lens_amd import native
        native.check(native._lib.vk_response_cells(
            int(bool(restore)), n, cell.shape[1], native.ptr(frozen), native.ptr(buf.dying), native.ptr(cell),
            native.ptr(m2c),
            native.ptr(divide), native.ptr(buf.save_cell), native.ptr(buf.save_m2c), native.ptr(buf.save_divide),
            native.stream_handle()), 'vk_response_cells')


# -- Process API (host Python over lens_amd.engine.Experiment) ---------------------------

class BatchedCellEnvironmentDiffusion(ProcessBase):
    """Process-API drop-in for ``CellEnvironmentDiffusion``
    (diffusion_cell_environment.py:14-138): the reference's ``name``, ``defaults``,
    ``ports_schema`` and update dict; ``next_update`` runs a batch of one through
    vk_response_begin, as :class:`~lens_amd.expression.BatchedODEExpression` does."""

    name = 'cell_environment_diffusion'
    defaults = {
        'molecules_to_diffuse': [],
        'default_state': {'global': {'volume': 1.2}},      # fL
        'default_default': 0,
        'permeabilities': {'porin': 1e-1},
        'avogadro': 6.02214076e23,                         # scipy.constants.N_A of today (the golden: N_A_LEGACY)
    }

    def __init__(self, parameters=None):
        super().__init__(parameters)
        self._dev = None

    def ports_schema(self):
        p = self.parameters
        dd = p['default_default']
        schema = {
            'internal': {m: {'_default': dd, '_divider': 'set'} for m in p['molecules_to_diffuse']},
            'external': {m: {'_default': dd, '_divider': 'set'} for m in p['molecules_to_diffuse']},
            'membrane': {porin: {'_default': dd, '_emit': True} for porin in p['permeabilities']},
            'fields': {m: {'_default': np.full((1, 1), dd)} for m in p['molecules_to_diffuse']},
            'global': {'volume': {'_default': dd}, 'location': {'_default': [0.5, 0.5]}},
            'dimensions': {'bounds': {'_default': [1, 1]}, 'n_bins': {'_default': [1, 1]}, 'depth': {'_default': 1}},
        }
        for port, conf in p['default_state'].items():
            for variable, default in conf.items():
                schema[port][variable]['_default'] = default
        return schema

    def next_update(self, timestep, states):
        import ctypes
        import torch
        from lens_amd import native
        p = self.parameters
        mols, porins = list(p['molecules_to_diffuse']), list(p['permeabilities'])
        nm, npn = len(mols), len(porins)
        mag = lambda x: float(getattr(x, 'magnitude', x))
        # one agent: rows = internal molecules, external molecules, porins
        col = [mag(states['internal'][m]) for m in mols] + [mag(states['external'][m]) for m in mols] + \
              [mag(states['membrane'][q]) for q in porins]
        native.load()
        dev = native.resolve_device(None)
        if self._dev is None:
            i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
            self._dev = (i32(list(range(nm))), i32(list(range(nm, 2 * nm))), i32(list(range(2 * nm, 2 * nm + npn))),
                         torch.tensor([float(p['permeabilities'][q]) for q in porins], dtype=torch.float64, device=dev))
        t = native.VkResponseTable()
        t.n_mol, t.n_porin = nm, npn
        t.mol_int_row, t.mol_ext_row, t.porin_row, t.porin_perm = (x.data_ptr() if x.numel() else None for x in self._dev)
        t.avogadro, t.volume_fl = float(p['avogadro']), mag(states['global']['volume'])
        conc = torch.tensor([[v] for v in col], dtype=torch.float64, device=dev).reshape(len(col), 1).contiguous()
        z = lambda rows, dtype=torch.float64: torch.zeros((max(rows, 1), 1), dtype=dtype, device=dev)
        frozen, dying, delta, counts = z(1, torch.int32), z(1, torch.int32), z(nm), z(nm)
        if nm:
            native.check(native._lib.vk_response_begin(
                ctypes.byref(t), 1, 1, float(timestep), native.ptr(conc), None, native.ptr(frozen), native.ptr(dying),
                native.ptr(delta), native.ptr(counts), None, None, None, None, None, None, None,
                native.stream_handle()), 'vk_response_begin')
        delta, counts = delta.cpu().numpy()[:, 0], counts.cpu().numpy()[:, 0]
        return {
            'fields': {m: {'_value': float(counts[i]),
                           '_updater': {'updater': 'update_field_with_exchange',
                                        'port_mapping': {'global': 'global', 'dimensions': 'dimensions'}}}
                       for i, m in enumerate(mols)},
            'internal': {m: float(delta[i]) for i, m in enumerate(mols)},
        }


class DeathFreezeState(ProcessBase):
    """Process-API restatement of ``DeathFreezeState`` (death.py:127-219): when a
    detector fires, ``dead`` is set and the ``targets`` processes are deleted from
    the compartment (lens_amd.engine.Experiment honours ``_delete``)."""

    name = 'death'

    def __init__(self, initial_parameters=None):
        initial_parameters = initial_parameters or {}
        self.detectors = []
        for name, conf in initial_parameters.get('detectors', {}).items():
            if name not in DETECTOR_DEFAULTS:
                raise KeyError(name)
            d = dict(DETECTOR_DEFAULTS[name])
            d.update(conf)
            self.detectors.append((d['antibiotic_key'], d['antibiotic_threshold']))
        self.targets = initial_parameters.get('targets', [])
        super().__init__(initial_parameters)

    def ports_schema(self):
        schema = {'global': {'dead': {'_default': 0, '_emit': True, '_updater': 'set'}},
                  'processes': {target: {'_default': None} for target in self.targets}}
        for key, _ in self.detectors:
            schema.setdefault('internal', {})[key] = {'_default': 0}
        return schema

    def next_update(self, timestep, states):
        for key, threshold in self.detectors:
            if states['internal'][key] > threshold:      # strictly above (death.py:116)
                return {'global': {'dead': 1},
                        'processes': {'_delete': [(target,) for target in self.targets]}}
        return {}
