"""Stochastic mass-action kinetics per agent: batched Gillespie steps.

The reference integrates ``Complexation`` (vivarium/processes/complexation.py:74,120)
with the Gillespie direct method of ``arrow.StochasticSystem``.  Here a network is
packed once into a few small device arrays (:class:`StochasticModel`,
:class:`StochasticEngine`) and every agent of a colony advances by one launch per
timestep (vk_ssa_step): one agent per lane, her counts a column of an int32
``[species][ld]`` array, her draws keyed by a key of her own.

This is NOT arrow's arithmetic nor its random stream.  The step is stated above
``vk_ssa_step`` in include/vk_kinetics.h and restated in NumPy by tests/ssa_ref.py;
DESIGN.md §17 says what is and what is not the reference.

``Colony(..., stochastic=StochasticModel(...))`` keeps the counts (``ssa``) and the
keys (``ssa_key``) per agent, steps them at the end of every timestep and divides
them with the reference's ``divide_split`` (vk_divide_counts).
"""

from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np

from lens_amd import native

MAX_SPECIES, MAX_REACTIONS, MAX_ORDER = native.VK_SSA_MAX_SPECIES, native.VK_SSA_MAX_REACTIONS, native.VK_SSA_MAX_ORDER
MAX_PASSIVE = 192                      # further rows of the count table that no reaction names
DIVIDER_NAMES = ('set', 'split')       # what a count row may declare (StochasticModel(dividers=...))
STATUS_NAMES = ((native.VK_SSA_MAX_EVENTS, 'max_events reached'), (native.VK_SSA_NONFINITE, 'propensity not finite'),
                (native.VK_SSA_OVERFLOW, 'a count would pass 2**31 - 1'), (native.VK_SSA_BAD_KEY, 'key outside [0, 2**31)'))


def describe_status(bits: int) -> str:
    return ', '.join(text for bit, text in STATUS_NAMES if bits & bit) or 'ok'


def _whole(value, what):
    """An int from an int or a float with an integral value (the reference writes -4.0)."""
    if isinstance(value, (bool, np.bool_)):
        raise ValueError('%s: %r is not a whole number' % (what, value))
    try:
        f = float(value)
    except (TypeError, ValueError):
        raise ValueError('%s: %r is not a whole number' % (what, value))
    if f != f or f in (float('inf'), float('-inf')) or f != int(f):
        raise ValueError('%s: %r is not a whole number' % (what, value))
    return int(f)


class StochasticModel:
    """A mass-action network in the reference's shape.

    ``species``: the ids, in row order.  ``stoichiometry``: ``{reaction: {species: int}}``;
    a negative entry makes the species a reactant of that order.  ``rates``:
    ``{reaction: rate}`` (or a sequence in the stoichiometry's order).  ``initial``:
    ``{species: count}`` (default 0) every agent starts with.  The reactions keep the
    stoichiometry's order; within a reaction the species are sorted by row.

    ``passive``: ids of further rows of the count table, after the ``species`` rows, that no
    reaction may name (at most 192).  The network's launches stage and read the ``species`` rows
    only; translation, transcription and degradation may write any row (:attr:`rows`), and
    division splits them all.  ``n_species`` and the packed arrays stay the network's own.

    ``dividers``: ``{row: 'set' | 'split'}`` over any rows, active or passive (default
    ``'split'``): both daughters of a mother keep her count of a ``'set'`` row, as the
    reference's flagella agent keeps its regulators and its RNase ('_divider': 'set',
    flagella_expression.py:73-90).  It changes nothing but division."""

    def __init__(self, species: Sequence[str], stoichiometry: Dict[str, Dict[str, int]], rates,
                 initial: Optional[Dict[str, int]] = None, seed: int = 0, max_events: int = 100000,
                 passive: Sequence[str] = (), dividers: Optional[Dict[str, str]] = None):
        self.species = [str(s) for s in species]
        self.passive = [str(s) for s in passive]
        if len(set(self.species + self.passive)) != len(self.species) + len(self.passive):
            raise ValueError('stochastic: species ids must be distinct')
        self.dividers = {}
        for name, divider in (dividers or {}).items():
            if name not in self.species and name not in self.passive:
                raise ValueError('stochastic: dividers names the unknown row %r' % (name,))
            if divider not in DIVIDER_NAMES:
                raise ValueError('stochastic: the divider of %r must be one of %s (got %r)' % (
                    name, sorted(DIVIDER_NAMES), divider))
            self.dividers[str(name)] = divider
        S = len(self.species)
        if not 1 <= S <= MAX_SPECIES:
            raise ValueError('stochastic: 1..%d species (got %d)' % (MAX_SPECIES, S))
        if len(self.passive) > MAX_PASSIVE:
            raise ValueError('stochastic: at most %d passive rows (got %d)' % (MAX_PASSIVE, len(self.passive)))
        if not isinstance(stoichiometry, dict):
            raise ValueError('stochastic: stoichiometry must be {reaction: {species: int}}')
        self.reactions = list(stoichiometry.keys())
        R = len(self.reactions)
        if not 1 <= R <= MAX_REACTIONS:
            raise ValueError('stochastic: 1..%d reactions (got %d)' % (MAX_REACTIONS, R))
        row = {s: i for i, s in enumerate(self.species)}
        self.matrix = np.zeros((R, S), dtype=np.int64)
        for r, rid in enumerate(self.reactions):
            for sp, value in stoichiometry[rid].items():
                if sp in self.passive:
                    raise ValueError('stochastic: reaction %r names the passive row %r (a row a reaction names '
                                     'belongs in species)' % (rid, sp))
                if sp not in row:
                    raise ValueError('stochastic: reaction %r names the unknown species %r' % (rid, sp))
                v = _whole(value, 'stochastic: stoichiometry of %r in %r' % (sp, rid))
                if v < -MAX_ORDER:
                    raise ValueError('stochastic: reactant order %d of %r in %r exceeds %d' % (-v, sp, rid, MAX_ORDER))
                if v > 2 ** 31 - 1:
                    raise ValueError('stochastic: stoichiometry of %r in %r does not fit int32' % (sp, rid))
                self.matrix[r, row[sp]] = v
        if isinstance(rates, dict):
            unknown = set(rates) - set(self.reactions)
            if unknown:
                raise ValueError('stochastic: rates for unknown reactions %s' % sorted(map(str, unknown)))
            missing = [rid for rid in self.reactions if rid not in rates]
            if missing:
                raise ValueError('stochastic: no rate for %s' % missing)
            rates = [rates[rid] for rid in self.reactions]
        self.rates = np.asarray(rates, dtype=np.float64).reshape(-1)
        if self.rates.shape[0] != R or not np.all(np.isfinite(self.rates)) or np.any(self.rates < 0):
            raise ValueError('stochastic: one finite rate >= 0 per reaction')
        row = {s: i for i, s in enumerate(self.rows)}
        self.initial = np.zeros(self.n_rows, dtype=np.int32)
        for sp, value in (initial or {}).items():
            if sp not in row:
                raise ValueError('stochastic: initial names the unknown species %r' % (sp,))
            v = _whole(value, 'stochastic: initial count of %r' % (sp,))
            if not 0 <= v <= 2 ** 31 - 1:
                raise ValueError('stochastic: initial count of %r must lie in 0..2**31 - 1' % (sp,))
            self.initial[row[sp]] = v
        self.seed = int(seed)
        self.max_events = _whole(max_events, 'stochastic: max_events')
        if not 1 <= self.max_events <= 2 ** 31 - 1:
            raise ValueError('stochastic: max_events must lie in 1..2**31 - 1')
        # the packed arrays (vk_ssa_net): reactant CSR and full-stoichiometry CSR, species ascending
        rp, rs, ro, sp_, ss, sd = [0], [], [], [0], [], []
        for r in range(R):
            for s in range(S):
                v = int(self.matrix[r, s])
                if v < 0:
                    rs.append(s)
                    ro.append(-v)
                if v != 0:
                    ss.append(s)
                    sd.append(v)
            rp.append(len(rs))
            sp_.append(len(ss))
        i32 = lambda a: np.asarray(a, dtype=np.int32)
        self.react_ptr, self.react_species, self.react_order = i32(rp), i32(rs), i32(ro)
        self.stoich_ptr, self.stoich_species, self.stoich_delta = i32(sp_), i32(ss), i32(sd)
        self.max_order = int(max(ro)) if ro else 0
        # inv[i] = 1.0 / (i + 1) in FP64: the choose() of the kernel multiplies by it
        self.inv = 1.0 / np.arange(1, MAX_ORDER + 1, dtype=np.float64)

    @property
    def n_species(self):
        return len(self.species)

    @property
    def n_reactions(self):
        return len(self.reactions)

    @property
    def rows(self):
        """Every row of the count table: the species, then the passive rows."""
        return self.species + self.passive

    @property
    def n_rows(self):
        return len(self.species) + len(self.passive)

    def index(self, species: str) -> int:
        """The row of a species or of a passive row."""
        rows = self.rows
        if species not in rows:
            raise ValueError('stochastic: no species %r (species: %s)' % (species, rows))
        return rows.index(species)

    def set_runs(self):
        """The maximal runs [lo, hi) of consecutive table rows whose divider is ``'set'``."""
        runs = []
        for r, name in enumerate(self.rows):
            if self.dividers.get(name) == 'set':
                if runs and runs[-1][1] == r:
                    runs[-1][1] = r + 1
                else:
                    runs.append([r, r + 1])
        return [tuple(run) for run in runs]

    def initial_counts(self, n: int, ld: int) -> np.ndarray:
        out = np.zeros((self.n_rows, ld), dtype=np.int32)
        out[:, :n] = self.initial[:, None]
        return out


_PACKED = ('react_ptr', 'react_species', 'react_order', 'stoich_ptr', 'stoich_species', 'stoich_delta', 'rates', 'inv')


class StochasticEngine:
    """A :class:`StochasticModel` resident on one GPU.  The engine holds the packed network
    as torch tensors; the library owns none of it."""

    def __init__(self, model: StochasticModel, device=None):
        import torch
        native.load()
        if not isinstance(model, StochasticModel):
            raise ValueError('StochasticEngine: a StochasticModel')
        self.model = model
        self.device = native.resolve_device(device)
        self._dev = {}
        for k in _PACKED:
            a = np.ascontiguousarray(getattr(model, k))
            if a.size == 0:
                a = np.zeros(1, dtype=a.dtype)           # a network without reactants: no null pointers
            self._dev[k] = torch.from_numpy(a).to(self.device)
        # the step word of the next launch: on the device, advanced by each launch, so graphs replay it
        self.step_counter = torch.zeros(1, dtype=torch.int64, device=self.device)

    def net(self) -> native.VkSsaNet:
        m, d = self.model, native.VkSsaNet()
        d.n_species, d.n_reactions, d.max_order, d.n_inv = m.n_species, m.n_reactions, m.max_order, len(m.inv)
        for k, v in self._dev.items():
            setattr(d, k, v.data_ptr())
        return d

    def _check_counts(self, counts, n, what):
        import torch
        S = self.model.n_rows                    # the launches stage and read rows < n_species only
        if (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[0] != S or
                not counts.is_contiguous()):
            raise ValueError('%s: counts must be a contiguous int32 [%d, ld] device tensor' % (what, S))
        ld = counts.shape[1]
        n = ld if n is None else int(n)
        if not 0 <= n <= ld:
            raise ValueError('%s: 0 <= n <= ld' % what)
        return n, ld

    def step(self, duration, counts, keys, n=None, events=None, status=None, step_counter=None, max_events=None,
             seed=None):
        """One vk_ssa_step launch on the current stream for agents [0, n) of ``counts``
        [n_rows, ld] (int32; passive rows are not touched) with ``keys`` [ld] (int64, each in [0, 2**31)).  ``step_counter`` (one
        device int64, default the engine's own) is read and advanced.  Returns (events
        [ld] int32, status [ld] int32: VK_SSA_* bits OR-ed in)."""
        import torch
        n, ld = self._check_counts(counts, n, 'StochasticEngine.step')
        if not torch.is_tensor(keys) or keys.dtype != torch.int64 or keys.dim() != 1 or keys.shape[0] < n:
            raise ValueError('StochasticEngine.step: keys must be an int64 device tensor over the agents')
        if events is None:
            events = torch.zeros(ld, dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.zeros(ld, dtype=torch.int32, device=self.device)
        counter = self.step_counter if step_counter is None else step_counter
        m = self.model
        d = self.net()
        native.check(native._lib.vk_ssa_step(
            ctypes.byref(d), n, ld, float(duration), native.ptr(counts), native.ptr(keys),
            (m.seed if seed is None else int(seed)) & (2 ** 64 - 1), native.ptr(counter),
            int(m.max_events if max_events is None else max_events), native.ptr(events), native.ptr(status),
            native.stream_handle()), 'vk_ssa_step')
        return events, status

    def propensities(self, counts, n=None, out=None):
        """a_r of every agent as the step evaluates it: float64 [R, ld]."""
        import torch
        n, ld = self._check_counts(counts, n, 'StochasticEngine.propensities')
        if out is None:
            out = torch.zeros((self.model.n_reactions, ld), dtype=torch.float64, device=self.device)
        d = self.net()
        native.check(native._lib.vk_ssa_propensities(
            ctypes.byref(d), n, ld, native.ptr(counts), native.ptr(out), native.stream_handle()),
            'vk_ssa_propensities')
        return out


def divide_counts(n_out, n_keep, n_src, src, kind, counts_src, key_src, counts_dst, key_dst, seed, step, key_base):
    """vk_divide_counts on the current stream (see include/vk_kinetics.h)."""
    native.check(native._lib.vk_divide_counts(
        int(n_out), int(n_keep), int(n_src), native.ptr(src), native.ptr(kind), native.ptr(counts_src),
        counts_src.shape[-1], native.ptr(key_src), native.ptr(counts_dst), counts_dst.shape[-1], native.ptr(key_dst),
        counts_src.shape[0], int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), int(key_base),
        native.stream_handle()), 'vk_divide_counts')


def passive_seed(seed, chunk):
    """The seed of the division launch of passive rows [S + 64 chunk, S + 64 chunk + 64)."""
    return ((int(seed) ^ native.VK_SSA_PASSIVE_DOMAIN) + int(chunk)) & (2 ** 64 - 1)


def divide_agent_counts(col, plan, old, new, ld):
    """The colony's divider of ``ssa`` / ``ssa_key`` (population.DIVIDERS): divide_split on every
    row, a coin per (mother, row) keyed by the mother's key; daughters get the keys from
    the colony's base on.  The rows the model declares ``'set'`` are then copied from the
    mother.  Once installed: the base moves past them, and the daughters' motors read their
    own share of the flagella complex."""
    base = col._ssa_key_base
    if base + plan.n_daughters - 1 > 2 ** 31 - 1:
        raise OverflowError('a stochastic key would pass 2**31 - 1 (the kernel puts it into a 32-bit counter word)')
    S, rows = col.stochastic.n_species, col.stochastic.n_rows
    divide_counts(plan.n_out, plan.n_keep, plan.n_src, plan.src, plan.kind, old['ssa'][:S], old['ssa_key'],
                  new['ssa'][:S], new['ssa_key'], col.stochastic.seed, col.step_index, base)
    # the passive rows, in chunks of at most 64 under seeds of their own; each launch writes the
    # daughters' keys again, with equal values (the same key_base)
    for chunk, lo in enumerate(range(S, rows, MAX_SPECIES)):
        hi = min(lo + MAX_SPECIES, rows)
        divide_counts(plan.n_out, plan.n_keep, plan.n_src, plan.src, plan.kind, old['ssa'][lo:hi], old['ssa_key'],
                      new['ssa'][lo:hi], new['ssa_key'], passive_seed(col.stochastic.seed, chunk), col.step_index, base)
    # the 'set' rows: over what the split wrote, each run of them copied from the mother (no coin
    # of any other row moves: the coins go by mother and row index within their launch)
    for lo, hi in col.stochastic.set_runs():
        native.check(native._lib.vk_divide_gather(
            *plan.ptrs, native.ptr(old['ssa'][lo:hi]), old['ssa'].shape[-1], native.ptr(new['ssa'][lo:hi]),
            new['ssa'].shape[-1], hi - lo, 4, native.VK_DIVIDE_SET, native.stream_handle()), 'vk_divide_gather(ssa set)')

    def installed(col):
        col._ssa_key_base = base + plan.n_daughters
        if col._ssa_complex() is not None:
            col._ssa_flagella()
    return installed


def flagella_target(n, counts_row, target, flags):
    """vk_ssa_flagella_target on the current stream: ``target[:n] = clamp(counts_row[:n], 0, 32)``;
    ``counts_row`` / ``target``: int32 device rows (views), ``flags``: one device int32."""
    native.check(native._lib.vk_ssa_flagella_target(
        int(n), native.ptr(counts_row), native.ptr(target), native.ptr(flags), native.stream_handle()),
        'vk_ssa_flagella_target')
