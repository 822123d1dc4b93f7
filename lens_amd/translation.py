"""Stochastic translation per agent: ribosomes bind transcripts and elongate proteins one
residue at a time from limited amino-acid pools.

The reference's ``Translation`` (vivarium/processes/translation.py:423-579) keeps a dict of
ribosomes per agent and steps it with ``polymerize_step`` (vivarium/library/polymerize.py:205-259).
Here every agent of a colony holds a bounded, ordered ribosome list (int32 ``[max_ribosomes][ld]``,
one packed word per ribosome, and its length) and advances by one launch per timestep
(vk_translation_step): one agent per lane.  Transcripts, proteins and the free ``Ribosome`` are
species of a :class:`~lens_amd.stochastic.StochasticModel`'s int table; the monomers, ATP and ADP
are an int table of their own.

Elongation is the reference's, operation for operation.  Initiation is the Gillespie direct
method in vk_ssa_step's arithmetic and Philox draws, NOT arrow's: trajectories agree with the
reference in distribution only.  The step is stated above ``vk_translation_step`` in
include/vk_kinetics.h and restated as Python loops by tests/translation_ref.py; DESIGN.md §20 says
what is and what is not the reference.
"""

from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np

from lens_amd import native
from lens_amd.stochastic import StochasticModel, _whole, divide_counts

MAX_SLOTS, MAX_TEMPLATES, MAX_MONOMERS = native.VK_TL_MAX_SLOTS, native.VK_TL_MAX_TEMPLATES, native.VK_TL_MAX_MONOMERS
UNBOUND_RIBOSOME_KEY = 'Ribosome'
RELEASE = {'reference': native.VK_TL_RELEASE_REFERENCE, 'template': native.VK_TL_RELEASE_TEMPLATE}
STATUS_NAMES = ((native.VK_TL_SLOTS_FULL, 'ribosome list full'), (native.VK_TL_BAD_KEY, 'key outside [0, 2**31)'),
                (native.VK_TL_NONFINITE, 'propensity not finite'),
                (native.VK_TL_OVERFLOW, 'a count would pass 2**31 - 1'), (native.VK_TL_MAX_EVENTS, 'max_events reached'))


def describe_status(bits: int) -> str:
    return ', '.join(text for bit, text in STATUS_NAMES if bits & bit) or 'ok'


def pack(template: int, position: int, occluding) -> int:
    """One ribosome as the list holds it: (position << 7) | (template << 1) | occluding."""
    return (int(position) << 7) | (int(template) << 1) | (1 if occluding else 0)


def unpack(word: int):
    """(template, position, occluding) of a packed ribosome."""
    word = int(word) & 0xFFFFFFFF
    return (word >> 1) & 63, word >> 7, bool(word & 1)


def sub_intervals(dt, rate):
    """The reference's float loop (translation.py:478-499, 533), run once: a list of
    (interval, elongates).  A trailing partial sub-interval elongates nothing."""
    out, time = [], 0
    while time < dt:
        distance = 1 / rate
        interval = min(distance, dt - time)
        out.append((interval, interval == distance))
        time += interval
    return out


class TranslationModel:
    """A translation process in the reference's config shapes.

    ``sequences``: ``{(operon, product): 'AWDPT...'}``; ``templates``: ``{(operon, product):
    {'id', 'position', 'direction', 'sites', 'terminators': [{'position', 'strength',
    'products'}]}}`` (``generate_template``); ``transcript_affinities``: ``{(operon, product):
    affinity}``, whose key order is the template order; ``symbol_to_monomer``: ``{symbol:
    monomer id}``; ``molecules``: the monomer ids in row order (ATP and ADP follow them).
    ``release``: which transcript an unoccluding ribosome releases, ``'reference'`` (always
    template 0, as the reference does) or ``'template'`` (her own).  ``transcript_species``:
    ``{operon: species}``, the name an operon's transcript has in the stochastic table where
    it is not the operon's own (the reference keeps transcripts and proteins in two stores, so
    an operon and its first product may share a name; one table needs two)."""

    def __init__(self, sequences, templates, transcript_affinities, elongation_rate, polymerase_occlusion,
                 symbol_to_monomer: Dict[str, str], molecules: Sequence[str], max_ribosomes: int = MAX_SLOTS,
                 release: str = 'reference', seed: int = 0, max_events: int = 100000,
                 transcript_species: Optional[Dict[str, str]] = None):
        if release not in RELEASE:
            raise ValueError('translation: release must be reference or template (got %r)' % (release,))
        self.release = release
        keys = [tuple(k) for k in transcript_affinities.keys()]
        if not keys or any(len(k) != 2 for k in keys):
            raise ValueError('translation: transcript_affinities must be {(operon, product): affinity}')
        if not 1 <= len(keys) <= MAX_TEMPLATES:
            raise ValueError('translation: 1..%d templates (got %d)' % (MAX_TEMPLATES, len(keys)))
        self.transcript_order = keys
        # gene_counts follows gather_genes' order (operons by first appearance, their products in
        # order); it equals transcript_order only if the keys are grouped by operon
        operons = {}
        for operon, product in keys:
            operons.setdefault(operon, []).append(product)
        if [(o, p) for o, ps in operons.items() for p in ps] != keys:
            raise ValueError('translation: transcript_affinities keys must be grouped by operon (the reference\'s '
                             'gene_counts order would differ from transcript_order)')
        self.operons = list(operons.keys())
        unknown = set(transcript_species or {}) - set(self.operons)
        if unknown:
            raise ValueError('translation: transcript_species names the unknown operons %s' % sorted(unknown))
        self.transcript_species = {o: str((transcript_species or {}).get(o, o)) for o in self.operons}
        self.affinity = np.asarray([float(transcript_affinities[k]) for k in transcript_affinities.keys()],
                                   dtype=np.float64)
        if not np.all(np.isfinite(self.affinity)) or np.any(self.affinity < 0):
            raise ValueError('translation: one finite affinity >= 0 per transcript')
        self.monomer_ids = [str(m) for m in molecules]
        if len(set(self.monomer_ids)) != len(self.monomer_ids) or {'ATP', 'ADP'} & set(self.monomer_ids):
            raise ValueError('translation: molecules must be distinct monomer ids (ATP and ADP follow them)')
        if not 1 <= len(self.monomer_ids) <= MAX_MONOMERS:
            raise ValueError('translation: 1..%d monomers (got %d)' % (MAX_MONOMERS, len(self.monomer_ids)))
        self.molecule_ids = self.monomer_ids + ['ATP', 'ADP']
        row = {m: i for i, m in enumerate(self.monomer_ids)}
        sequences = {tuple(k): v for k, v in sequences.items()}
        templates = {tuple(k): v for k, v in templates.items()}
        seq_ptr, seq, prod_ptr, self.products, self.template_products = [0], [], [0], [], []
        for key in keys:
            if key not in sequences or key not in templates:
                raise ValueError('translation: transcript %r has no sequence or no template' % (key,))
            tpl, sequence = templates[key], sequences[key]
            if tpl.get('sites'):
                raise ValueError('translation: template %r has sites (not supported)' % (key,))
            if tpl.get('direction', 1) != 1:
                raise ValueError('translation: template %r has direction %r (only 1 is supported)' % (
                    key, tpl.get('direction')))
            terminators = tpl.get('terminators', [])
            if len(terminators) != 1:
                raise ValueError('translation: template %r has %d terminators (exactly one is supported)' % (
                    key, len(terminators)))
            if not 1 <= len(sequence) <= native.VK_TL_MAX_POSITION:
                raise ValueError('translation: the sequence of %r must hold 1..2**24 - 1 residues' % (key,))
            if terminators[0].get('position', 0) - tpl.get('position', 0) != len(sequence):
                raise ValueError('translation: the terminator of %r is not at len(sequence) = %d' % (key, len(sequence)))
            for symbol in sequence:
                if symbol not in symbol_to_monomer or symbol_to_monomer[symbol] not in row:
                    raise ValueError('translation: symbol %r of %r has no monomer among the molecules' % (symbol, key))
                seq.append(row[symbol_to_monomer[symbol]])
            seq_ptr.append(len(seq))
            products = [str(p) for p in terminators[0].get('products', [])]
            if len(set(products)) != len(products):
                raise ValueError('translation: the terminator of %r names a product twice' % (key,))
            self.template_products.append(products)
            self.products.extend(p for p in products if p not in self.products)
            prod_ptr.append(prod_ptr[-1] + len(products))
        clash = set(self.products) & (set(self.transcript_species.values()) | {UNBOUND_RIBOSOME_KEY})
        if clash:
            raise ValueError('translation: %s cannot be both a product and a transcript or the free ribosome' % (
                sorted(clash),))
        self.seq_ptr, self.prod_ptr = np.asarray(seq_ptr, dtype=np.int32), np.asarray(prod_ptr, dtype=np.int32)
        self.seq = np.asarray(seq, dtype=np.uint8)
        self.elongation_rate = elongation_rate
        if not (float(elongation_rate) > 0 and np.isfinite(float(elongation_rate))):
            raise ValueError('translation: elongation_rate must be finite and > 0')
        self.polymerase_occlusion = _whole(polymerase_occlusion, 'translation: polymerase_occlusion')
        if not -2 ** 31 <= self.polymerase_occlusion <= 2 ** 31 - 1:
            raise ValueError('translation: polymerase_occlusion does not fit int32')
        self.max_ribosomes = _whole(max_ribosomes, 'translation: max_ribosomes')
        if not 1 <= self.max_ribosomes <= MAX_SLOTS:
            raise ValueError('translation: max_ribosomes must lie in 1..%d' % MAX_SLOTS)
        self.seed = int(seed)
        self.max_events = _whole(max_events, 'translation: max_events')
        if not 1 <= self.max_events <= 2 ** 31 - 1:
            raise ValueError('translation: max_events must lie in 1..2**31 - 1')

    @property
    def n_templates(self):
        return len(self.transcript_order)

    @property
    def n_monomers(self):
        return len(self.monomer_ids)

    def length(self, template: int) -> int:
        return int(self.seq_ptr[template + 1] - self.seq_ptr[template])

    def species(self):
        """Every species the stochastic table must hold: the operons' transcripts, the
        products and the free ribosome."""
        return [self.transcript_species[o] for o in self.operons] + self.products + [UNBOUND_RIBOSOME_KEY]

    def bind(self, stochastic: StochasticModel):
        """(operon_species [T], prod_species, ribosome_species): rows of the stochastic table.
        ValueError if a species is missing from it."""
        if not isinstance(stochastic, StochasticModel):
            raise ValueError('translation needs a StochasticModel (stochastic=) that holds its transcripts, proteins '
                             'and %r' % UNBOUND_RIBOSOME_KEY)
        missing = [s for s in self.species() if s not in stochastic.rows]
        if missing:
            raise ValueError('translation: the StochasticModel lacks the species %s' % missing)
        operon = np.asarray([stochastic.index(self.transcript_species[o]) for o, _ in self.transcript_order],
                            dtype=np.int32)
        prod = np.asarray([stochastic.index(p) for ps in self.template_products for p in ps], dtype=np.int32)
        return operon, prod, stochastic.index(UNBOUND_RIBOSOME_KEY)

    def plan(self, dt):
        return sub_intervals(dt, self.elongation_rate)

    def check_ribosomes(self, ribosomes):
        """Packed words of one agent's ``[(template, position, occluding), ...]``; ValueError
        if the list does not fit or a ribosome stands outside its template."""
        if len(ribosomes) > self.max_ribosomes:
            raise ValueError('translation: %d ribosomes exceed max_ribosomes = %d' % (len(ribosomes), self.max_ribosomes))
        words = []
        for t, p, occluding in ribosomes:
            t, p = _whole(t, 'translation: template index'), _whole(p, 'translation: position')
            if not 0 <= t < self.n_templates or not 0 <= p < self.length(t):
                raise ValueError('translation: ribosome (%d, %d) stands outside its template' % (t, p))
            words.append(pack(t, p, occluding))
        return np.asarray(words, dtype=np.uint32).view(np.int32)

    def initial_molecules(self, n: int, ld: int, counts=None) -> np.ndarray:
        out = np.zeros((len(self.molecule_ids), ld), dtype=np.int32)
        for name, value in (counts or {}).items():
            if name not in self.molecule_ids:
                raise ValueError('translation: no molecule %r (molecules: %s)' % (name, self.molecule_ids))
            out[self.molecule_ids.index(name), :n] = np.asarray(value, dtype=np.int64)
        return out


class TranslationEngine:
    """A :class:`TranslationModel` bound to a :class:`StochasticModel`'s table, resident on one
    GPU.  The engine holds the packed tables and the sub-interval plans as torch tensors; the
    library owns none of it."""

    def __init__(self, model: TranslationModel, stochastic_model: StochasticModel, device=None):
        import torch
        if not isinstance(model, TranslationModel):
            raise ValueError('TranslationEngine: a TranslationModel')
        operon, prod, self.ribosome_species = model.bind(stochastic_model)      # before anything is built
        native.load()
        self.model, self.stochastic_model = model, stochastic_model
        self.device = native.resolve_device(device)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros(1, dtype=a.dtype))).to(self.device)
        self._dev = {'operon_species': put(operon), 'prod_species': put(prod), 'seq_ptr': put(model.seq_ptr),
                     'prod_ptr': put(model.prod_ptr), 'seq': put(model.seq), 'affinity': put(model.affinity)}
        self._plans = {}
        self.step_counter = torch.zeros(1, dtype=torch.int64, device=self.device)

    def plan(self, dt):
        """The sub-interval plan of a step of ``dt`` on the device: (interval float64 [K],
        elongate int32 [K], K).  Kept per ``dt``, so a captured graph's plan stays alive."""
        import torch
        dt = float(dt)
        if not (dt >= 0.0 and np.isfinite(dt)):
            raise ValueError('TranslationEngine: dt must be finite and >= 0')
        if dt not in self._plans:
            p = self.model.plan(dt)
            iv = np.asarray([x for x, _ in p] or [0.0], dtype=np.float64)
            el = np.asarray([int(y) for _, y in p] or [0], dtype=np.int32)
            self._plans[dt] = (torch.from_numpy(iv).to(self.device), torch.from_numpy(el).to(self.device), len(p))
        return self._plans[dt]

    def table(self, dt) -> native.VkTlModel:
        m, d = self.model, native.VkTlModel()
        interval, elongate, d.n_plan = self.plan(dt)
        # n_species bounds the rows the kernel may touch: every row of the table, passive ones included
        d.n_templates, d.n_monomers, d.n_species = m.n_templates, m.n_monomers, self.stochastic_model.n_rows
        d.max_slots, d.occlusion, d.release = m.max_ribosomes, m.polymerase_occlusion, RELEASE[m.release]
        d.ribosome_species = self.ribosome_species
        for k, v in self._dev.items():
            setattr(d, k, v.data_ptr())
        d.interval, d.elongate = interval.data_ptr(), elongate.data_ptr()
        return d

    def step(self, dt, slots, length, molecules, counts, keys, n=None, events=None, status=None, step_counter=None,
             advance=True, max_events=None, seed=None):
        """One vk_translation_step launch on the current stream for agents [0, n): ``slots``
        [max_ribosomes, ld] and ``length`` [ld] (int32), ``molecules`` [monomers + 2, ld],
        ``counts`` [n_rows, ld] (the stochastic table, edited in place), ``keys`` [ld] (int64).
        ``step_counter`` (one device int64, default the engine's own) is read, and advanced
        if ``advance``.  Returns (events [ld] int32, status [ld] int32: VK_TL_* bits OR-ed in)."""
        import torch
        m = self.model
        ld = counts.shape[-1] if torch.is_tensor(counts) and counts.dim() == 2 else -1
        for t, rows, what in ((slots, m.max_ribosomes, 'slots'), (molecules, m.n_monomers + 2, 'molecules'),
                              (counts, self.stochastic_model.n_rows, 'counts')):
            if (not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 2 or t.shape != (rows, ld) or
                    not t.is_contiguous()):
                raise ValueError('TranslationEngine.step: %s must be a contiguous int32 [%d, ld] device tensor' % (
                    what, rows))
        n = ld if n is None else int(n)
        if not 0 <= n <= ld:
            raise ValueError('TranslationEngine.step: 0 <= n <= ld')
        if not torch.is_tensor(length) or length.dtype != torch.int32 or length.dim() != 1 or length.shape[0] < n:
            raise ValueError('TranslationEngine.step: length must be an int32 device tensor over the agents')
        if not torch.is_tensor(keys) or keys.dtype != torch.int64 or keys.dim() != 1 or keys.shape[0] < n:
            raise ValueError('TranslationEngine.step: keys must be an int64 device tensor over the agents')
        if events is None:
            events = torch.zeros(ld, dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.zeros(ld, dtype=torch.int32, device=self.device)
        counter = self.step_counter if step_counter is None else step_counter
        d = self.table(dt)
        native.check(native._lib.vk_translation_step(
            ctypes.byref(d), n, ld, native.ptr(slots), native.ptr(length), native.ptr(molecules), native.ptr(counts),
            native.ptr(keys), (m.seed if seed is None else int(seed)) & (2 ** 64 - 1), native.ptr(counter),
            1 if advance else 0, int(m.max_events if max_events is None else max_events), native.ptr(events),
            native.ptr(status), native.stream_handle()), 'vk_translation_step')
        return events, status


def divide_ribosomes(n_out, n_src, src, kind, slots_src, length_src, key_src, slots_dst, length_dst, seed, step):
    """vk_divide_ribosomes on the current stream (see include/vk_kinetics.h)."""
    native.check(native._lib.vk_divide_ribosomes(
        int(n_out), int(n_src), native.ptr(src), native.ptr(kind), native.ptr(slots_src), native.ptr(length_src),
        slots_src.shape[-1], native.ptr(key_src), native.ptr(slots_dst), native.ptr(length_dst), slots_dst.shape[-1],
        slots_src.shape[0], int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), native.stream_handle()),
        'vk_divide_ribosomes')


def divide_agent_ribosomes(col, plan, old, new, ld):
    """The colony's divider of ``ribosome_slots`` / ``ribosome_count`` (population.DIVIDERS): the
    list entry by entry, a coin per (mother, entry) keyed by the mother's key (the old ``ssa_key``)."""
    divide_ribosomes(plan.n_out, plan.n_src, plan.src, plan.kind, old['ribosome_slots'], old['ribosome_count'],
                     old['ssa_key'], new['ribosome_slots'], new['ribosome_count'], col.translation.seed,
                     col.step_index)


def divide_agent_molecules(col, plan, old, new, ld):
    """The colony's divider of ``tl_molecules``: divide_split like the stochastic counts, by the
    mothers' keys under a domain of its own; the daughters' keys it would hand out are dropped."""
    import torch
    divide_counts(plan.n_out, plan.n_keep, plan.n_src, plan.src, plan.kind, old['tl_molecules'], old['ssa_key'],
                  new['tl_molecules'], torch.empty(ld, dtype=torch.int64, device=col.device),
                  col.translation.seed ^ native.VK_TL_DIVIDE_DOMAIN, col.step_index, col._ssa_key_base)
