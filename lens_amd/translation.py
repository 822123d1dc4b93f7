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
from lens_amd.polymerize import Polymerase, PolymeraseEngine, PolymeraseModel, sub_intervals    # noqa: F401
from lens_amd.polymerize import describe_status as _describe_status, status_names
from lens_amd.stochastic import StochasticModel, _whole

MAX_SLOTS, MAX_TEMPLATES, MAX_MONOMERS = native.VK_TL_MAX_SLOTS, native.VK_TL_MAX_TEMPLATES, native.VK_TL_MAX_MONOMERS
UNBOUND_RIBOSOME_KEY = 'Ribosome'
RELEASE = {'reference': native.VK_TL_RELEASE_REFERENCE, 'template': native.VK_TL_RELEASE_TEMPLATE}
STATUS_NAMES = status_names('ribosome')


def describe_status(bits: int) -> str:
    return _describe_status(bits, 'ribosome')


def pack(template: int, position: int, occluding) -> int:
    """One ribosome as the list holds it: (position << 7) | (template << 1) | occluding."""
    return (int(position) << 7) | (int(template) << 1) | (1 if occluding else 0)


def unpack(word: int):
    """(template, position, occluding) of a packed ribosome."""
    word = int(word) & 0xFFFFFFFF
    return (word >> 1) & 63, word >> 7, bool(word & 1)


class TranslationModel(PolymeraseModel):
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

    process = 'translation'

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
        self.max_ribosomes = self._check_parameters(elongation_rate, polymerase_occlusion, max_ribosomes,
                                                    'max_ribosomes', MAX_SLOTS, seed, max_events)

    @property
    def n_templates(self):
        return len(self.transcript_order)

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


class TranslationEngine(PolymeraseEngine):
    """A :class:`TranslationModel` bound to a :class:`StochasticModel`'s table, resident on one
    GPU.  The engine holds the packed tables and the sub-interval plans as torch tensors; the
    library owns none of it."""

    def __init__(self, model: TranslationModel, stochastic_model: StochasticModel, device=None):
        if not isinstance(model, TranslationModel):
            raise ValueError('TranslationEngine: a TranslationModel')
        operon, prod, self.ribosome_species = model.bind(stochastic_model)      # before anything is built
        super().__init__(model, stochastic_model, device)
        put = self.put
        self._dev = {'operon_species': put(operon), 'prod_species': put(prod), 'seq_ptr': put(model.seq_ptr),
                     'prod_ptr': put(model.prod_ptr), 'seq': put(model.seq), 'affinity': put(model.affinity)}

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
        m = self.model
        ld, n, events, status = self._check_step_tensors(slots, m.max_ribosomes, length, molecules, counts, keys, n,
                                                         events, status)
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


POLYMERASE = Polymerase(model='translation', slots='ribosome_slots', count='ribosome_count', molecules='tl_molecules',
                        max_slots='max_ribosomes', check='check_ribosomes', unpack=unpack, divide=divide_ribosomes,
                        domain=native.VK_TL_DIVIDE_DOMAIN)
