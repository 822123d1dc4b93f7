"""Stochastic transcription per agent: RNA polymerases bind the chromosome's promoters, whose
affinity the transcription factors switch, and elongate transcripts one base at a time from
limited nucleotide pools.

The reference's ``Transcription`` (vivarium/processes/transcription.py:370-553) keeps a
``Chromosome`` (vivarium/states/chromosome.py) with a dict of RNAPs per agent and steps it with
``polymerize_step`` (vivarium/library/polymerize.py:205-259).  Here every agent of a colony holds
a bounded, ordered RNAP list (int32 ``[max_rnaps][ld]``, one packed word per RNAP, and its
length) and advances by one launch per timestep (vk_transcription_step): one agent per lane.
Transcripts, transcription factors and the free ``RNA Polymerase`` are species of a
:class:`~lens_amd.stochastic.StochasticModel`'s int table; the nucleotides, ATP and ADP are an
int table of their own.

The reference's, operation for operation: the sequences (``Chromosome.sequences``), the affinity
vector from the sites' states (``Template.binding_state``, first factor over its threshold in
dict order), elongation with stalls, the read-through rule of ``terminates_at``, unocclusion,
and the books with their ATP quirk (ATP's own monomer entry is overwritten by the hydrolysis
cost, so the stored ATP may go below zero while ``limit['ATP']`` never does).

THE ENGINE'S OWN, not the reference's: initiation is the Gillespie direct method in vk_ssa_step's
arithmetic and Philox draws, NOT arrow's; the read-through uniform is Philox, not Python's
``random.random()``; the factor levels are ``counts / mmol_to_counts`` at the start of the launch
(the reference reads what ``concentrations_deriver`` left); the process edits the int table in
place in front of translation and the network (the reference applies all updates to the step-start
state); the RNAP list divides by a coin per (mother, entry).  Trajectories agree with the
reference in distribution only.  The step is stated above ``vk_transcription_step`` in
include/vk_kinetics.h and restated as Python loops by tests/transcription_ref.py; DESIGN.md §21
says what is and what is not the reference.

Only the single childless root domain is supported (nothing in the reference's processes ever
calls ``initiate_replication``), so every promoter's copy number is 1; ``copy`` is kept as an
array so that replication domains can lift this later.
"""

from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence

import numpy as np

from lens_amd import native
from lens_amd.polymerize import Polymerase, PolymeraseEngine, PolymeraseModel, sub_intervals    # noqa: F401
from lens_amd.polymerize import describe_status as _describe_status, status_names
from lens_amd.stochastic import StochasticModel, _whole
from lens_amd.translation import divide_ribosomes

MAX_SLOTS, MAX_TEMPLATES, MAX_TERMINATORS = native.VK_TX_MAX_SLOTS, native.VK_TX_MAX_TEMPLATES, native.VK_TX_MAX_TERMINATORS
MAX_SITES, MAX_FACTORS, MAX_MONOMERS = native.VK_TX_MAX_SITES, native.VK_TX_MAX_FACTORS, native.VK_TX_MAX_MONOMERS
MAX_AFFINITIES = native.VK_TX_MAX_AFFINITIES
UNBOUND_RNAP_KEY = 'RNA Polymerase'
NUCLEOTIDES = {'A': 'ATP', 'G': 'GTP', 'U': 'UTP', 'C': 'CTP'}
ROOT_DOMAINS = {0: {'id': 0, 'lead': 0, 'lag': 0, 'children': []}}
SEQUENCE = {'auto': native.VK_TX_SEQUENCE_AUTO, 'global': native.VK_TX_SEQUENCE_GLOBAL, 'lds': native.VK_TX_SEQUENCE_LDS}
STATUS_NAMES = status_names('RNAP')


def describe_status(bits: int) -> str:
    return _describe_status(bits, 'RNAP')


def pack(template: int, terminator: int, position: int, occluding) -> int:
    """One RNAP as the list holds it: (position << 9) | (terminator << 7) | (template << 1) | occluding."""
    return (int(position) << 9) | (int(terminator) << 7) | (int(template) << 1) | (1 if occluding else 0)


def unpack(word: int):
    """(template, terminator, position, occluding) of a packed RNAP."""
    word = int(word) & 0xFFFFFFFF
    return (word >> 1) & 63, (word >> 7) & 3, word >> 9, bool(word & 1)


def rna_bases(sequence: str) -> str:
    """chromosome.py:24-30: A -> U, T -> A, C -> G, G -> C."""
    return sequence.translate(str.maketrans('ATCG', 'UAGC'))


def sequence_monomers(sequence: str, begin: int, end: int) -> str:
    """chromosome.py:32-37: the slice a promoter reads, backwards for direction -1."""
    return sequence[begin:end] if begin < end else sequence[begin:end:-1]


def _number(x, what):
    try:
        x = float(x)
    except (TypeError, ValueError):
        raise ValueError('transcription: %s must be a number (got %r)' % (what, x))
    if not math.isfinite(x) or x < 0:
        raise ValueError('transcription: %s must be finite and >= 0 (got %r)' % (what, x))
    return x


class TranscriptionModel(PolymeraseModel):
    """A transcription process in the reference's config shapes.

    ``sequence``: the chromosome's DNA; ``templates``: ``{promoter id: {'id', 'position',
    'direction', 'sites': [{'position', 'length', 'thresholds': {factor: mM}}], 'terminators':
    [{'position', 'strength', 'products': [operon, ...]}]}}``, whose key order is the promoter
    order; thresholds are plain magnitudes in mM.  ``genes``: ``{operon: [gene, ...]}`` (kept; the
    step does not read it).  ``promoter_affinities``: ``{(promoter id, state of site 0, ...):
    affinity}``, a state being a factor name or ``None``; missing keys mean 0.0.
    ``transcription_factors``: every factor a threshold may name.  ``monomer_ids``: the monomers in
    row order; the molecule rows are these, then ``ATP`` if it is no monomer, then ``ADP``.
    ``transcript_species``: ``{operon: species}``, the name a terminator's product has in the
    stochastic table where it is not the operon's own.  ``domains``: the chromosome's replication
    domains; anything but the single childless root is refused.  ``sequence_path``: where the kernel reads
    the templates' bases, ``'global'`` (the byte table in global memory), ``'lds'`` (2 bits per base
    staged in LDS whenever it fits) or ``'auto'`` (staged only where that costs no occupancy); the
    results are the same."""

    process = 'transcription'

    def __init__(self, sequence, templates, genes, promoter_affinities, transcription_factors, elongation_rate,
                 polymerase_occlusion, symbol_to_monomer: Optional[Dict[str, str]] = None,
                 monomer_ids: Optional[Sequence[str]] = None, max_rnaps: int = MAX_SLOTS, seed: int = 0,
                 max_events: int = 100000, transcript_species: Optional[Dict[str, str]] = None, domains=None,
                 sequence_path: str = 'auto'):
        if sequence_path not in SEQUENCE:
            raise ValueError('transcription: sequence_path must be auto, global or lds (got %r)' % (sequence_path,))
        self.sequence_path = sequence_path
        domains = ROOT_DOMAINS if domains is None else domains
        if len(domains) != 1 or any(d.get('children') for d in domains.values()):
            raise ValueError('transcription: only the single childless root domain is supported (replication domains '
                             'are not; got %d domains)' % len(domains))
        symbol_to_monomer = dict(NUCLEOTIDES if symbol_to_monomer is None else symbol_to_monomer)
        self.monomer_ids = [str(m) for m in (list(NUCLEOTIDES.values()) if monomer_ids is None else monomer_ids)]
        if len(set(self.monomer_ids)) != len(self.monomer_ids) or 'ADP' in self.monomer_ids:
            raise ValueError('transcription: monomer_ids must be distinct and not ADP')
        if not 1 <= len(self.monomer_ids) <= MAX_MONOMERS:
            raise ValueError('transcription: 1..%d monomers (got %d)' % (MAX_MONOMERS, len(self.monomer_ids)))
        self.molecule_ids = self.monomer_ids + ([] if 'ATP' in self.monomer_ids else ['ATP']) + ['ADP']
        self.atp_row, self.adp_row = self.molecule_ids.index('ATP'), len(self.molecule_ids) - 1
        row = {m: i for i, m in enumerate(self.monomer_ids)}
        self.sequence, self.genes = str(sequence), dict(genes or {})
        self.transcription_factors = [str(f) for f in transcription_factors]
        self.promoter_order = [k for k in templates.keys()]
        P = len(self.promoter_order)
        if not 1 <= P <= MAX_TEMPLATES:
            raise ValueError('transcription: 1..%d promoters (got %d)' % (MAX_TEMPLATES, P))
        self.transcript_species = {str(k): str(v) for k, v in (transcript_species or {}).items()}
        self.sequences, self.term_pos_rel, self.site_factors, self.site_thresholds = [], [], [], []
        self.terminator_products = []            # per promoter, per terminator: the species names
        self.terminator_operons = []             # and the products' own names (the reference's operons)
        n_term = np.zeros(P, dtype=np.int32)
        term_pos = np.zeros(MAX_TERMINATORS * P, dtype=np.int32)
        term_strength, term_from = np.zeros(MAX_TERMINATORS * P), np.zeros(MAX_TERMINATORS * P)
        seq_ptr, seq = [0], []
        operons = []
        for p, key in enumerate(self.promoter_order):
            tpl = templates[key]
            if tpl.get('id', key) != key:
                raise ValueError('transcription: promoter %r carries the id %r' % (key, tpl.get('id')))
            direction, position = tpl.get('direction', 1), _whole(tpl.get('position', 0), 'transcription: position')
            if direction not in (1, -1):
                raise ValueError('transcription: promoter %r has direction %r (1 or -1)' % (key, direction))
            terminators = list(tpl.get('terminators', []))
            if not 1 <= len(terminators) <= MAX_TERMINATORS:
                raise ValueError('transcription: promoter %r has %d terminators (1..%d)' % (
                    key, len(terminators), MAX_TERMINATORS))
            # relative positions (chromosome.py:100): (terminator - promoter) * direction
            rel = [(_whole(t.get('position', 0), 'transcription: terminator position') - position) * direction
                   for t in terminators]
            if rel[0] < 1 or any(b <= a for a, b in zip(rel, rel[1:])):
                raise ValueError('transcription: the terminators of %r must stand at strictly increasing relative '
                                 'positions >= 1 (got %s)' % (key, rel))
            if rel[-1] > native.VK_TX_MAX_POSITION:
                raise ValueError('transcription: promoter %r is longer than 2**22 - 1 bases' % (key,))
            # Chromosome.sequences (chromosome.py:248-254)
            rna = rna_bases(sequence_monomers(self.sequence, position, terminators[-1]['position']))
            if len(rna) != rel[-1]:
                raise ValueError('transcription: the sequence gives promoter %r %d bases, its last terminator stands '
                                 'at %d' % (key, len(rna), rel[-1]))
            for symbol in rna:
                if symbol not in symbol_to_monomer or symbol_to_monomer[symbol] not in row:
                    raise ValueError('transcription: symbol %r of %r has no monomer among monomer_ids' % (symbol, key))
                seq.append(row[symbol_to_monomer[symbol]])
            seq_ptr.append(len(seq))
            strengths = [_number(t.get('strength', 0), 'the strength of a terminator of %r' % (key,))
                         for t in terminators]
            n_term[p] = len(terminators)
            products = []
            for i, t in enumerate(terminators):
                # Template.strength_from (polymerize.py:140-144), in its order of summation
                total = 0
                for index in range(i, len(terminators)):
                    total += strengths[index]
                if i + 1 < len(terminators) and not total > 0:
                    raise ValueError('transcription: the strengths of %r from terminator %d on sum to 0, and a draw '
                                     'would be needed there' % (key, i))
                term_pos[MAX_TERMINATORS * p + i], term_strength[MAX_TERMINATORS * p + i] = rel[i], strengths[i]
                term_from[MAX_TERMINATORS * p + i] = total
                names = [self.transcript_species.get(str(o), str(o)) for o in t.get('products', [])]
                if len(set(names)) != len(names):
                    raise ValueError('transcription: a terminator of %r names a product twice' % (key,))
                operons.extend(str(o) for o in t.get('products', []))
                products.append(names)
            self.terminator_products.append(products)
            self.terminator_operons.append([[str(o) for o in t.get('products', [])] for t in terminators])
            self.sequences.append(rna)
            self.term_pos_rel.append(rel)
            sites = list(tpl.get('sites', []))
            if len(sites) > MAX_SITES:
                raise ValueError('transcription: promoter %r has %d sites (at most %d)' % (key, len(sites), MAX_SITES))
            factors, values = [], []
            for site in sites:
                thresholds = site.get('thresholds', {})
                if len(thresholds) > MAX_FACTORS:
                    raise ValueError('transcription: a site of %r has %d thresholds (at most %d)' % (
                        key, len(thresholds), MAX_FACTORS))
                for f in thresholds:
                    if f not in self.transcription_factors:
                        raise ValueError('transcription: %r of a site of %r is no transcription factor' % (f, key))
                factors.append([str(f) for f in thresholds])
                values.append([_number(v, 'the threshold of %r at %r' % (f, key)) for f, v in thresholds.items()])
            self.site_factors.append(factors)
            self.site_thresholds.append(values)
        unknown = set(self.transcript_species) - set(operons)
        if unknown:
            raise ValueError('transcription: transcript_species names the unknown operons %s' % sorted(unknown))
        self.products = []
        for products in self.terminator_products:
            for names in products:
                self.products.extend(n for n in names if n not in self.products)
        clash = set(self.products) & (set(self.transcription_factors) | {UNBOUND_RNAP_KEY})
        if clash:
            raise ValueError('transcription: %s cannot be both a product and a factor or the free RNAP' % sorted(clash))
        # one dense table per promoter, mixed radix over the site states (0 = None, 1 + i = factor i)
        aff_ptr = [0]
        for factors in self.site_factors:
            size = 1
            for f in factors:
                size *= 1 + len(f)
            aff_ptr.append(aff_ptr[-1] + size)
        if aff_ptr[-1] > MAX_AFFINITIES:
            raise ValueError('transcription: the promoters\' site states take %d affinity entries (at most %d)' % (
                aff_ptr[-1], MAX_AFFINITIES))
        affinity = np.zeros(aff_ptr[-1], dtype=np.float64)
        for binding, value in promoter_affinities.items():
            binding = tuple(binding)
            if not binding or binding[0] not in self.promoter_order:
                raise ValueError('transcription: the affinity key %r names no promoter' % (binding,))
            p = self.promoter_order.index(binding[0])
            factors = self.site_factors[p]
            # binding_state (polymerize.py:133-138) is (id, state of every site): other lengths never match
            if len(binding) != 1 + len(factors):
                raise ValueError('transcription: the affinity key %r must hold one state per site of %r (%d)' % (
                    binding, binding[0], len(factors)))
            idx = 0
            for state, f in zip(binding[1:], factors):
                if state is not None and state not in f:
                    raise ValueError('transcription: the affinity key %r names %r, which its site cannot take' % (
                        binding, state))
                idx = idx * (1 + len(f)) + (0 if state is None else 1 + f.index(state))
            affinity[aff_ptr[p] + idx] = _number(value, 'the affinity of %r' % (binding,))
        self.affinity, self.aff_ptr = affinity, np.asarray(aff_ptr, dtype=np.int32)
        self.copy = np.ones(P, dtype=np.int32)           # the root domain alone: every promoter once
        self.n_term, self.term_pos, self.term_strength, self.term_from = n_term, term_pos, term_strength, term_from
        self.seq_ptr, self.seq = np.asarray(seq_ptr, dtype=np.int32), np.asarray(seq, dtype=np.uint8)
        if len(seq) > 2 ** 31 - 17:
            raise ValueError('transcription: the templates hold too many bases')
        words = np.zeros((len(seq) + 15) // 16 * 16, dtype=np.uint32)
        words[:len(seq)] = self.seq
        self.seq2 = (words.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1).astype(np.uint32)
        self.max_rnaps = self._check_parameters(elongation_rate, polymerase_occlusion, max_rnaps, 'max_rnaps',
                                                MAX_SLOTS, seed, max_events)

    @property
    def n_templates(self):
        return len(self.promoter_order)

    def factors_used(self):
        """The factors a threshold names, in order of first appearance."""
        out = []
        for factors in self.site_factors:
            for f in factors:
                out.extend(x for x in f if x not in out)
        return out

    def product_sequences(self):
        """Chromosome.product_sequences (chromosome.py:256-266): ``{product: RNA}``, each product of
        a terminator mapped to her promoter's RNA from the promoter up to that terminator; a later
        promoter (or terminator) that names the same product overwrites an earlier one.  The keys are
        the products' own names (the operons), not ``transcript_species``."""
        sequences = {}
        for rna, rel, operons in zip(self.sequences, self.term_pos_rel, self.terminator_operons):
            for position, products in zip(rel, operons):
                for product in products:
                    sequences[product] = rna[:position]
        return sequences

    def species(self):
        """Every species the stochastic table must hold: the products, the factors that a
        threshold names and the free RNAP."""
        return self.products + self.factors_used() + [UNBOUND_RNAP_KEY]

    def affinity_of(self, template: int, states) -> float:
        """The table entry of promoter ``template`` at her sites' states (factor names or None)."""
        idx = 0
        for state, f in zip(states, self.site_factors[template]):
            idx = idx * (1 + len(f)) + (0 if state is None else 1 + f.index(state))
        return float(self.affinity[self.aff_ptr[template] + idx])

    def binding_state(self, template: int, levels):
        """Template.binding_state / BindingSite.state_when (polymerize.py:87-97, 133-138): per site the
        first factor in its threshold order with level >= threshold, else None."""
        out = []
        for factors, values in zip(self.site_factors[template], self.site_thresholds[template]):
            state = None
            for f, threshold in zip(factors, values):
                if levels[f] >= threshold:
                    state = f
                    break
            out.append(state)
        return tuple(out)

    def bind(self, stochastic: StochasticModel):
        """(prod_ptr [4 P + 1], prod_species, thr_species, rnap_species): rows of the stochastic table.
        ValueError if a species is missing from it."""
        if not isinstance(stochastic, StochasticModel):
            raise ValueError('transcription needs a StochasticModel (stochastic=) that holds its transcripts, factors '
                             'and %r' % UNBOUND_RNAP_KEY)
        missing = [s for s in self.species() if s not in stochastic.rows]
        if missing:
            raise ValueError('transcription: the StochasticModel lacks the species %s' % missing)
        prod_ptr, prod = [0], []
        for products in self.terminator_products:
            for i in range(MAX_TERMINATORS):
                prod.extend(stochastic.index(n) for n in (products[i] if i < len(products) else []))
                prod_ptr.append(len(prod))
        thr = [stochastic.index(f) for factors in self.site_factors for site in factors for f in site]
        return (np.asarray(prod_ptr, dtype=np.int32), np.asarray(prod, dtype=np.int32), np.asarray(thr, dtype=np.int32),
                stochastic.index(UNBOUND_RNAP_KEY))

    def check_rnaps(self, rnaps):
        """Packed words of one agent's ``[(template, terminator, position, occluding), ...]``;
        ValueError if the list does not fit, an RNAP stands outside its template or has passed the
        terminator it names."""
        if len(rnaps) > self.max_rnaps:
            raise ValueError('transcription: %d RNAPs exceed max_rnaps = %d' % (len(rnaps), self.max_rnaps))
        words = []
        for t, i, p, occluding in rnaps:
            t, i, p = (_whole(t, 'transcription: template index'), _whole(i, 'transcription: terminator index'),
                       _whole(p, 'transcription: position'))
            if not 0 <= t < self.n_templates or not 0 <= i < self.n_term[t] or not 0 <= p < self.term_pos_rel[t][i] \
                    or (i and p < self.term_pos_rel[t][i - 1]):
                raise ValueError('transcription: RNAP (%d, %d, %d) stands outside its template or terminator' % (t, i, p))
            words.append(pack(t, i, p, occluding))
        return np.asarray(words, dtype=np.uint32).view(np.int32)


class TranscriptionEngine(PolymeraseEngine):
    """A :class:`TranscriptionModel` bound to a :class:`StochasticModel`'s table, resident on one
    GPU.  The engine holds the packed tables and the sub-interval plans as torch tensors; the
    library owns none of it."""

    def __init__(self, model: TranscriptionModel, stochastic_model: StochasticModel, device=None):
        if not isinstance(model, TranscriptionModel):
            raise ValueError('TranscriptionEngine: a TranscriptionModel')
        prod_ptr, prod, thr, self.rnap_species = model.bind(stochastic_model)      # before anything is built
        super().__init__(model, stochastic_model, device)
        put = self.put
        site_ptr, thr_ptr, thr_value = [0], [0], []
        for factors, values in zip(model.site_factors, model.site_thresholds):
            for v in values:
                thr_value.extend(v)
                thr_ptr.append(len(thr_value))
            site_ptr.append(len(thr_ptr) - 1)
        self._dev = {'copy': put(model.copy), 'n_term': put(model.n_term), 'term_pos': put(model.term_pos),
                     'prod_ptr': put(prod_ptr), 'prod_species': put(prod), 'seq_ptr': put(model.seq_ptr),
                     'site_ptr': put(np.asarray(site_ptr, dtype=np.int32)),
                     'thr_ptr': put(np.asarray(thr_ptr, dtype=np.int32)), 'thr_species': put(thr),
                     'aff_ptr': put(model.aff_ptr), 'seq': put(model.seq), 'seq2': put(model.seq2.view(np.int32)),
                     'term_strength': put(model.term_strength), 'term_from': put(model.term_from),
                     'thr_value': put(np.asarray(thr_value, dtype=np.float64)), 'affinity': put(model.affinity)}

    def table(self, dt) -> native.VkTxModel:
        m, d = self.model, native.VkTxModel()
        interval, elongate, d.n_plan = self.plan(dt)
        # n_species bounds the rows the kernel may touch: every row of the table, passive ones included
        d.n_templates, d.n_monomers, d.n_species = m.n_templates, m.n_monomers, self.stochastic_model.n_rows
        d.max_slots, d.occlusion, d.rnap_species = m.max_rnaps, m.polymerase_occlusion, self.rnap_species
        d.n_affinities, d.atp_row, d.adp_row, d.n_bases = len(m.affinity), m.atp_row, m.adp_row, len(m.seq)
        d.sequence = SEQUENCE[m.sequence_path]
        for k, v in self._dev.items():
            setattr(d, k, v.data_ptr())
        d.interval, d.elongate = interval.data_ptr(), elongate.data_ptr()
        return d

    def step(self, dt, slots, length, molecules, counts, mmol_to_counts, keys, n=None, events=None, status=None,
             step_counter=None, advance=True, max_events=None, seed=None):
        """One vk_transcription_step launch on the current stream for agents [0, n): ``slots``
        [max_rnaps, ld] and ``length`` [ld] (int32), ``molecules`` [len(molecule_ids), ld],
        ``counts`` [n_rows, ld] (the stochastic table, edited in place), ``mmol_to_counts`` [ld]
        (float64), ``keys`` [ld] (int64).  ``step_counter`` (one device int64, default the engine's
        own) is read, and advanced if ``advance``.  Returns (events [ld] int32, status [ld] int32:
        VK_TX_* bits OR-ed in)."""
        import torch
        m = self.model
        ld, n, events, status = self._check_step_tensors(slots, m.max_rnaps, length, molecules, counts, keys, n,
                                                         events, status)
        if (not torch.is_tensor(mmol_to_counts) or mmol_to_counts.dtype != torch.float64 or mmol_to_counts.dim() != 1 or
                mmol_to_counts.shape[0] < n or not mmol_to_counts.is_contiguous()):
            raise ValueError('TranscriptionEngine.step: mmol_to_counts must be a float64 device tensor over the agents')
        counter = self.step_counter if step_counter is None else step_counter
        d = self.table(dt)
        native.check(native._lib.vk_transcription_step(
            ctypes.byref(d), n, ld, native.ptr(slots), native.ptr(length), native.ptr(molecules), native.ptr(counts),
            native.ptr(mmol_to_counts), native.ptr(keys), (m.seed if seed is None else int(seed)) & (2 ** 64 - 1),
            native.ptr(counter), 1 if advance else 0, int(m.max_events if max_events is None else max_events),
            native.ptr(events), native.ptr(status), native.stream_handle()), 'vk_transcription_step')
        return events, status


def divide_rnaps(n_out, n_src, src, kind, slots_src, length_src, key_src, slots_dst, length_dst, seed, step):
    """The RNAP lists over a division plan: vk_divide_ribosomes as it is (it copies packed words and
    never looks inside them), under the transcription seed mixed with VK_TX_DIVIDE_DOMAIN."""
    divide_ribosomes(n_out, n_src, src, kind, slots_src, length_src, key_src, slots_dst, length_dst,
                     (int(seed) ^ native.VK_TX_DIVIDE_DOMAIN) & (2 ** 64 - 1), step)


POLYMERASE = Polymerase(model='transcription', slots='rnap_slots', count='rnap_count', molecules='tx_molecules',
                        max_slots='max_rnaps', check='check_rnaps', unpack=unpack, divide=divide_rnaps,
                        domain=native.VK_TX_DIVIDE_DOMAIN)
