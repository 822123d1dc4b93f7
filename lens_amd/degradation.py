"""RNA degradation per agent: endoRNAses degrade transcripts by Michaelis-Menten kinetics and
return their nucleotides to the pool.

The reference's ``RnaDegradation`` (vivarium/processes/degradation.py:136-182) sums, per
transcript, ``kcat * E * S / (S + km)`` over the enzymes that name it, scales the level by
``mmol_to_counts`` and the timestep, adds the fraction the previous step left
(``partial_transcripts``), removes the whole part and keeps the rest.  Here every agent of a
colony advances by one launch per timestep (vk_rna_degradation_step): one agent per lane, her
transcripts and enzymes rows of a :class:`~lens_amd.stochastic.StochasticModel`'s int table
(active or passive rows), her carry a column of an FP64 ``[n_transcripts][ld]`` array, her
nucleotides, ATP and ADP the pools of the :class:`~lens_amd.transcription.TranscriptionModel`.

The reference's, operation for operation: the rate law and its order of evaluation, the carry,
and the books with their signs -- the reference subtracts a negative count, so a degraded base
RAISES ATP by one and LOWERS ADP by one (degradation.py:172-178); kept, as the transcription
step keeps its ATP quirk.

THE ENGINE'S OWN, not the reference's: the clamp ``d <= counts[t]`` (the reference would let a
transcript go negative, and translation reads the counts as its unbound transcripts; the excess
is dropped, the carry keeps only the fraction); the process edits the int table in place after
translation and in front of the network (the reference applies every process's update to the
step-start state); and the factor :data:`KM_TO_MM` below.  The step is stated above
``vk_rna_degradation_step`` in include/vk_kinetics.h and restated as Python loops by
tests/degradation_ref.py; DESIGN.md §22 says what is and what is not the reference.
"""

from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence

import numpy as np

from lens_amd import native
from lens_amd.stochastic import StochasticModel
from lens_amd.transcription import NUCLEOTIDES, TranscriptionModel

MAX_TRANSCRIPTS, MAX_ENZYMES, MAX_PAIRS = native.VK_DEG_MAX_TRANSCRIPTS, native.VK_DEG_MAX_ENZYMES, native.VK_DEG_MAX_PAIRS
MAX_MONOMERS, MAX_LENGTH = native.VK_DEG_MAX_MONOMERS, native.VK_DEG_MAX_LENGTH
# The reference multiplies each km by ``units.mole / units.fL`` and adds it to a level in mmol / L
# (degradation.py:148-153), so pint converts mol / fL to mM: 1 mol / fL = 1e15 mol / L = 1e18 mM.
# NOT VERIFIED: pint is not available where this was written, so whether pint's own conversion
# gives the bits of ``km * 1e18`` (it may multiply by other factors in another order) is unknown.
KM_TO_MM = 1e18
STATUS_NAMES = ((native.VK_DEG_NONFINITE, 'mmol_to_counts not finite and > 0, or a level not finite'),
                (native.VK_DEG_OVERFLOW, 'a pool would leave int32'))


def describe_status(bits: int) -> str:
    return ', '.join(text for bit, text in STATUS_NAMES if bits & bit) or 'ok'


def _positive(x, what):
    try:
        x = float(x)
    except (TypeError, ValueError):
        raise ValueError('degradation: %s must be a number (got %r)' % (what, x))
    if not math.isfinite(x) or not x > 0:
        raise ValueError('degradation: %s must be finite and > 0 (got %r)' % (what, x))
    return x


class DegradationModel:
    """An RNA degradation process in the reference's config shapes.

    ``sequences``: ``{transcript: 'GCC...'}``, whose key order is the transcript order.
    ``catalytic_rates``: ``{enzyme: kcat}``, whose key order is the enzyme order.
    ``michaelis_constants``: ``{'transcripts': {enzyme: {transcript: km}}}``, each km a plain
    magnitude in mol / fL (the reference's number before ``* units.mole / units.fL``).  A
    transcript no enzyme names is never degraded.  ``transcript_species``: ``{transcript:
    species}``, the name a transcript has in the stochastic table where it is not its own.
    ``symbol_to_monomer`` / ``monomer_ids``: as the TranscriptionModel's; the pools are hers, so
    :meth:`bind` asks for the same ``monomer_ids``."""

    def __init__(self, sequences: Dict[str, str], catalytic_rates: Dict[str, float], michaelis_constants,
                 transcript_species: Optional[Dict[str, str]] = None,
                 symbol_to_monomer: Optional[Dict[str, str]] = None, monomer_ids: Optional[Sequence[str]] = None):
        symbol_to_monomer = dict(NUCLEOTIDES if symbol_to_monomer is None else symbol_to_monomer)
        self.monomer_ids = [str(m) for m in (list(NUCLEOTIDES.values()) if monomer_ids is None else monomer_ids)]
        if len(set(self.monomer_ids)) != len(self.monomer_ids) or 'ADP' in self.monomer_ids:
            raise ValueError('degradation: monomer_ids must be distinct and not ADP')
        if not 1 <= len(self.monomer_ids) <= MAX_MONOMERS:
            raise ValueError('degradation: 1..%d monomers (got %d)' % (MAX_MONOMERS, len(self.monomer_ids)))
        self.molecule_ids = self.monomer_ids + ([] if 'ATP' in self.monomer_ids else ['ATP']) + ['ADP']
        self.atp_row, self.adp_row = self.molecule_ids.index('ATP'), len(self.molecule_ids) - 1
        row = {m: i for i, m in enumerate(self.monomer_ids)}
        self.transcript_order = [str(t) for t in sequences.keys()]
        self.enzyme_order = [str(e) for e in catalytic_rates.keys()]
        T, E = len(self.transcript_order), len(self.enzyme_order)
        if not 1 <= T <= MAX_TRANSCRIPTS:
            raise ValueError('degradation: 1..%d transcripts (got %d)' % (MAX_TRANSCRIPTS, T))
        if not 1 <= E <= MAX_ENZYMES:
            raise ValueError('degradation: 1..%d enzymes (got %d)' % (MAX_ENZYMES, E))
        self.sequences = {str(t): str(s) for t, s in sequences.items()}
        self.kcat = {str(e): _positive(k, 'the catalytic rate of %r' % (e,)) for e, k in catalytic_rates.items()}
        constants = (michaelis_constants or {}).get('transcripts', {})
        for enzyme, kms in constants.items():
            if str(enzyme) not in self.kcat:
                raise ValueError('degradation: michaelis_constants names the enzyme %r, which has no catalytic rate' % (
                    enzyme,))
            for transcript in kms:
                if str(transcript) not in self.sequences:
                    raise ValueError('degradation: michaelis_constants names the transcript %r, which has no sequence' % (
                        transcript,))
        self.km = {str(e): {str(t): _positive(km, 'the km of %r at %r' % (t, e)) for t, km in kms.items()}
                   for e, kms in constants.items()}
        self.transcript_species = {str(k): str(v) for k, v in (transcript_species or {}).items()}
        unknown = set(self.transcript_species) - set(self.transcript_order)
        if unknown:
            raise ValueError('degradation: transcript_species names the unknown transcripts %s' % sorted(unknown))
        names = [self.transcript_species.get(t, t) for t in self.transcript_order]
        if len(set(names)) != len(names) or set(names) & set(self.enzyme_order):
            raise ValueError('degradation: the transcripts\' species must be distinct and no enzymes')
        self.composition = np.zeros((T, MAX_MONOMERS), dtype=np.int32)
        for t, name in enumerate(self.transcript_order):
            sequence = self.sequences[name]
            if len(sequence) > MAX_LENGTH:
                raise ValueError('degradation: transcript %r is longer than %d bases' % (name, MAX_LENGTH))
            for symbol in sequence:
                if symbol not in symbol_to_monomer or symbol_to_monomer[symbol] not in row:
                    raise ValueError('degradation: symbol %r of %r has no monomer among monomer_ids' % (symbol, name))
                self.composition[t, row[symbol_to_monomer[symbol]]] += 1
        self.length = self.composition.sum(axis=1).astype(np.int32)
        # the pairs of each transcript in the reference's loop order (degradation.py:146-147): enzymes in
        # catalytic_rates order; within a transcript that is the order her terms are added in
        ptr, enzyme, kcat, km = [0], [], [], []
        for name in self.transcript_order:
            for e, ename in enumerate(self.enzyme_order):
                if name in self.km.get(ename, {}):
                    enzyme.append(e)
                    kcat.append(self.kcat[ename])
                    km.append(self.km[ename][name] * KM_TO_MM)
            ptr.append(len(enzyme))
        if len(enzyme) > MAX_PAIRS:
            raise ValueError('degradation: %d (enzyme, transcript) pairs (at most %d)' % (len(enzyme), MAX_PAIRS))
        self.pair_ptr, self.pair_enzyme = np.asarray(ptr, dtype=np.int32), np.asarray(enzyme, dtype=np.int32)
        self.pair_kcat, self.pair_km = np.asarray(kcat, dtype=np.float64), np.asarray(km, dtype=np.float64)

    @classmethod
    def from_transcription(cls, transcription: TranscriptionModel, catalytic_rates, michaelis_constants, **model):
        """The model whose sequences are ``transcription.product_sequences()`` and whose monomers
        and species names are the transcription model's."""
        model.setdefault('monomer_ids', transcription.monomer_ids)
        model.setdefault('transcript_species', dict(transcription.transcript_species))
        return cls(transcription.product_sequences(), catalytic_rates, michaelis_constants, **model)

    @property
    def n_transcripts(self):
        return len(self.transcript_order)

    @property
    def n_enzymes(self):
        return len(self.enzyme_order)

    @property
    def n_pairs(self):
        return len(self.pair_enzyme)

    @property
    def n_monomers(self):
        return len(self.monomer_ids)

    def transcript_names(self):
        """The transcripts' species of the stochastic table, in transcript order."""
        return [self.transcript_species.get(t, t) for t in self.transcript_order]

    def species(self):
        """Every row the stochastic table must hold: the transcripts, then the enzymes."""
        return self.transcript_names() + list(self.enzyme_order)

    def bind(self, stochastic: StochasticModel, transcription: TranscriptionModel):
        """(transcript_row [T], enzyme_row [E]): rows of the stochastic table.  ValueError if the
        table lacks a species or the transcription model holds other pools."""
        if not isinstance(stochastic, StochasticModel):
            raise ValueError('degradation needs a StochasticModel (stochastic=) that holds its transcripts and enzymes')
        if not hasattr(transcription, 'molecule_ids'):       # a TranscriptionModel, or what names her pools' rows
            raise ValueError('degradation needs a TranscriptionModel (transcription=): the nucleotide pools are hers')
        if list(transcription.molecule_ids) != self.molecule_ids:
            raise ValueError('degradation: the transcription model\'s pools are %s, not %s' % (
                transcription.molecule_ids, self.molecule_ids))
        missing = [s for s in self.species() if s not in stochastic.rows]
        if missing:
            raise ValueError('degradation: the StochasticModel lacks the species %s' % missing)
        return (np.asarray([stochastic.index(s) for s in self.transcript_names()], dtype=np.int32),
                np.asarray([stochastic.index(s) for s in self.enzyme_order], dtype=np.int32))


class DegradationEngine:
    """A :class:`DegradationModel` bound to a :class:`StochasticModel`'s table and a
    :class:`TranscriptionModel`'s pools, resident on one GPU.  The engine holds the packed model as
    torch tensors; the library owns none of it."""

    def __init__(self, model: DegradationModel, stochastic_model: StochasticModel, transcription_model: TranscriptionModel,
                 device=None):
        import torch
        if not isinstance(model, DegradationModel):
            raise ValueError('DegradationEngine: a DegradationModel')
        transcript_row, enzyme_row = model.bind(stochastic_model, transcription_model)     # before anything is built
        native.load()
        self.model, self.stochastic_model = model, stochastic_model
        self.device = native.resolve_device(device)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros(1, dtype=a.dtype))).to(self.device)
        self._dev = {'transcript_row': put(transcript_row), 'enzyme_row': put(enzyme_row), 'pair_ptr': put(model.pair_ptr),
                     'pair_enzyme': put(model.pair_enzyme), 'composition': put(model.composition.reshape(-1)),
                     'length': put(model.length), 'kcat': put(model.pair_kcat), 'km': put(model.pair_km)}

    def table(self) -> native.VkDegModel:
        m, d = self.model, native.VkDegModel()
        d.n_transcripts, d.n_enzymes, d.n_pairs, d.n_monomers = m.n_transcripts, m.n_enzymes, m.n_pairs, m.n_monomers
        d.n_rows, d.atp_row, d.adp_row = self.stochastic_model.n_rows, m.atp_row, m.adp_row
        for k, v in self._dev.items():
            setattr(d, k, v.data_ptr())
        return d

    def step(self, timestep, counts, partial, molecules, mmol_to_counts, n=None, degraded=None, status=None):
        """One vk_rna_degradation_step launch on the current stream for agents [0, n): ``counts``
        [n_rows, ld] (int32, the stochastic table, edited in place), ``partial`` [n_transcripts, ld]
        (float64, the carry), ``molecules`` [len(molecule_ids), ld] (int32, transcription's pools),
        ``mmol_to_counts`` [ld] (float64).  Returns (degraded [ld] int32: the transcripts each agent
        lost, status [ld] int32: VK_DEG_* bits OR-ed in)."""
        import torch
        m = self.model
        ld = counts.shape[-1] if torch.is_tensor(counts) and counts.dim() == 2 else -1
        for t, rows, dtype, what in ((counts, self.stochastic_model.n_rows, torch.int32, 'counts'),
                                     (partial, m.n_transcripts, torch.float64, 'partial'),
                                     (molecules, len(m.molecule_ids), torch.int32, 'molecules')):
            if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 2 or t.shape != (rows, ld) or not t.is_contiguous():
                raise ValueError('DegradationEngine.step: %s must be a contiguous %s [%d, ld] device tensor' % (
                    what, str(dtype).replace('torch.', ''), rows))
        n = ld if n is None else int(n)
        if not 0 <= n <= ld:
            raise ValueError('DegradationEngine.step: 0 <= n <= ld')
        if (not torch.is_tensor(mmol_to_counts) or mmol_to_counts.dtype != torch.float64 or mmol_to_counts.dim() != 1 or
                mmol_to_counts.shape[0] < n or not mmol_to_counts.is_contiguous()):
            raise ValueError('DegradationEngine.step: mmol_to_counts must be a float64 device tensor over the agents')
        if degraded is None:
            degraded = torch.zeros(ld, dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.zeros(ld, dtype=torch.int32, device=self.device)
        for t, what in ((degraded, 'degraded'), (status, 'status')):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < n:
                raise ValueError('DegradationEngine.step: %s must be an int32 device tensor over the agents' % what)
        d = self.table()
        native.check(native._lib.vk_rna_degradation_step(
            ctypes.byref(d), n, ld, float(timestep), native.ptr(counts), native.ptr(partial), native.ptr(molecules),
            native.ptr(mmol_to_counts), native.ptr(degraded), native.ptr(status), native.stream_handle()),
            'vk_rna_degradation_step')
        return degraded, status
