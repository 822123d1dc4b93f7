"""What translation and transcription share on the host: the reference keeps it in one place too
(vivarium/library/polymerize.py, which both ``Translation`` and ``Transcription`` step through).

Here: the sub-interval plan, the status bits of a polymerase step (the same five for
vk_translation_step and vk_transcription_step), the checks of the parameters both models take,
the molecule pools, the engines' plan cache and tensor checks, and the colony's dividers of a
polymerase list and of a pool.  The device side of the same core is csrc/vk_polymerize.h.
What differs stays in lens_amd/translation.py and lens_amd/transcription.py: the config shapes,
the packed words and the tables the kernels read.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from lens_amd import native
from lens_amd.stochastic import _whole, divide_counts

assert (native.VK_TL_SLOTS_FULL, native.VK_TL_BAD_KEY, native.VK_TL_NONFINITE, native.VK_TL_OVERFLOW,
        native.VK_TL_MAX_EVENTS) == (native.VK_TX_SLOTS_FULL, native.VK_TX_BAD_KEY, native.VK_TX_NONFINITE,
                                     native.VK_TX_OVERFLOW, native.VK_TX_MAX_EVENTS)
STATUS_NAMES = ((native.VK_TL_SLOTS_FULL, '{} list full'), (native.VK_TL_BAD_KEY, 'key outside [0, 2**31)'),
                (native.VK_TL_NONFINITE, 'propensity not finite'),
                (native.VK_TL_OVERFLOW, 'a count would pass 2**31 - 1'), (native.VK_TL_MAX_EVENTS, 'max_events reached'))


def status_names(what: str):
    """STATUS_NAMES with the polymerase whose list is full named: ``what``."""
    return tuple((bit, text.format(what)) for bit, text in STATUS_NAMES)


def describe_status(bits: int, what: str) -> str:
    """The status bits of a polymerase step in words."""
    return ', '.join(text for bit, text in status_names(what) if bits & bit) or 'ok'


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


# What a colony holds for one kind of polymerase, by attribute name: the model, the list
# ([max][ld] packed words and its length), the pools, and how a list is checked, unpacked and dealt
# out at division (``divide``: divide_ribosomes or divide_rnaps; ``domain``: the pool divider's)
Polymerase = namedtuple('Polymerase', 'model slots count molecules max_slots check unpack divide domain')


class PolymeraseModel:
    """The parameters and pools both models have.  A subclass sets ``process`` (the prefix of its
    error texts) and ``molecule_ids`` / ``monomer_ids`` / ``seq_ptr``."""

    process = 'polymerize'

    def _check_parameters(self, elongation_rate, polymerase_occlusion, max_slots, max_name, limit, seed, max_events):
        """Sets elongation_rate, polymerase_occlusion, seed and max_events, and returns the checked
        ``max_slots`` (the model's ``max_name``: max_ribosomes or max_rnaps, 1..``limit``)."""
        what = self.process
        self.elongation_rate = elongation_rate
        if not (float(elongation_rate) > 0 and np.isfinite(float(elongation_rate))):
            raise ValueError('%s: elongation_rate must be finite and > 0' % what)
        self.polymerase_occlusion = _whole(polymerase_occlusion, '%s: polymerase_occlusion' % what)
        if not -2 ** 31 <= self.polymerase_occlusion <= 2 ** 31 - 1:
            raise ValueError('%s: polymerase_occlusion does not fit int32' % what)
        max_slots = _whole(max_slots, '%s: %s' % (what, max_name))
        if not 1 <= max_slots <= limit:
            raise ValueError('%s: %s must lie in 1..%d' % (what, max_name, limit))
        self.seed = int(seed)
        self.max_events = _whole(max_events, '%s: max_events' % what)
        if not 1 <= self.max_events <= 2 ** 31 - 1:
            raise ValueError('%s: max_events must lie in 1..2**31 - 1' % what)
        return max_slots

    @property
    def n_monomers(self):
        return len(self.monomer_ids)

    def length(self, template: int) -> int:
        return int(self.seq_ptr[template + 1] - self.seq_ptr[template])

    def plan(self, dt):
        return sub_intervals(dt, self.elongation_rate)

    def initial_molecules(self, n: int, ld: int, counts=None) -> np.ndarray:
        out = np.zeros((len(self.molecule_ids), ld), dtype=np.int32)
        for name, value in (counts or {}).items():
            if name not in self.molecule_ids:
                raise ValueError('%s: no molecule %r (molecules: %s)' % (self.process, name, self.molecule_ids))
            out[self.molecule_ids.index(name), :n] = np.asarray(value, dtype=np.int64)
        return out


class PolymeraseEngine:
    """A model bound to a :class:`StochasticModel`'s table, resident on one GPU: the device, the
    plan cache and the step word.  The engine holds the packed tables and the sub-interval plans as
    torch tensors; the library owns none of it."""

    def __init__(self, model, stochastic_model, device=None):
        import torch
        native.load()
        self.model, self.stochastic_model = model, stochastic_model
        self.device = native.resolve_device(device)
        self._plans = {}
        self.step_counter = torch.zeros(1, dtype=torch.int64, device=self.device)

    def put(self, a):
        """A host table on the device (an empty one as one zero, so that it has an address)."""
        import torch
        return torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros(1, dtype=a.dtype))).to(self.device)

    def plan(self, dt):
        """The sub-interval plan of a step of ``dt`` on the device: (interval float64 [K],
        elongate int32 [K], K).  Kept per ``dt``, so a captured graph's plan stays alive."""
        import torch
        dt = float(dt)
        if not (dt >= 0.0 and np.isfinite(dt)):
            raise ValueError('%s: dt must be finite and >= 0' % type(self).__name__)
        if dt not in self._plans:
            p = self.model.plan(dt)
            iv = np.asarray([x for x, _ in p] or [0.0], dtype=np.float64)
            el = np.asarray([int(y) for _, y in p] or [0], dtype=np.int32)
            self._plans[dt] = (torch.from_numpy(iv).to(self.device), torch.from_numpy(el).to(self.device), len(p))
        return self._plans[dt]

    def _check_step_tensors(self, slots, max_slots, length, molecules, counts, keys, n, events, status):
        """The tensor checks of ``step()``: (ld, n, events, status), the last two allocated if None."""
        import torch
        who = type(self).__name__
        ld = counts.shape[-1] if torch.is_tensor(counts) and counts.dim() == 2 else -1
        for t, rows, what in ((slots, max_slots, 'slots'), (molecules, len(self.model.molecule_ids), 'molecules'),
                              (counts, self.stochastic_model.n_rows, 'counts')):
            if (not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 2 or t.shape != (rows, ld) or
                    not t.is_contiguous()):
                raise ValueError('%s.step: %s must be a contiguous int32 [%d, ld] device tensor' % (who, what, rows))
        n = ld if n is None else int(n)
        if not 0 <= n <= ld:
            raise ValueError('%s.step: 0 <= n <= ld' % who)
        if not torch.is_tensor(length) or length.dtype != torch.int32 or length.dim() != 1 or length.shape[0] < n:
            raise ValueError('%s.step: length must be an int32 device tensor over the agents' % who)
        if not torch.is_tensor(keys) or keys.dtype != torch.int64 or keys.dim() != 1 or keys.shape[0] < n:
            raise ValueError('%s.step: keys must be an int64 device tensor over the agents' % who)
        if events is None:
            events = torch.zeros(ld, dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.zeros(ld, dtype=torch.int32, device=self.device)
        return ld, n, events, status


# -- the colony's dividers (population.DIVIDERS) ---------------------------------------------------

def divide_agent_list(col, plan, old, new, ld, pol: Polymerase):
    """A polymerase list entry by entry, a coin per (mother, entry) keyed by the mother's key (the old
    ``ssa_key``), under the seed of the model that owns the list."""
    pol.divide(plan.n_out, plan.n_src, plan.src, plan.kind, old[pol.slots], old[pol.count], old['ssa_key'],
               new[pol.slots], new[pol.count], getattr(col, pol.model).seed, col.step_index)


def divide_agent_pool(col, plan, old, new, ld, array, owner, domain):
    """The pool ``array`` of the colony's model ``owner``: divide_split like the stochastic counts
    (``'_divider': 'split'``), by the mothers' keys under ``domain``, a domain of the pool's own; the
    daughters' keys it would hand out are dropped."""
    import torch
    divide_counts(plan.n_out, plan.n_keep, plan.n_src, plan.src, plan.kind, old[array], old['ssa_key'], new[array],
                  torch.empty(ld, dtype=torch.int64, device=col.device), getattr(col, owner).seed ^ domain,
                  col.step_index, col._ssa_key_base)
