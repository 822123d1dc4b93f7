"""Who is in the colony: the table of per-agent arrays, the population plan, the dividers
and the one install.

Everything that changes which agents a colony holds, in what order or at what capacity goes
through here.  :func:`plan_population` turns divide / remove flags into a
:class:`PopulationPlan` (the only caller of vk_divide_plan / vk_population_plan);
:func:`regather` builds every per-agent array of the new population from the old ones, each by
the divider its row of the table names; :func:`install` puts new arrays into the colony (also
``Colony.sort_by_bin``'s and ``distributed.install_agents``').  Nothing here re-bins: callers
with a lattice call ``refresh_bins()`` after installing (``refresh_bins`` calls the router,
which installs).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from lens_amd import native
from lens_amd.motility import DIVISION_MODES
from lens_amd.polymerize import divide_agent_list, divide_agent_pool
from lens_amd.stochastic import divide_agent_counts
from lens_amd.transcription import POLYMERASE as RNAP
from lens_amd.translation import POLYMERASE as RIBOSOME

_SET, _SPLIT, _ZERO = native.VK_DIVIDE_SET, native.VK_DIVIDE_SPLIT, native.VK_DIVIDE_ZERO

# Every per-agent array (agent = column; the last dimension is the capacity ``ld``), in the
# order agent_array_names() reports, with its divider: what each daughter gets of the
# mother's value.  A vk_divide_gather mode, or row ranges (lo, hi, mode) of one, or the name
# of a divider with a launch of its own (DIVIDERS below).  A colony has an array if and only
# if the attribute is a tensor.  A new per-agent array is one row here, and a new divider one
# function in DIVIDERS.
# The order is also the dependency order: regather() runs the plain modes first, then each
# named divider once, in the order in which their first arrays stand here.  A named divider
# reads the old arrays; of the new ones it finds the plain-mode arrays (``cell``, which the
# divider of ``location`` reads) and those of the named dividers before it (``ssa`` /
# ``ssa_key`` stand before the translation arrays), and no others exist yet.
AGENT_ARRAYS = (
    ('params', _SET), ('conc', _SET), ('m2c', _SET), ('flux', _SET), ('counts', _SET), ('status', _SET),
    ('nsteps', _SET), ('h_state', _SET),
    ('location', 'locations'),           # daughters along the mother's angle (vk_divide_locations)
    ('cell', ((0, native.VK_CELL_ANGLE, _SPLIT), (native.VK_CELL_ANGLE, native.VK_CELL_ROWS, _SET))),
    ('divide', _ZERO),
    ('lin_root', 'lineage'), ('lin_depth', 'lineage'), ('lin_path', 'lineage'),      # vk_divide_lineage
    # 'dead' has no divider in the reference (both daughters inherit it); the daughters'
    # processes are generated anew, so they are not frozen
    ('dead', _SET), ('frozen', _ZERO),
    # the receptor's and the motor's scalars, PMF and the expression's concentrations have
    # no divider either.  The flagella count is split, the flagella go by the model's
    # ``division`` mode, daughters get fresh keys (vk_divide_flagella)
    ('motil', _SET), ('flag', _SET), ('flag_int', 'flagella'), ('flag_expr', _SET), ('motile_key', 'flagella'),
    ('mech_angle', _SET),
    ('ordinal', 'given'),                # the router's global order, computed by a collective
    ('env_fields', _SET),                # NonSpatialEnvironment: each agent's own 1x1 field
)
# The per-agent arrays of Colony(stochastic=...), two more rows of the same table, reported
# after the ones above: the int counts of the stochastic network, split by divide_split with
# a coin per (mother, species), and the key each agent draws by; daughters get fresh keys
# (vk_divide_counts).  With them stands TreeMass's ``global.initial_mass`` ([ld] FP64, fg), which
# only a colony whose CellModel is 'tree_mass' holds -- its mass is folded over these counts, so
# it always has them: the reference's '_divider': 'split' (tree_mass.py:41-45)
STOCHASTIC_ARRAYS = (('ssa', 'counts'), ('ssa_key', 'counts'), ('initial_mass', _SPLIT))
# The per-agent arrays of Colony(translation=...): the ribosome list ([max_ribosomes][ld], one
# packed word per ribosome, in insertion order) and its length, divided entry by entry with a
# coin per (mother, entry) (vk_divide_ribosomes), and the monomers, ATP and ADP, split by
# divide_split like the counts above (vk_divide_counts under a domain of its own)
TRANSLATION_ARRAYS = (('ribosome_slots', 'ribosomes'), ('ribosome_count', 'ribosomes'), ('tl_molecules', 'molecules'))
# The per-agent arrays of Colony(transcription=...): the RNAP list ([max_rnaps][ld], one packed
# word per RNAP, in insertion order) and its length, and the nucleotides, ATP and ADP.  They go by
# the dividers of the rows above: 'ribosomes' deals every polymerase list a colony holds (the same
# vk_divide_ribosomes, the RNAPs under the transcription seed), 'molecules' splits every pool
# (divide_split, each under a domain of its own)
TRANSCRIPTION_ARRAYS = (('rnap_slots', 'ribosomes'), ('rnap_count', 'ribosomes'), ('tx_molecules', 'molecules'))
# The per-agent array of Colony(degradation=...): the fraction of a transcript that the last step
# left undegraded ([n_transcripts][ld] FP64).  The reference generates the daughters' processes
# anew, so their ``partial_transcripts`` start at 0: the plain zero divider
DEGRADATION_ARRAYS = (('deg_partial', _ZERO),)
_ALL_AGENT_ARRAYS = AGENT_ARRAYS + STOCHASTIC_ARRAYS + TRANSLATION_ARRAYS + TRANSCRIPTION_ARRAYS + DEGRADATION_ARRAYS


@dataclass(frozen=True)
class PopulationPlan:
    """Slot j of the new population takes agent ``src[j]`` of the old one; ``kind[j]`` < 0 is a
    survivor, 0 / 1 a daughter (``src`` / ``kind``: device int32, ``n_out`` slots used).
    Survivors come first in their old order, then the daughters in mother order; a removed
    mother leaves no daughters.  ``ordinal``: the router's global order of the ``n_out`` agents."""
    n_src: int
    n_out: int
    n_removed: int
    src: torch.Tensor
    kind: torch.Tensor
    ordinal: Optional[torch.Tensor] = None

    @property
    def n_daughters(self):
        return 2 * (self.n_out - self.n_src + self.n_removed)

    @property
    def n_keep(self):
        return self.n_out - self.n_daughters

    @property
    def ptrs(self):
        """The leading arguments of every gather and divider launch."""
        return self.n_out, native.ptr(self.src), native.ptr(self.kind)


def plan_population(n, divide, remove, device):
    """The plan of agents [0, n) by their ``divide`` and ``remove`` flags (device int32, either
    may be None): vk_divide_plan without ``remove``, else vk_population_plan.  One host read:
    ``n_out``, and with both flags the number removed beside it (equal counts can hide a
    removal).  No agents: an empty plan and no launch."""
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=device)
    src, kind = (i32(2 * n), i32(2 * n)) if divide is not None else (i32(n), i32(n))
    if n == 0:
        return PopulationPlan(0, 0, 0, src, kind)
    n_out = torch.empty(1, dtype=torch.int64, device=device)
    lib, st = native._lib, native.stream_handle()
    if remove is None:
        scratch = torch.empty(int(lib.vk_divide_scratch_bytes(n)), dtype=torch.uint8, device=device)
        native.check(lib.vk_divide_plan(native.ptr(divide), n, native.ptr(src), native.ptr(kind), native.ptr(n_out),
                                        native.ptr(scratch), st), 'vk_divide_plan')
        return PopulationPlan(n, int(n_out.item()), 0, src, kind)
    scratch = torch.empty(int(lib.vk_population_scratch_bytes(n)), dtype=torch.uint8, device=device)
    native.check(lib.vk_population_plan(native.ptr(divide), native.ptr(remove), n, native.ptr(src), native.ptr(kind),
                                        native.ptr(n_out), native.ptr(scratch), st), 'vk_population_plan')
    if divide is None:
        n_out = int(n_out.item())
        return PopulationPlan(n, n_out, n - n_out, src, kind)
    n_out, n_removed = torch.stack([n_out[0], (remove[:n] != 0).sum()]).tolist()
    return PopulationPlan(n, n_out, n_removed, src, kind)


def grown_capacity(ld, n):
    """The capacity for ``n`` agents of a colony that has ``ld``: ``ld`` while they fit, else a
    quarter more than now (and at least ``n``).  The only copy of the rule."""
    return ld if n <= ld else max(n, int(ld * 1.25) + 64)


def install(col, arrays, n):
    """Put ``arrays`` ({name: tensor} over names of the table, all of one capacity; also
    ``agent_order``, n keys) into the colony ``col`` for ``n`` agents: the one place where
    per-agent arrays are replaced.  The sticky status words go by column, so they are read
    before the columns move; the scratch follows a changed capacity; ``_layout`` always moves,
    since captured graphs hold the old buffers.  Bins are the caller's (module docstring)."""
    known = {name for name, _ in _ALL_AGENT_ARRAYS}
    unknown = [name for name in arrays if name not in known and name != 'agent_order']
    if unknown:
        raise ValueError('install: %s: no per-agent arrays (population.AGENT_ARRAYS)' % ', '.join(unknown))
    lds = {t.shape[-1] for name, t in arrays.items() if name != 'agent_order'}
    if len(lds) != 1 or n > max(lds):
        raise ValueError('install: arrays of one capacity >= n (got %s for n = %d)' % (sorted(lds), n))
    if getattr(col, '_ssa', None) is not None:       # objects that only borrow the colony's hooks lack it
        col._ssa_check()
    for name, t in arrays.items():
        setattr(col, name, t)
    ld, = lds
    col.n = n
    if ld != col.ld:
        col.ld = ld
        col._capacity_scratch()
    col._layout += 1


# -- dividers with a launch of their own ------------------------------------------------------
# divider(col, plan, old, new, ld): reads ``old`` ({name: array} of the colony as it is) and
# writes its arrays in ``new`` (allocated, capacity ``ld``); it sets nothing on ``col``, so a
# refusal (OverflowError) leaves the colony as it was.  It may return a function of the colony
# to run once the new arrays are installed: its own bookkeeping.

def _lineage(old):
    return [native.ptr(old[name]) for name in ('lin_root', 'lin_depth', 'lin_path')]


def divide_lineage(col, plan, old, new, ld):
    native.check(native._lib.vk_divide_lineage(
        *plan.ptrs, *_lineage(old), *_lineage(new), native.ptr(col._overflow), native.stream_handle()),
        'vk_divide_lineage')

    def installed(col):
        if int(col._overflow.item()):
            raise OverflowError('a lineage exceeded 64 generations (phylogeny path bits)')
    return installed


def divide_locations(col, plan, old, new, ld):
    """Along the mother's angle, by a quarter of the length she had: the gathered cell rows."""
    native.check(native._lib.vk_divide_locations(
        *plan.ptrs, native.ptr(old['location']), col.ld, native.ptr(new['location']), ld, native.ptr(new['cell']),
        native.stream_handle()), 'vk_divide_locations')


def divide_flagella(col, plan, old, new, ld):
    """The split's draw is keyed by the mother's lineage; a colony on the coarse motor has no
    flagella and gets keys only."""
    m, base = col.motility, col._key_base
    if base + plan.n_daughters - 1 > 2 ** 31 - 1:
        raise OverflowError('a motility key would pass 2**31 - 1 (the kernels put it into a 32-bit counter word)')
    native.check(native._lib.vk_divide_flagella(
        plan.n_out, plan.n_keep, plan.n_src, native.ptr(plan.src), native.ptr(plan.kind),
        native.ptr(old.get('flag_int')), col.ld, native.ptr(old['motile_key']), *_lineage(old),
        native.ptr(new.get('flag_int')), ld, native.ptr(new['motile_key']), DIVISION_MODES[m.division],
        m.seed & (2 ** 64 - 1), col.step_index & (2 ** 64 - 1), base, native.stream_handle()), 'vk_divide_flagella')

    def installed(col):
        col._key_base = base + plan.n_daughters
    return installed


def divide_given(col, plan, old, new, ld):
    new['ordinal'].zero_()
    new['ordinal'][:plan.n_out] = plan.ordinal


POLYMERASES = (RIBOSOME, RNAP)            # the order of their rows in the table above


def divide_polymerases(col, plan, old, new, ld):
    """'ribosomes': every polymerase list the colony holds, each under the seed of her own model
    (vk_divide_ribosomes; THE ENGINE'S OWN rule for the RNAPs, whose store in the reference declares
    no divider)."""
    for pol in POLYMERASES:
        if pol.slots in old:
            divide_agent_list(col, plan, old, new, ld, pol)


def divide_pools(col, plan, old, new, ld):
    """'molecules': translation's monomer pools and transcription's nucleotide pools, each under a
    domain of its own."""
    for pol in POLYMERASES:
        if pol.molecules in old:
            divide_agent_pool(col, plan, old, new, ld, pol.molecules, pol.model, pol.domain)


DIVIDERS = {'locations': divide_locations, 'lineage': divide_lineage, 'flagella': divide_flagella,
            'given': divide_given, 'counts': divide_agent_counts, 'ribosomes': divide_polymerases,
            'molecules': divide_pools}


def regather(col, plan, declared=True):
    """Every per-agent array of ``col`` gathered once by ``plan`` and installed, the capacity
    grown when ``plan.n_out`` passes it: each array with the divider its row declares into
    uninitialised arrays (division), or, ``declared=False``, all with the set divider into
    zero-filled ones (removal: the plan holds no daughters; ``agent_order`` is compacted to
    its ``n_out`` keys).  Only the old arrays are read; then bins and occupancies are rebuilt."""
    dev, st = col.device, native.stream_handle()
    ld = grown_capacity(col.ld, plan.n_out)
    alloc = torch.empty if declared else torch.zeros
    old = {name: getattr(col, name) for name in col.agent_array_names()}
    new, named = {}, {}

    def gather(name, t, ld_dst, ranges):
        t = t.contiguous()               # flux / counts / nsteps may view step_many's buffers
        out = alloc(t.shape[:-1] + (ld_dst,), dtype=t.dtype, device=dev)
        size, ld_t = t.element_size(), t.shape[-1]
        for lo, hi, mode in ranges:
            rows = 1 if t.dim() == 1 else (t.shape[0] if hi is None else hi) - lo
            native.check(native._lib.vk_divide_gather(
                *plan.ptrs, t.data_ptr() + lo * ld_t * size, ld_t, out.data_ptr() + lo * ld_dst * size, ld_dst, rows,
                size, mode, st), 'vk_divide_gather(%s)' % name)
        return out

    for name, divider in _ALL_AGENT_ARRAYS:
        if name not in old:
            continue
        if not declared:
            divider = _SET
        if isinstance(divider, int):
            divider = ((0, None, divider),)          # every row
        if isinstance(divider, tuple):
            new[name] = gather(name, old[name], ld, divider)
        else:
            named.setdefault(divider, []).append(name)
    if not declared and col.agent_order is not None:
        new['agent_order'] = gather('agent_order', col.agent_order, plan.n_out, ((0, None, _SET),))
    installed = []
    for divider, names in named.items():             # in table order
        for name in names:
            new[name] = torch.empty(old[name].shape[:-1] + (ld,), dtype=old[name].dtype, device=dev)
        installed.append(DIVIDERS[divider](col, plan, old, new, ld))
    install(col, new, plan.n_out)
    for after in installed:
        if after is not None:
            after(col)
    if col.lattice is not None:
        col.refresh_bins()               # bins, host and device occupancy
