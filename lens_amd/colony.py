"""Persistent SoA colony: the batched replacement of the reference's per-agent loop.

The reference advances a colony by walking its Store tree once per agent and
per process every timestep (``Experiment.update``, vivarium/core/experiment.py:
1351-1450; 59-154 us of Python per agent-step).  Here every
agent is a column of device-resident FP64 arrays and one timestep is a fixed
sequence of kernel launches on one stream:

environment ``'held'`` (BASELINE config 2)
    kinetics only; external concentrations stay at their per-agent values.
environment ``'nonspatial'`` (config 1; NonSpatialEnvironment per agent,
vivarium/processes/nonspatial_environment.py:14-82)
    kinetics -> exchange into each agent's own 1x1 field -> external := field.
a :class:`~lens_amd.lattice.Lattice` (configs 3-4; DiffusionField + agents)
    kinetics (external from the previous step: the reference's one-step lag)
    -> gather external := pre-step field at the agent's bin
    -> diffusion substeps -> exchange scatter in agent order.
a :class:`~lens_amd.static_field.StaticField` (the reference's static lattice without its
multibody; vivarium/processes/static_field.py)
    kinetics (external from the previous step) -> external := the analytic gradient at the
    agent's own position (vk_static_gather).  No field store: exchange counts are dropped.
    A motile colony senses the gradient where it is (the _static launches), not a bin.

Step order and quirks follow SURVEY.md Appendix A.5.

With a :class:`~lens_amd.motility.MotilityModel` a lattice colony's step starts
with the move: each agent senses the pre-step ligand plane, its receptor and
motor update (the reference's chemoreceptor_cluster.py / coarse_motor.py), it
runs or tumbles (this engine's kinematics, not the reference's multibody), and
the bins and their agent-ordered occupancy are rebuilt on the device -- then
the step above, with the exchange going into the bin the agent has reached.
A model with ``flagella=FlagellaModel(...)`` runs the reference's multi-flagellar
motor (flagella_activity.py) in the coarse motor's place, on two more per-agent
arrays (``flag``, ``flag_int``); :meth:`Colony.set_flagella` changes the counts.
With ``FlagellaModel(expression=...)`` the counts follow an expressed protein instead
(``flag_expr``: vk_expression_step, then the counts deriver vk_flagella_counts, before
the growth launch touches ``mmol_to_counts``).  A model with ``division=`` combines with
``cells=``: the cell's angle is the swimming direction, every agent draws by a key of
her own (``motile_key``), and division hands the motile state to the daughters with the
reference's dividers (vk_divide_flagella; the reference's ChemotaxisODEExpressionFlagella).

With a :class:`~lens_amd.mechanics.ContactModel` (``mechanics=``) the step starts
with the contact launch instead: overlapping capsules push each other apart
(this engine's own contact model, standing where the reference runs its pymunk
multibody), and the bins and their occupancy are rebuilt on the device in the
same way.  It combines with ``cells=``: growth and division then produce an
expanding colony instead of a pile of overlapping daughters.

A ContactModel with ``channels=`` makes the plane the reference's mother machine: the
contact launch keeps every cell in its channel and flags the cells pushed out of
the top, which take part in the step (their exchange lands) and leave at its end,
in the same plan as division (vk_population_plan), or through :meth:`Colony.remove`
when there are no cells.  ``remove(mask)`` takes agents out of any unrouted colony.

:meth:`Colony.colony_metrics` says which cells of such a colony form a connected colony
and gives each colony's cell count, mass, area, centroid and axes (lens_amd/colonies.py,
standing where the reference's ColonyShapeDeriver emits ``colony_global``); it is a call
of its own and no part of the step.

With a :class:`~lens_amd.response.CellResponse` (``response=``) each agent is the
reference's antibiotic-response cell: before the kinetics launch the death
detector and the membrane's porin diffusion are evaluated from the step-start
state and the pump's expression goes into an update buffer; after it the updates
are applied in the compartment's process order (kinetics, expression, membrane
last), dying agents are marked dead and frozen, and a frozen agent's kinetics,
growth and expression results are discarded while its membrane keeps leaking.
The exchange then adds each agent's int64 kinetic counts and its float membrane
counts to the field, agent after agent.

With a :class:`~lens_amd.stochastic.StochasticModel` (``stochastic=``) every agent also
carries the int counts of a mass-action network (``ssa``) and a key of her own for its
draws (``ssa_key``); at the end of the step, where the expression step sits and before
growth and division, the network advances by the Gillespie direct method (vk_ssa_step),
and division splits the counts with the reference's ``divide_split`` (vk_divide_counts).
``FlagellaModel(0, complexes='flagella')`` then takes the flagella count from that species.

With a :class:`~lens_amd.translation.TranslationModel` (``translation=``, beside
``stochastic=``) every agent also carries an ordered ribosome list (``ribosome_slots``,
``ribosome_count``) and her monomer, ATP and ADP pools (``tl_molecules``).  Right before the
network's step the ribosomes elongate and bind transcripts (vk_translation_step), editing the
``ssa`` counts in place: transcripts, proteins and free ribosomes are species of that table.
Division splits the pools with ``divide_split`` and deals the ribosomes out by a coin each
(vk_divide_ribosomes).

With a :class:`~lens_amd.transcription.TranscriptionModel` (``transcription=``, beside
``stochastic=``; ``translation=`` is not needed) every agent carries an ordered RNAP list
(``rnap_slots``, ``rnap_count``) and her nucleotide, ATP and ADP pools (``tx_molecules``).  In
front of the translation launch the RNAPs elongate, read through or terminate, and bind the
promoters whose affinity the factor levels (``ssa`` counts / ``mmol_to_counts``) switch
(vk_transcription_step), editing the ``ssa`` counts in place: promoters -> transcripts ->
proteins -> complexes -> motor with no host read in the step.  Division deals the RNAPs out by
a coin each (vk_divide_ribosomes under the transcription seed) and splits the pools.

With a :class:`~lens_amd.degradation.DegradationModel` (``degradation=``, beside ``stochastic=``
and ``transcription=``, whose pools it refills) every agent also carries the fraction of each
transcript the last step left undegraded (``deg_partial``).  After the translation launch and in
front of the network's, in the compartment's process order, endoRNAses degrade the transcripts
by the reference's Michaelis-Menten law (vk_rna_degradation_step), editing the ``ssa`` counts
and the ``tx_molecules`` pools in place.  Daughters start with a carry of 0.  The table may hold
rows that no reaction names (``StochasticModel(passive=...)``), so the whole flagella chromosome
runs in one colony (``configs.flagella_gene_expression``).

With a :class:`~lens_amd.cells.CellModel` the step continues like the
reference's deriver pass: the growth process (from the step-start state),
then TreeMass / DeriveGlobals (``mmol_to_counts`` for the next step's
exchange), then division: survivors keep their order, daughters are appended
in mother order, every per-agent array is gathered once with its divider.

Which agents the colony holds, in what order and at what capacity changes in one place,
lens_amd/population.py: division, removal and the mother machine's outflow take one plan
(``plan_population``) and gather by the table of per-agent arrays (``regather``); they,
:meth:`Colony.sort_by_bin` and the router's migration end in one ``install``, which reads the
sticky status words before the columns move and always moves ``_layout``.
"""

from __future__ import annotations

import ctypes
import dataclasses
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from lens_amd import native
from lens_amd.cells import CellModel, cell_step_tree, lineage_ids
from lens_amd.colonies import ColonyShape, ColonyShapeModel
from lens_amd.configs import initial_conc
from lens_amd.degradation import DegradationEngine, DegradationModel, describe_status as describe_deg_status
from lens_amd.expression import ExpressionEngine
from lens_amd.kinetics import KineticsEngine
from lens_amd.lattice import Lattice, occupancy, segment_index, whole_plane, N_A_LEGACY
from lens_amd.mechanics import ContactBuffers, ContactModel, contact_step
from lens_amd.motility import (DeviceOccupancy, MotilityModel, ROW_NAMES as MOTIL_ROW_NAMES, FLAG_ROW_NAMES,
                               FLAGI_ROW_NAMES, check_flagella_counts, flagella_step, motility_step)
# the table of per-agent arrays and everything that re-lays a colony out (lens_amd/population.py)
from lens_amd.population import (AGENT_ARRAYS, POLYMERASES, _ALL_AGENT_ARRAYS, install, plan_population,
                                 regather)
from lens_amd.rate_law_compiler import compile_rate_laws, RateLawTable
from lens_amd.response import CellResponse, ResponseBuffers, ResponseEngine
from lens_amd.static_field import StaticField
from lens_amd.stochastic import StochasticEngine, StochasticModel, describe_status, flagella_target
from lens_amd.transcription import (TranscriptionEngine, TranscriptionModel, describe_status as describe_tx_status,
                                    POLYMERASE as RNAP)
from lens_amd.translation import (TranslationEngine, TranslationModel, describe_status as describe_tl_status,
                                  POLYMERASE as RIBOSOME)


def mmol_to_counts_from_mass(mass_fg, density_g_per_L=1100.0, avogadro=N_A_LEGACY):
    """DeriveGlobals: (N_A/mol * mass/density).to('L/mmol') (derive_globals.py:219-220)."""
    return avogadro * (mass_fg / density_g_per_L * 1e-15) * 1e-3


# Tensors sized by the capacity that are not per-agent state: Colony._capacity_scratch
# allocates them (the first row) or drops them for their users to allocate again (the second)
CAPACITY_SCRATCH = ('bin_lin', 'bin_ix', 'env_bins', 'outflow', '_flag_expr_update', 'ssa_events', '_ssa_status',
                    'tl_events', '_tl_status', 'tx_events', '_tx_status', 'deg_degraded', '_deg_status',
                    '_counts_alt', 'flux_steps', 'counts_steps', 'nsteps_steps', '_colony_shape')

# The stochastic stages of a step, in step order (Colony._finish_step), by attribute name: the
# engine, the events each agent had in the last step and her sticky status word (both capacity
# scratch), the label and the wording of a raised status, and for the two polymerases the record of
# their lists and pools (lens_amd/polymerize.py).  A colony has a stage if and only if it has the
# engine.  A new stage is one row here, its launch in _finish_step and its arrays in population.py.
Stage = namedtuple('Stage', 'engine events status label describe polymerase', defaults=(None,))
STOCHASTIC_STAGES = (
    Stage('_tx', 'tx_events', '_tx_status', 'transcription', describe_tx_status, RNAP),
    Stage('_tl', 'tl_events', '_tl_status', 'translation', describe_tl_status, RIBOSOME),
    Stage('_deg', 'deg_degraded', '_deg_status', 'degradation', describe_deg_status),
    Stage('_ssa', 'ssa_events', '_ssa_status', 'stochastic', describe_status),
)
# the order in which a raised status is reported: the network's first, then by age of the stage
_REPORT_ORDER = tuple(stage for engine in ('_ssa', '_tl', '_tx', '_deg')
                      for stage in STOCHASTIC_STAGES if stage.engine == engine)
# the polymerases' stages in the order of their arrays (population.POLYMERASES): snapshot()'s order
_POLYMERASE_STAGES = tuple(stage for pol in POLYMERASES for stage in STOCHASTIC_STAGES if stage.polymerase is pol)


def stage_attributes(stage):
    """Every Colony attribute a stage names; all of them are None on a colony without the stage."""
    pol = stage.polymerase
    return (stage.engine,) + (() if pol is None else (pol.model, pol.slots, pol.count, pol.molecules))


class Colony:
    # optional state that a colony may never get (and that objects made by Colony.__new__ lack)
    location = ordinal = env_fields = None       # set with a lattice / by the router / nonspatial
    static = None                                # Colony(environment=StaticField(...))
    agent_order = None       # sort_by_bin: the reference index of the agent in each column
    attempts = None          # count_attempts
    _flag_expression = _flag_flags = None        # FlagellaModel(expression=...) / (complexes=...)
    # Colony(stochastic=..., translation=..., transcription=..., degradation=...): what the table of
    # stages does not name; the engines, lists and pools it names are declared below the class
    stochastic = ssa = ssa_key = degradation = deg_partial = None
    _tree = initial_mass = None                  # CellModel(molecular_weights=...) / model='tree_mass'
    _x_stream = _p_stream = None                 # capture(overlap=True)
    _counts_alt = flux_steps = counts_steps = nsteps_steps = None    # capture(overlap=True), step_many
    _colony_shape = None                         # colony_metrics

    def __init__(self, config, n_agents: int, *, capacity: Optional[int] = None, device=None,
                 integrator: str = 'dopri5', rtol: float = 1e-8, atol: float = 1e-12,
                 max_steps: int = 100000, environment='held', env_volume_L: float = 1e-14,
                 avogadro: float = N_A_LEGACY, exchange: str = 'sorted', mass_fg: float = 1339.0,
                 table: Optional[RateLawTable] = None, specialize: bool = False,
                 cells: Optional[CellModel] = None, agent_ids=None, motility: Optional[MotilityModel] = None,
                 mechanics: Optional[ContactModel] = None, response: Optional[CellResponse] = None,
                 stochastic: Optional[StochasticModel] = None, translation: Optional[TranslationModel] = None,
                 transcription: Optional[TranscriptionModel] = None,
                 degradation: Optional[DegradationModel] = None):
        if integrator not in ('euler', 'dopri5'):
            raise ValueError('integrator must be euler or dopri5')
        if exchange not in ('sorted', 'atomic'):
            raise ValueError('exchange must be sorted or atomic')
        static = environment if isinstance(environment, StaticField) else None
        if static is not None:
            # checked before anything is built: a static field is the reference's static lattice
            # without its multibody -- there is no field store to exchange with and nothing
            # that places a capsule or a daughter
            for given, what, why in (
                    (mechanics, 'mechanics', 'capsules push each other on a Lattice plane'),
                    (response, 'response', 'the membrane needs a field to exchange with'),
                    (cells, 'cells', 'growth and division are out of scope on a static field'),
                    (stochastic, 'stochastic', 'the stochastic network is out of scope on a static field')):
                if given is not None:
                    raise ValueError('a StaticField environment takes no %s= (%s)' % (what, why))
            if motility is not None and motility.ligand_id not in static.gradient_molecules:
                raise ValueError('motility: the static field has no gradient of %r (gradient molecules: %s)' % (
                    motility.ligand_id, static.gradient_molecules))
        if motility is not None and static is None:
            # checked before anything is built: a motile colony moves and re-bins its
            # agents on the device, on one whole plane (row bands: not yet; division when the
            # model says how the motile state divides)
            if not isinstance(environment, Lattice):
                raise ValueError('motility needs a Lattice environment (agents move through its ligand plane) or a '
                                 'StaticField (they sense its gradient where they are)')
            if motility.ligand_id not in environment.molecules:
                raise ValueError('motility: the lattice has no %r plane (molecules: %s)' % (
                    motility.ligand_id, environment.molecules))
            if not whole_plane(environment):
                raise ValueError('motility needs a whole, unbanded plane (row bands are not supported)')
            if cells is not None and motility.division is None:
                # the model must say how the motile state divides (MotilityModel(division=...))
                raise ValueError('motility with cells (growth and division) is not supported')
        complexes = motility.flagella.complexes if motility is not None and motility.flagella is not None else None
        if complexes is not None and stochastic is None:
            raise ValueError('FlagellaModel(complexes=%r) needs a colony with stochastic=StochasticModel(...)' % (
                complexes,))
        if stochastic is not None:
            # checked before anything is built: the draws go by a key per agent that is not
            # global across ranks, and a frozen agent would need its counts saved and restored
            if not isinstance(stochastic, StochasticModel):
                raise ValueError('stochastic must be a StochasticModel')
            if isinstance(environment, Lattice) and not whole_plane(environment):
                raise ValueError('stochastic needs a whole, unbanded plane (row bands are not supported: the draw '
                                 'keys are not global across ranks)')
            if response is not None:
                raise ValueError('stochastic with response is not supported (a frozen agent would need its counts '
                                 'saved and restored)')
            if complexes is not None:
                stochastic.index(complexes)      # ValueError: the network has no such species
        if translation is not None:
            # checked before anything is built: the transcripts, the proteins and the free ribosome
            # are species of the stochastic table, so every refusal above holds for translation too
            if not isinstance(translation, TranslationModel):
                raise ValueError('translation must be a TranslationModel')
            if stochastic is None:
                raise ValueError('translation needs a colony with stochastic=StochasticModel(...): its transcripts, '
                                 'proteins and free ribosomes are species of that table')
            translation.bind(stochastic)         # ValueError: the table lacks a species
        if transcription is not None:
            # checked before anything is built, like translation: the transcripts, the factors and
            # the free RNAP are species of the stochastic table (translation= is not needed)
            if not isinstance(transcription, TranscriptionModel):
                raise ValueError('transcription must be a TranscriptionModel')
            if stochastic is None:
                raise ValueError('transcription needs a colony with stochastic=StochasticModel(...): its transcripts, '
                                 'factors and free RNA polymerases are species of that table')
            transcription.bind(stochastic)       # ValueError: the table lacks a species
        if degradation is not None:
            # checked before anything is built: the transcripts and the enzymes are rows of the
            # stochastic table, and the nucleotides return to transcription's pools
            if not isinstance(degradation, DegradationModel):
                raise ValueError('degradation must be a DegradationModel')
            if stochastic is None or transcription is None:
                raise ValueError('degradation needs a colony with stochastic=StochasticModel(...) and '
                                 'transcription=TranscriptionModel(...): its transcripts and enzymes are rows of that '
                                 'table, and the nucleotide pools are transcription\'s')
            degradation.bind(stochastic, transcription)      # ValueError: the table lacks a species
        tree = None
        if cells is not None and cells.weighted:
            # checked before anything is built: TreeMass folds rows of the stochastic table
            if stochastic is None:
                raise ValueError('a CellModel with molecular_weights needs a colony with '
                                 'stochastic=StochasticModel(...): the weighted rows are rows of that table')
            tree = cells.bind(stochastic)        # ValueError: a name that is no row of the table
        if mechanics is not None:
            # checked before anything is built, like motility: the contact launch moves and
            # re-bins the agents on the device, on one whole plane
            if not isinstance(environment, Lattice):
                raise ValueError('mechanics needs a Lattice environment (capsules move on its plane)')
            if not whole_plane(environment):
                raise ValueError('mechanics needs a whole, unbanded plane (row bands are not supported)')
            if motility is not None:
                raise ValueError('mechanics with motility is not supported (two writers of position and heading)')
            if cells is not None and float(cells.width) != mechanics.width:
                raise ValueError('mechanics: the ContactModel\'s width (%r) must equal the CellModel\'s (%r)' % (
                    mechanics.width, cells.width))
            if mechanics.channels is not None:
                mechanics.check_channels(environment.bounds)     # ValueError: channels that do not fit the plane
        self.config = config
        self.table = table or compile_rate_laws(config['reactions'], config['kinetic_parameters'])
        self.response = response
        self._resp_layout = None
        if response is not None:
            # checked before anything is built: the response needs a field to exchange with,
            # and the agents stay where the contact launch or division puts them
            if not isinstance(response, CellResponse):
                raise ValueError('response must be a CellResponse')
            if environment == 'held':
                raise ValueError('response: a held environment has no field for the membrane to exchange with '
                                 '(use nonspatial or a Lattice)')
            if motility is not None:
                raise ValueError('response with motility is not supported')
            if isinstance(environment, Lattice):
                if not whole_plane(environment):
                    raise ValueError('response needs a whole, unbanded plane (row bands are not supported)')
                for mol in (response.membrane or {}).get('molecules_to_diffuse', []):
                    if mol not in environment.molecules:
                        raise ValueError('response: the lattice has no %r plane for the membrane to exchange with '
                                         '(molecules: %s)' % (mol, environment.molecules))
            elif environment != 'nonspatial':
                raise ValueError('environment must be held, nonspatial or a Lattice')
            self._resp_layout = response.bind(self.table)     # ValueError: a key that resolves to no row
        self.device = native.resolve_device(device)
        # lattice colonies: optionally run kinetics + gather on a side stream
        # beside the diffusion passes (step()); results are identical either way.
        # Off by default: on one MI355X the C4 stencil passes already fill the
        # chip, and the overlap measured 2.1003 -> 2.1001 ms per step (r01k)
        self.overlap_kinetics = False
        self._side_stream = torch.cuda.Stream(self.device) if self.device.type == 'cuda' else None
        # banded lattices: the first halo exchange of a step runs on a comm stream
        # beside the kinetics and the gather (it writes only halo rows)
        self.overlap_halo = True
        # lattice colonies stored in bin order: the gather and the exchange can ride on
        # the first and final diffusion passes (vk_diffuse_coupled; same results).  Off
        # by default: on one MI355X at C4 the coupled step ran 1.533 ms against 1.511
        # with the separate launches (profiles/r04/r04h/couple_ab.log)
        self.fuse_coupling = False
        # lattice colonies on the specialised agent-per-lane DP45 kernel: the gather of
        # the next step's local environment rides on the kinetics launch
        # (vk_step_dopri5_gather; the same values as vk_gather right after it)
        self.fuse_gather = True
        self._couple = None
        self.last_step_coupled = False
        self._comm_stream = torch.cuda.Stream(self.device) if self.device.type == 'cuda' else None
        self.engine = KineticsEngine(self.table, self.device)
        if specialize and integrator == 'dopri5':
            self.engine.specialize()     # straight-line rate laws (hiprtc), bit-identical results
        self.n = int(n_agents)
        self.ld = int(capacity or n_agents)
        if self.n > self.ld:
            raise ValueError('capacity < n_agents')
        self.integrator, self.rtol, self.atol, self.max_steps = integrator, rtol, atol, max_steps
        self.avogadro = avogadro
        self.exchange_mode = exchange
        t, ld, dev = self.table, self.ld, self.device
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
        self.params = torch.from_numpy(np.repeat(t.param_defaults[:, None], ld, axis=1)).to(dev).contiguous()
        conc0 = initial_conc(t, config.get('initial_state', {}), ld)
        if response is not None:
            # the response's own rows follow the table's n_species rows
            L = self._resp_layout
            conc0 = np.concatenate([conc0, np.zeros((L.n_rows - t.n_species, ld))], axis=0)
            for row, value in L.initial.items():
                conc0[row, :] = value
        self.conc = torch.from_numpy(conc0).to(dev).contiguous()
        self.m2c = torch.full((ld,), mmol_to_counts_from_mass(mass_fg, avogadro=avogadro),
                              dtype=torch.float64, device=dev)
        self.mass_fg = float(mass_fg)        # every agent's mass when there are no cells (colony_metrics)
        self.flux = z(t.n_reactions, ld)
        self.counts = z(t.n_ext, ld, dtype=torch.int64)
        self.status = z(ld, dtype=torch.int32)
        self.nsteps = z(ld, dtype=torch.int32)
        self.h_state = z(ld)
        self.time = 0.0
        self.step_index = 0
        self._layout = 0             # bumped when buffers are reallocated (Colony.capture checks it)
        self.lattice: Optional[Lattice] = None
        self.static: Optional[StaticField] = static
        self.router = None       # distributed.AgentRouter (row-banded multi-rank lattice colonies)
        self.cells = cells
        self.motility = motility
        self.mechanics = mechanics
        self.stochastic = stochastic
        if stochastic is not None:
            # the network on the device, the int counts and the key each agent draws by for
            # life (daughters get fresh ones); the engine's step word lives on the device
            self._ssa = StochasticEngine(stochastic, dev)
            self.ssa = torch.from_numpy(stochastic.initial_counts(self.n, ld)).to(dev).contiguous()
            self.ssa_key = torch.arange(ld, dtype=torch.int64, device=dev)
            self._ssa_key_base = self.n
        self.translation = translation
        if translation is not None:
            # the ribosome lists (empty), their lengths and the monomer pools (zero until
            # set_translation_molecules); the draws go by ssa_key and the ssa engine's step word
            self._tl = TranslationEngine(translation, stochastic, dev)
            self.ribosome_slots = z(translation.max_ribosomes, ld, dtype=torch.int32)
            self.ribosome_count = z(ld, dtype=torch.int32)
            self.tl_molecules = z(len(translation.molecule_ids), ld, dtype=torch.int32)
        self.transcription = transcription
        if transcription is not None:
            # the RNAP lists (empty), their lengths and the nucleotide pools (zero until
            # set_transcription_molecules); the draws go by ssa_key and the ssa engine's step word
            self._tx = TranscriptionEngine(transcription, stochastic, dev)
            self.rnap_slots = z(transcription.max_rnaps, ld, dtype=torch.int32)
            self.rnap_count = z(ld, dtype=torch.int32)
            self.tx_molecules = z(len(transcription.molecule_ids), ld, dtype=torch.int32)
        self.degradation = degradation
        if degradation is not None:
            # the carry of every transcript: 0, as the reference's partial_transcripts start
            self._deg = DegradationEngine(degradation, stochastic, transcription, dev)
            self.deg_partial = z(degradation.n_transcripts, ld)
        if response is not None:
            self.dead = z(ld, dtype=torch.int32)
            self.frozen = z(ld, dtype=torch.int32)
            # DeriveGlobals' volume of mass_fg (fL), every agent's when there are no cells
            volume_fl = CellModel(initial_mass=mass_fg).derive(mass_fg)[0]
            self._resp = ResponseEngine(self._resp_layout, dev, avogadro, volume_fl, t.n_reactions, t.n_ext)
        if cells is not None:
            if tree is not None:
                # TreeMass over the count table: the weighted rows (ascending) and their weights,
                # uploaded once; the initial deriver pass folds the initial counts
                self._tree = tree.upload(dev)
                rows, m2c = cells.initial_rows(ld, weighted=tree.pairs(stochastic.initial))
                if cells.model == 'tree_mass':
                    self.initial_mass = torch.full((ld,), float(cells.initial_mass), dtype=torch.float64, device=dev)
            else:
                rows, m2c = cells.initial_rows(ld)
            self.cell = torch.from_numpy(rows).to(dev).contiguous()
            self.m2c.copy_(torch.from_numpy(m2c))
            self.divide = z(ld, dtype=torch.int32)
            self.roots = [str(i) for i in range(self.n)] if agent_ids is None else [str(x) for x in agent_ids]
            if len(self.roots) != self.n:
                raise ValueError('agent_ids must name every agent')
            self.lin_root = torch.arange(ld, dtype=torch.int32, device=dev)
            self.lin_depth = z(ld, dtype=torch.int32)
            self.lin_path = z(ld, dtype=torch.int64)
            self._overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        self.environment = environment
        if isinstance(environment, (Lattice, StaticField)):
            if static is None:
                self.lattice = environment
            self._setup_maps(environment.molecules)
            if static is not None:
                # the deriver's update holds the gradient's molecules only: {molecule: conc row}
                self._static_rows = {m: t.species.index(('external', m)) for m in static.gradient_molecules
                                     if ('external', m) in t.species}
            self.location = z(2, ld)
            if motility is not None:
                self.motil = torch.from_numpy(motility.initial_rows(self.n, ld)).to(dev).contiguous()
                # global inner-update index of the next motility launch (the Philox counter
                # word): on the device, advanced by each launch, so graphs replay it
                self._motil_counter = z(1, dtype=torch.int64)
                if motility.flagella is not None:
                    # the multi-flagellar motor's state: FP64 rows, and count / count / mask
                    flag, flag_int = motility.flagella.initial_rows(self.n, ld, motility.seed)
                    self.flag = torch.from_numpy(flag).to(dev).contiguous()
                    self.flag_int = torch.from_numpy(flag_int).to(dev).contiguous()
                if cells is not None:
                    # one heading: the cell's angle is the swimming direction, so daughters
                    # are placed along it (vk_divide_locations); and a key per agent for the
                    # motility draws that she keeps for life, whoever divides around her
                    self.cell[native.VK_CELL_ANGLE, :self.n] = self.motil[native.VK_MOTIL_ANGLE, :self.n]
                    self.motile_key = torch.arange(ld, dtype=torch.int64, device=dev)
                    self._key_base = self.n
                if motility.flagella is not None and motility.flagella.expression is not None:
                    # the flagella count follows the expressed protein (ODE_expression + its
                    # counts deriver); the derivers run once at t = 0
                    fm = motility.flagella
                    self.flag_expr = torch.from_numpy(np.ascontiguousarray(
                        np.repeat(fm.expression_initial[:, None], ld, axis=1))).to(dev).contiguous()
                    self._flag_expression = ExpressionEngine(fm.expression_table, dev)
                    self._flag_flags = z(1, dtype=torch.int32)
                    self._flagella_counts()
                if complexes is not None:
                    # the flagella count follows the stochastic network's complex; once at t = 0
                    self._flag_flags = z(1, dtype=torch.int32)
                    self._ssa_flagella()
            if mechanics is not None and cells is None:
                self.mech_angle = torch.from_numpy(mechanics.initial_angles(self.n, ld)).to(dev).contiguous()
        elif environment == 'nonspatial':
            mols = []
            extra = self._resp_layout.molecules if response is not None else []
            for e in t.external_ids + [k[1] for k in t.species if k[0] == 'external'] + extra:
                if e not in mols:
                    mols.append(e)
            self._setup_maps(mols)
            self.env_molecules = mols
            self.env_fields = torch.ones((len(mols), ld), dtype=torch.float64, device=dev)
            depth_um = env_volume_L * 1e15                     # V / (1 um * 1 um)
            bin_volume = (depth_um * 1.0 * 1.0) * 1e-15 / 1    # get_bin_volume([1,1],[1,1],depth)
            self.env_binvol_avogadro = bin_volume * avogadro
        elif environment != 'held':
            raise ValueError('environment must be held, nonspatial, a Lattice or a StaticField')
        self._capacity_scratch()
        if self.env_fields is not None:
            self._env_to_external()          # derivers run once at t = 0
        if static is not None:
            self._static_refresh()           # derivers run once at t = 0
        if response is not None and self.lattice is not None and exchange == 'sorted':
            # the occupancy of the initial bins (set_agents(location=...) rebuilds it)
            lat = self.lattice
            self._occ_dev.sort(self.bin_lin, self.n, lat.rows_local * lat.ny, None)

    def _capacity_scratch(self):
        """Everything sized by the capacity that is not per-agent state (CAPACITY_SCRATCH and
        the buffer objects), for the current ``ld``: the only place that allocates it.  Called
        by the constructor and by population.install whenever ``ld`` changes; captured graphs
        hold the old buffers, so ``_layout`` moves."""
        ld, dev, lat = self.ld, self.device, self.lattice
        i32 = lambda: torch.zeros(ld, dtype=torch.int32, device=dev)
        if lat is not None or getattr(self, 'static', None) is not None:   # a borrowed hook: see stochastic below
            self.bin_lin, self.bin_ix = i32(), i32()
        if lat is not None:
            if self.motility is not None or self.mechanics is not None or self.response is not None:
                # these colonies exchange in agent order through an occupancy built on the device
                self._occ_dev = DeviceOccupancy(ld, dev)
        if self.env_fields is not None:
            self.env_bins = torch.arange(ld, dtype=torch.int32, device=dev)     # agent a owns bin a
        if self.mechanics is not None:
            # the contact launch's scratch; its counter and flag word are not per agent and carry over
            gx, gy = self.mechanics.grid(lat.bounds)
            old = getattr(self, '_mech', None)
            self._mech = ContactBuffers(ld, gx * gy, dev)
            if old is not None:
                self._mech.counter.copy_(old.counter)
                self._mech.flags.copy_(old.flags)
            if self.mechanics.channels is not None:
                # the mother machine's outflow flags: written by every contact launch, read at
                # the end of the step
                self.outflow = i32()
        if self.response is not None:
            self._resp_buf = ResponseBuffers(self._resp_layout, ld, self.table.n_reactions, dev,
                                             self.cells is not None)
        if self._flag_expression is not None:
            self._flag_expr_update = torch.zeros((len(self._flag_expression.table.outputs), ld),
                                                 dtype=torch.float64, device=dev)
        for stage in STOCHASTIC_STAGES:
            if getattr(self, stage.engine, None) is not None:   # objects that only borrow this hook lack it
                # what each agent fired (initiated, lost) in the last step; the status bits are sticky
                # and checked before the capacity changes (population.install), so nothing is lost here
                setattr(self, stage.events, i32())
                setattr(self, stage.status, i32())
        # sized by ld too, allocated by their users (capture(overlap=True), step_many, colony_metrics)
        self._counts_alt = self.flux_steps = self.counts_steps = self.nsteps_steps = None
        self._colony_shape = None
        self._layout += 1

    # -- maps between SoA rows and field planes ---------------------------------
    def _setup_maps(self, molecules):
        t = self.table
        gf, gr, xc, xf = [], [], [], []
        for f, mol in enumerate(molecules):
            key = ('external', mol)
            if key in t.species:
                gf.append(f)
                gr.append(t.species.index(key))
        for e, mol in enumerate(t.external_ids):
            if mol in molecules:
                xc.append(e)
                xf.append(molecules.index(mol))
        i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=self.device)
        if self.response is not None:
            # the membrane reads the agent's ('external', m) row and writes float counts
            # into m's plane, whether or not a rate law mentions the molecule
            L, fc, ff = self._resp_layout, [], []
            for m, mol in enumerate(L.molecules):
                f, row = molecules.index(mol), int(L.mol_ext_row[m])
                if row not in gr:
                    gf.append(f)
                    gr.append(row)
                fc.append(m)
                ff.append(f)
            self.map_fexch_count, self.map_fexch_field = i32(fc), i32(ff)
        self.map_gather_field, self.map_gather_row = i32(gf), i32(gr)
        self.map_exch_count, self.map_exch_field = i32(xc), i32(xf)

    # -- state I/O ----------------------------------------------------------------
    def set_agents(self, params=None, conc=None, mmol_to_counts=None, location=None, environment=None):
        """Upload per-agent arrays ([rows, n] numpy or torch; columns 0..n-1).
        ``environment`` ([molecules, n], a nonspatial colony): each agent's own field,
        copied into its external rows as the derivers do."""
        def put(dst, src):
            src = torch.as_tensor(src, dtype=dst.dtype)
            if src.dim() == 1:
                dst[:self.n].copy_(src[:self.n].to(self.device))
            else:
                dst[:, :self.n].copy_(src[:, :self.n].to(self.device))
        if params is not None:
            put(self.params, params)
        if conc is not None:
            put(self.conc, conc)
        if mmol_to_counts is not None:
            put(self.m2c, mmol_to_counts)
        if environment is not None:
            if self.env_fields is None:
                raise ValueError('environment values need a nonspatial colony')
            put(self.env_fields, environment)
            self._env_to_external()
        if location is not None:
            if self.lattice is None and self.static is None:
                raise ValueError('locations need a lattice or a static field environment')
            put(self.location, location)
            if self.static is not None:
                self._static_refresh()
            else:
                self.refresh_bins()

    def set_flagella(self, counts):
        """The flagella count each agent is to have (the reference's ``internal_counts``
        ``flagella``): an int for every agent, or one value per agent column [0, n) as a
        host array or a device int32 tensor.  The next inner update grows or removes
        flagella to match.  The values are copied into the existing ``flag_int`` row, so a
        captured graph sees them at its next replay.  Host values outside 0..32 raise; a
        device tensor is not read back, and the kernel clamps what it finds."""
        if self.motility is None or self.motility.flagella is None:
            raise ValueError('set_flagella: a colony with motility=MotilityModel(flagella=FlagellaModel(...))')
        if self.motility.flagella.expression is not None:
            raise ValueError('set_flagella: the count is derived from the expressed protein every step '
                             '(FlagellaModel(expression=...)) and would be overwritten')
        if self.motility.flagella.complexes is not None:
            raise ValueError('set_flagella: the count follows the stochastic network\'s complex every step '
                             '(FlagellaModel(complexes=...)) and would be overwritten')
        row = self.flag_int[native.VK_FLAGI_TARGET, :self.n]
        if torch.is_tensor(counts) and counts.device.type == self.device.type and self.device.type != 'cpu':
            if counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] < self.n:
                raise ValueError('set_flagella: a device tensor must be int32 over agents [0, n)')
            row.copy_(counts[:self.n])
            return
        c = check_flagella_counts(counts.cpu().numpy() if torch.is_tensor(counts) else counts)
        if c.ndim == 0:
            row.fill_(int(c))
        else:
            if c.shape[0] < self.n:
                raise ValueError('set_flagella: one count per agent (%d < %d)' % (c.shape[0], self.n))
            row.copy_(torch.from_numpy(c[:self.n].astype(np.int32)))

    # -- the polymerase lists and pools: one implementation behind the six public methods ----------
    def _polymerase_model(self, pol, what):
        model = getattr(self, pol.model)
        if model is None:
            raise ValueError('%s: a colony with %s=%sModel(...)' % (what, pol.model, pol.model.capitalize()))
        return model

    def _lists(self, pol, what):
        self._polymerase_model(pol, what)
        slots = getattr(self, pol.slots)[:, :self.n].cpu().numpy()
        count = getattr(self, pol.count)[:self.n].cpu().numpy()
        return [[pol.unpack(w) for w in slots[:count[a], a]] for a in range(self.n)]

    def _set_lists(self, pol, what, lists):
        model = self._polymerase_model(pol, what)
        if len(lists) != self.n:
            raise ValueError('%s: one list per agent (%d != %d)' % (what, len(lists), self.n))
        slots = np.zeros((getattr(model, pol.max_slots), self.n), dtype=np.int32)
        count = np.zeros(self.n, dtype=np.int32)
        for a, entries in enumerate(lists):
            words = getattr(model, pol.check)(list(entries))
            slots[:len(words), a], count[a] = words, len(words)
        getattr(self, pol.slots)[:, :self.n].copy_(torch.from_numpy(slots))
        getattr(self, pol.count)[:self.n].copy_(torch.from_numpy(count))

    def _set_molecules(self, pol, what, counts):
        ids = self._polymerase_model(pol, what).molecule_ids
        for name, value in counts.items():
            if name not in ids:
                raise ValueError('%s: no molecule %r (molecules: %s)' % (what, name, ids))
            v = np.asarray(value)
            if v.ndim and v.shape[0] < self.n:
                raise ValueError('%s: one count per agent (%d < %d)' % (what, v.shape[0], self.n))
            v = np.broadcast_to(v[:self.n] if v.ndim else v, (self.n,)).astype(np.int64)
            if np.any(v < -2 ** 31) or np.any(v > 2 ** 31 - 1):
                raise ValueError('%s: the count of %r does not fit int32' % (what, name))
            getattr(self, pol.molecules)[ids.index(name), :self.n].copy_(torch.from_numpy(v.astype(np.int32)))

    def ribosomes(self):
        """Host copy of the ribosome lists: per agent a list of (template, position, occluding)
        in insertion order; ``template`` indexes the model's ``transcript_order``."""
        return self._lists(RIBOSOME, 'ribosomes')

    def set_ribosomes(self, lists):
        """The ribosome list of every agent [0, n): per agent a sequence of (template, position,
        occluding).  Copied into the existing arrays, so a captured graph sees them at its next
        replay.  A list longer than ``max_ribosomes`` or a ribosome outside its template raises."""
        self._set_lists(RIBOSOME, 'set_ribosomes', lists)

    def set_translation_molecules(self, **counts):
        """Monomer, ATP and ADP counts by name: an int for every agent or one value per agent
        [0, n).  Copied into the existing ``tl_molecules`` rows."""
        self._set_molecules(RIBOSOME, 'set_translation_molecules', counts)

    def rnaps(self):
        """Host copy of the RNAP lists: per agent a list of (template, terminator, position,
        occluding) in insertion order; ``template`` indexes the model's ``promoter_order``."""
        return self._lists(RNAP, 'rnaps')

    def set_rnaps(self, lists):
        """The RNAP list of every agent [0, n): per agent a sequence of (template, terminator,
        position, occluding).  Copied into the existing arrays, so a captured graph sees them at
        its next replay.  A list longer than ``max_rnaps`` or an RNAP outside its template raises."""
        self._set_lists(RNAP, 'set_rnaps', lists)

    def set_transcription_molecules(self, **counts):
        """Nucleotide, ATP and ADP counts by name: an int for every agent or one value per agent
        [0, n).  Copied into the existing ``tx_molecules`` rows."""
        self._set_molecules(RNAP, 'set_transcription_molecules', counts)

    def agent_array_names(self):
        """Every per-agent array this colony has (agent = column), as attribute names in
        the order of AGENT_ARRAYS: what division gathers and the router migrates."""
        return [name for name, _ in _ALL_AGENT_ARRAYS if torch.is_tensor(getattr(self, name, None))]

    def refresh_bins(self):
        """Recompute bin sites and the agent-ordered bin occupancy (after moves).
        A row-banded colony with a router first moves agents that left this
        rank's band to their owner (a collective: every rank calls it)."""
        lat = self.lattice
        if self.router is not None:
            self.router.route()
        lat.bin_sites(self.location, self.n, self.bin_lin, self.bin_ix)
        ix = self.bin_ix[:self.n]
        if self.n and (int(ix.min()) < lat.row_lo_global or int(ix.max()) >= lat.row_hi_global):
            raise ValueError('agents outside this rank\'s row band: attach a distributed.AgentRouter '
                             '(division moves daughters across band edges)')
        self.occ = occupancy(self.bin_lin, self.n, self.agent_order)
        if self.response is not None and self.exchange_mode == 'sorted':
            # a response colony exchanges through the device occupancy: one ordered kernel
            self._occ_dev.sort(self.bin_lin, self.n, lat.rows_local * lat.ny, self.agent_order)
        self._update_coupling()
        self._layout += 1            # captured graphs hold the old occupancy buffers

    def _update_coupling(self):
        """The segment index of the coupled passes (vk_diffuse_coupled), kept only
        while the agents are stored in bin order on a whole, unbanded plane and
        each plane gathers into / takes counts from at most one SoA row."""
        self._couple = None
        lat, n = self.lattice, self.n
        if lat is None or self.cells is not None or self.router is not None or n == 0:
            return
        if self.motility is not None or self.mechanics is not None:
            return      # agents leave bin order every step: the separate launches
        if self.response is not None:
            return      # the mixed exchange is its own launch
        if not whole_plane(lat):
            return
        # stored in bin order, and within a bin in the exchange's agent order
        # (occupancy: agent_order after sort_by_bin, else the column order)
        b = self.bin_lin[:n].to(torch.int64)
        key = self.agent_order
        if n > 1:
            same = b[1:] == b[:-1]
            ok = (b[1:] > b[:-1]) | (same & (key[1:n] > key[:n - 1]) if key is not None else same)
            if not bool(ok.all()):
                return
        nf = len(lat.molecules)
        rows = []
        for fields, srcs in ((self.map_gather_field, self.map_gather_row), (self.map_exch_field, self.map_exch_count)):
            r = [-1] * nf
            for f, x in zip(fields.tolist(), srcs.tolist()):
                if r[f] != -1:
                    return
                r[f] = x
            rows.append(r)
        self._couple = (segment_index(self.bin_lin, n, lat.rows_local, lat.ny), rows[0], rows[1])

    def sort_by_bin(self):
        """Store the agents in bin order, so that the exchange scatter and the
        gather read the per-agent arrays and the lattice as streams instead of
        scattered lines.  The sort key is (bin, reference order): agents sharing
        a bin stay in the reference's relative order, and the exchange
        occupancy keeps ordering each bin by ``self.agent_order`` after later
        moves (refresh_bins), so every result is unchanged -- the exchange adds
        a bin's agents in the reference's agent order, and agents do not
        interact otherwise.  ``self.agent_order[k]`` is the index (in the
        layout before the first sort) of the agent now stored in column k.
        Sort again after agents move to keep the streams.  Colonies whose agent
        order is itself a result -- division appends daughters in mother order,
        a row band's router keeps the single-rank order -- keep their layout."""
        if self.lattice is None:
            raise ValueError('sort_by_bin: a lattice colony')
        if self.cells is not None or self.router is not None:
            raise ValueError('sort_by_bin: division and routed bands keep the reference agent order')
        n = self.n
        prev = self.agent_order
        key = prev if prev is not None else torch.arange(n, dtype=torch.int64, device=self.device)
        by_key = torch.sort(key[:n], stable=True).indices
        perm = by_key[torch.sort(self.bin_lin[:n].to(torch.int64)[by_key], stable=True).indices]
        # every column of the capacity: the permuted agents, then the unused ones as they are
        columns = torch.cat([perm, torch.arange(n, self.ld, device=self.device)])
        new = {name: getattr(self, name).index_select(-1, columns) for name in self.agent_array_names()}
        new['agent_order'] = key[perm]
        install(self, new, n)
        self.refresh_bins()          # the bins are a function of the location: the same values, permuted
        return self.agent_order

    def _gather_fused(self):
        """Whether this step's kinetics launch also does the gather."""
        return (self.fuse_gather and self.lattice is not None and self.integrator == 'dopri5' and
                self.response is None and self.engine.default_variant() == 2 and 0 < self.map_gather_field.numel() <= 8)

    def kinetics_and_gather(self, dt: float):
        """kinetics(dt) then gather_external(), as one launch when the kernel allows."""
        if not self._gather_fused():
            self.kinetics(dt)
            self.gather_external()
            return
        lat = self.lattice
        self.engine.dopri5_gather(dt, self.params, self.conc, self.m2c, self.n, self.h_state, self.rtol, self.atol,
                                  self.max_steps, self.flux, self.counts, self.status, self.nsteps, lat.fields,
                                  lat.field_stride, self.bin_lin, self.map_gather_field, self.map_gather_row)
        if self.attempts is not None:
            self.attempts += self.nsteps[:self.n].sum()

    def gather_external(self):
        """external := field at the agent's bin (get_local_environments)."""
        self.lattice.gather(self.bin_lin, self.n, self.map_gather_field, self.map_gather_row, self.conc)

    def _static_gather(self):
        """external := the static field at the agent's own position (StaticField.next_update)."""
        self.static.gather(self.location, self.n, self.conc, self._static_rows)

    def _static_refresh(self):
        """The bins and the externals of the current positions: what the derivers leave at
        t = 0 and after positions were set.  Buffers stay, captured graphs stay valid."""
        sf = self.static
        native.check(native._lib.vk_bin_sites(
            native.ptr(self.location), self.n, self.ld, sf.n_bins[0], sf.n_bins[1], sf.bounds[0], sf.bounds[1], 0,
            native.ptr(self.bin_lin), native.ptr(self.bin_ix), native.stream_handle()), 'vk_bin_sites')
        self._static_gather()

    def _env_to_external(self):
        if self.map_gather_field.numel():
            native.check(native._lib.vk_gather(
                native.ptr(self.env_fields), self.ld, native.ptr(self.env_bins), self.n,
                native.ptr(self.map_gather_field), native.ptr(self.map_gather_row),
                int(self.map_gather_field.numel()), native.ptr(self.conc), self.ld,
                native.stream_handle()), 'vk_gather')

    # -- one timestep -------------------------------------------------------------
    def count_attempts(self, on: bool = True):
        """Accumulate DP45 attempts (accepted + rejected steps) of every agent
        into ``self.attempts`` (device int64), summed right after the kinetics
        launch -- before division copies a mother's ``nsteps`` into both
        daughters (bench flop accounting)."""
        self.attempts = torch.zeros((), dtype=torch.int64, device=self.device) if on else None

    def _kin_conc(self):
        """The kinetics' view of ``conc``: the table's rows (a response colony keeps its
        own rows after them, in the same allocation)."""
        return self.conc if self.response is None else self.conc[:self.table.n_species]

    def kinetics(self, dt: float):
        if self.integrator == 'euler':
            self.engine.euler(dt, self.params, self._kin_conc(), self.m2c, self.n, self.flux, self.counts,
                              self.status)
        else:
            self.engine.dopri5(dt, self.params, self._kin_conc(), self.m2c, self.n, self.h_state, self.rtol,
                               self.atol, self.max_steps, self.flux, self.counts, self.status,
                               self.nsteps)
            if self.attempts is not None:
                self.attempts += self.nsteps[:self.n].sum()

    def _step_buffers(self, k):
        t, ld = self.table, self.ld
        if self.flux_steps is None or self.flux_steps.shape[0] != k:
            self.flux_steps = torch.zeros((k, t.n_reactions, ld), dtype=torch.float64, device=self.device)
            self.counts_steps = torch.zeros((k, t.n_ext, ld), dtype=torch.int64, device=self.device)
            self.nsteps_steps = torch.zeros((k, ld), dtype=torch.int32, device=self.device)
            self._layout += 1

    def step_many(self, dt: float = 1.0, steps: int = 1):
        """``steps`` timesteps of a colony whose agents do not couple between
        steps (environment 'held', no cells, DP45 with the specialised kernel)
        in ONE launch (vk_step_dopri5_multi): each step equals :meth:`step`
        bit for bit.  Every step's fluxes, exchange counts and attempts stay in
        ``flux_steps`` [steps, R, ld], ``counts_steps`` [steps, E, ld] and
        ``nsteps_steps`` [steps, ld]; ``flux`` / ``counts`` / ``nsteps`` view
        the last step's."""
        if self.response is not None:
            raise ValueError('step_many: a colony with a response steps with step()')
        if self.stochastic is not None:
            raise ValueError('step_many: a colony with stochastic kinetics steps with step()')
        if self.environment != 'held' or self.cells is not None or self.integrator != 'dopri5':
            raise ValueError('step_many: held externals, no division, DP45 (agents must not couple between steps)')
        k = int(steps)
        self._step_buffers(k)
        self.engine.dopri5_multi(dt, k, self.params, self.conc, self.m2c, self.n, self.h_state, self.rtol,
                                 self.atol, self.max_steps, self.flux_steps, self.counts_steps, self.status,
                                 self.nsteps_steps)
        self.flux, self.counts, self.nsteps = self.flux_steps[k - 1], self.counts_steps[k - 1], self.nsteps_steps[k - 1]
        if self.attempts is not None:
            self.attempts += self.nsteps_steps[:, :self.n].sum()
        self.time += dt * k
        self.step_index += k

    def step(self, dt: float = 1.0, halo_exchange=None, allreduce=None, timing=None, stamp=None):
        """One timestep.  ``timing`` (optional) = {'kin': (ev0, ev1), 'diff': (ev0, ev1)}
        of torch.cuda.Events recorded on the launch stream around those kernels.
        ``stamp`` (optional, a callable of 0 / 1 / 2) writes a device timestamp
        on the launch stream before the kinetics, after it, and at the end of
        the step (bench instrumentation that also works inside a captured graph)."""
        timing = {k: v for k, v in (timing or {}).items() if v is not None}
        if stamp is not None:
            stamp(0)
        if self.motility is not None:
            self._motility_step(dt)
        if self.mechanics is not None:
            self._mechanics_step()
        if self.response is not None:
            if self.router is not None or halo_exchange is not None:
                raise ValueError('a colony with a response takes no router and no row bands')
            if self.overlap_kinetics or self.fuse_coupling:
                raise ValueError('a colony with a response runs its launches in order on one stream '
                                 '(overlap_kinetics and fuse_coupling are not available)')
            self._response_begin(dt)
        if self.lattice is not None and self.overlap_kinetics:
            # kinetics + gather read only the pre-step field and agent state, so
            # they run on a side stream beside the diffusion passes; the pass
            # that overwrites the field waits for the gather, the exchange for
            # the counts (both through one event)
            lat, main = self.lattice, torch.cuda.current_stream(self.device)
            side = self._side_stream
            side.wait_stream(main)                       # previous step's writers
            with torch.cuda.stream(side):
                if 'kin' in timing:
                    timing['kin'][0].record()
                self.kinetics_and_gather(dt)             # + the pre-step field (one-step lag)
                if 'kin' in timing:
                    timing['kin'][1].record()
                done = torch.cuda.Event()
                done.record()
            lat.diffuse(dt, halo_exchange=halo_exchange, allreduce=allreduce,
                        events=timing.get('diff'), before_final=lambda: main.wait_event(done))
            self._step_exchange()
            self._finish_step(dt)
            return
        halo_done = None
        if (self.lattice is not None and halo_exchange is not None and self.overlap_halo and
                self._comm_stream is not None and (self.lattice.pad_top or self.lattice.pad_bot)):
            halo_done = self.lattice.exchange_first_halo(dt, halo_exchange, self._comm_stream)
        if 'kin' in timing:
            timing['kin'][0].record()
        coupled = (self.lattice is not None and halo_done is None and halo_exchange is None and
                   self.fuse_coupling and self._couple is not None and self.exchange_mode == 'sorted' and
                   self.lattice.coupled_plan_ok(dt))
        fused = self.lattice is not None and not coupled and self._gather_fused()
        if fused:
            self.kinetics_and_gather(dt)                     # + the pre-step field (one-step lag)
        else:
            self.kinetics(dt)
        if self.response is not None:
            self._response_end()
        if 'kin' in timing:
            timing['kin'][1].record()
        if stamp is not None:
            stamp(1)
        if self.lattice is not None:
            lat = self.lattice
            if not (halo_done is None and halo_exchange is None and self._coupled_step(dt, allreduce, timing)):
                if not fused:
                    self.gather_external()                   # pre-step field (one-step lag)
                # with the first halo exchange in flight, the band's interior passes run
                # first and the launch stream waits for the halo before the edge passes
                lat.diffuse(dt, halo_exchange=halo_exchange, allreduce=allreduce,
                            events=timing.get('diff'), halo_event=halo_done)
                self._step_exchange()
        elif self.environment == 'nonspatial':
            if self.map_exch_count.numel():
                native.check(native._lib.vk_exchange_atomic(
                    native.ptr(self.env_fields), self.ld, native.ptr(self.env_bins), self.n,
                    native.ptr(self.counts), self.ld, native.ptr(self.map_exch_count),
                    native.ptr(self.map_exch_field), int(self.map_exch_count.numel()),
                    self.env_binvol_avogadro, native.stream_handle()), 'vk_exchange_atomic')
            if self.response is not None and self.map_fexch_count.numel():
                # each agent owns its bin: (field + int counts) + float counts, exactly
                native.check(native._lib.vk_exchange_atomic_f64(
                    native.ptr(self.env_fields), self.ld, native.ptr(self.env_bins), self.n,
                    native.ptr(self._resp_buf.fcounts), self.ld, native.ptr(self.map_fexch_count),
                    native.ptr(self.map_fexch_field), int(self.map_fexch_count.numel()),
                    self.env_binvol_avogadro, native.stream_handle()), 'vk_exchange_atomic_f64')
            self._env_to_external()
        elif self.static is not None:
            # the field deriver, after the move and the kinetics: the next step's kinetics reads
            # the field where this step left the agent.  Exchange counts are computed and
            # dropped, as with 'held': the reference's static lattice has no field store
            self._static_gather()
        self._finish_step(dt)
        if stamp is not None:
            stamp(2)

    # -- multi-rate advance (Experiment.update, experiment.py:1351-1450) -------------
    def run(self, interval: float, kinetics_dt: float = 1.0, diffusion_dt: float = 1.0, halo_exchange=None,
            allreduce=None):
        """Advance a lattice colony by ``interval`` with the kinetics and the
        diffusion field on their own clocks (each agent's kinetics process's
        ``time_step``, the DiffusionField's ``time_step``), scheduled as the
        reference's Experiment.update does: a process runs when its front time
        <= time, with timestep = min(front + dt, interval) - front, and computes
        its update from the state at that moment; the global step is the
        smallest timestep that ran; updates whose front lands by then are
        applied in store order -- the environment's (fields += delta, every
        agent's external := the field at its bin when the diffusion ran)
        before the agents' (internal += delta or := the DP45 end state,
        fluxes, exchange into the field at apply time, in agent order).
        ``run(dt, dt, dt)`` equals :meth:`step` (dt) bit for bit.  A row-banded
        colony passes ``halo_exchange`` / ``allreduce`` as to :meth:`step`.
        Cells (growth / division) step with :meth:`step`."""
        if self.static is not None:
            raise ValueError('run() schedules a diffusing lattice; a colony in a StaticField steps with step() '
                             '(its field deriver runs on the step clock)')
        if self.lattice is None:
            raise ValueError('run() schedules a lattice colony; use step() otherwise')
        if self.cells is not None:
            raise ValueError('growth and division run with step(): their derivers fix one clock')
        if self.motility is not None:
            raise ValueError('a motile colony steps with step(): the move runs on the step clock')
        if self.mechanics is not None:
            raise ValueError('a colony with mechanics steps with step(): the contacts run on the step clock')
        if self.response is not None:
            raise ValueError('a colony with a response steps with step(): its processes share the step clock')
        if self.stochastic is not None:
            raise ValueError('a colony with stochastic kinetics steps with step(): its step runs on the step clock')
        procs = [('diffusion', float(diffusion_dt)), ('kinetics', float(kinetics_dt))]   # store order
        front = {name: 0.0 for name, _ in procs}      # every update() call starts its fronts at 0
        pending = {}
        time = 0.0
        while time < interval:
            full_step = float('inf')
            for name, dt in procs:
                f = front[name]
                if f <= time:
                    future = min(f + dt, interval)
                    timestep = future - f
                    pending[name] = self._compute(name, timestep, halo_exchange, allreduce)
                    full_step = min(full_step, timestep)
                    front[name] = future
            future = time + full_step
            for name, _ in procs:
                if front[name] <= future and name in pending:
                    self._apply(name, pending.pop(name))
            time = future
            self.time += full_step
        self.step_index += 1
        return self

    def _compute(self, name, timestep, halo_exchange=None, allreduce=None):
        """A process's update from the current state, not yet applied."""
        lat, t = self.lattice, self.table
        if name == 'diffusion':
            delta = lat.diffuse_delta(timestep, allreduce=allreduce, halo_exchange=halo_exchange)
            ext = torch.empty((t.n_species, self.ld), dtype=torch.float64, device=self.device)
            lat.gather(self.bin_lin, self.n, self.map_gather_field, self.map_gather_row, ext)
            return delta, ext
        nd = t.n_dyn
        flux = torch.empty_like(self.flux)
        counts = torch.empty_like(self.counts)
        if self.integrator == 'euler':
            delta = torch.zeros((nd, self.ld), dtype=torch.float64, device=self.device)
            self.engine.euler(timestep, self.params, self.conc, self.m2c, self.n, flux, counts, self.status,
                              delta=delta)
            return 'delta', delta, flux, counts
        end = self.conc.clone()
        self.engine.dopri5(timestep, self.params, end, self.m2c, self.n, self.h_state, self.rtol, self.atol,
                           self.max_steps, flux, counts, self.status, self.nsteps)
        return 'set', end[:nd], flux, counts

    def _apply(self, name, update):
        lat, t = self.lattice, self.table
        n = self.n
        if name == 'diffusion':
            delta, ext = update
            own = slice(lat.row_lo, lat.row_hi)         # the accumulate updater: field + delta
            lat.fields[:, own] += delta[:, own]
            rows = self.map_gather_row.to(torch.int64)
            self.conc[rows, :n] = ext[rows, :n]         # external: set
            return
        mode, value, flux, counts = update
        nd = t.n_dyn
        if mode == 'delta':
            self.conc[:nd, :n] += value[:, :n]          # internal: accumulate
        else:
            self.conc[:nd, :n] = value[:, :n]
        self.flux.copy_(flux)
        self.counts.copy_(counts)
        self._step_exchange()

    def _coupled_step(self, dt, allreduce, timing):
        """gather + diffusion + exchange as one coupled pass sequence, when the
        colony and the plan allow it (vk_diffuse_coupled); False: nothing ran."""
        cp, lat = self._couple, self.lattice
        self.last_step_coupled = False
        if (cp is None or not self.fuse_coupling or self.exchange_mode != 'sorted' or
                not lat.coupled_plan_ok(dt)):
            return False
        seg, grow, crow = cp
        self.last_step_coupled = lat.diffuse_coupled(dt, self.bin_lin, self.n, seg, grow, self.conc, crow,
                                                     self.counts, allreduce=allreduce, events=timing.get('diff'))
        return self.last_step_coupled

    def _motility_step(self, dt):
        """First in a motile colony's step: sense the pre-step ligand plane, receptor,
        motor, move (vk_motility_step; bins come out of the kernel), then the device
        occupancy of the new bins for the ordered exchange.  No host read and no
        re-layout: ``_layout`` stays, captured graphs stay valid.  In a StaticField the
        ligand is its gradient at the agent's position (the _static launches), and there is
        no exchange to order."""
        if self.router is not None:
            raise ValueError('a motile colony takes no router')
        field = self.lattice if self.static is None else self.static
        # a dividing colony draws by the agent's own key; its column order is the reference's
        # agent order, which the occupancy below keeps (key None)
        key = self.motile_key if self.cells is not None else self.agent_order
        if self.motility.flagella is not None:
            flagella_step(self.motility, field, self.location, self.motil, self.flag, self.flag_int, self.n,
                          dt, self._motil_counter, key=key, bin_lin=self.bin_lin, bin_ix=self.bin_ix)
        else:
            motility_step(self.motility, field, self.location, self.motil, self.n, dt, self._motil_counter,
                          key=key, bin_lin=self.bin_lin, bin_ix=self.bin_ix)
        if self.cells is not None:
            # one heading: a device row copy in stream order
            self.cell[native.VK_CELL_ANGLE, :self.n].copy_(self.motil[native.VK_MOTIL_ANGLE, :self.n])
        if self.static is None and self.exchange_mode == 'sorted' and self.map_exch_count.numel():
            lat = self.lattice
            self._occ_dev.sort(self.bin_lin, self.n, lat.rows_local * lat.ny, self.agent_order)

    def _mechanics_step(self):
        """First in the step of a colony with mechanics: the contact relaxation
        (vk_contact_step; bins come out of it), then the device occupancy of the new
        bins for the ordered exchange.  No host read and no re-layout: ``_layout``
        stays, captured graphs stay valid."""
        if self.router is not None:
            raise ValueError('a colony with mechanics takes no router')
        if self.cells is not None:
            angle, length = self.cell[native.VK_CELL_ANGLE], self.cell[native.VK_CELL_LENGTH]
        else:
            angle, length = self.mech_angle, None
        key = self.agent_order
        contact_step(self.mechanics, self.lattice, self.location, angle, self.n, self._mech, length=length,
                     key=key, bin_lin=self.bin_lin, bin_ix=self.bin_ix,
                     outflow=self.outflow if self.mechanics.channels is not None else None)
        if self.exchange_mode == 'sorted' and (self.map_exch_count.numel() or self.response is not None):
            lat = self.lattice
            self._occ_dev.sort(self.bin_lin, self.n, lat.rows_local * lat.ny, key)

    def colony_metrics(self, link_gap: float = 0.5, min_cells: int = 3):
        """Which cells form a colony, and each colony's cell count, mass, cell area,
        centroid, angle and axes (lens_amd/colonies.py: this engine's own definition,
        standing where the reference's ColonyShapeDeriver emits ``colony_global``).
        For colonies with ``mechanics=``: width and max_length are the ContactModel's,
        angle and length come from where the contact launch takes them, mass from the
        cells' mass row (``cells=``) or the colony's ``mass_fg``, the key is
        ``agent_order``.  Returns a :class:`~lens_amd.colonies.ColonyMetrics` (a host
        read).  The buffers are made on first use and dropped when the capacity
        changes; a colony that never calls this launches nothing for it."""
        if self.mechanics is None:
            raise ValueError('colony_metrics needs a colony with mechanics= (the capsules\' width and max_length)')
        shape = self._colony_shape
        if shape is None or (shape.model.link_gap, shape.model.min_cells) != (float(link_gap), int(min_cells)):
            model = ColonyShapeModel(link_gap=link_gap, min_cells=min_cells, max_length=self.mechanics.max_length,
                                     width=self.mechanics.width)
            shape = self._colony_shape = ColonyShape(model, self.lattice.bounds, self.ld, self.device,
                                                     length=self.mechanics.length, mass=self.mass_fg)
        if self.cells is not None:
            angle, length = self.cell[native.VK_CELL_ANGLE], self.cell[native.VK_CELL_LENGTH]
            mass = self.cell[native.VK_CELL_MASS]
        else:
            angle, length, mass = self.mech_angle, None, None
        shape.launch(self.n, self.location, angle, length=length, mass=mass, key=self.agent_order)
        return shape.result()

    # -- the antibiotic response (lens_amd/response.py) ----------------------------
    def _response_begin(self, dt):
        """Before the kinetics launch, all from the step-start state: the detector, the
        membrane terms, the frozen agents' saved columns, the expression update."""
        volume = self.cell[native.VK_CELL_VOLUME] if self.cells is not None else None
        self._resp.begin(dt, self.n, self.conc, volume, self.frozen, self._resp_buf, self.flux, self.status,
                         self.nsteps)

    def _response_end(self):
        """After the kinetics launch: frozen agents get their columns back, live ones the
        expression update, every agent the membrane delta; dying agents freeze."""
        self._resp.end(self.n, self.conc, self.frozen, self.dead, self._resp_buf, self.flux, self.status,
                       self.nsteps, self.counts)

    def _step_exchange(self):
        lat = self.lattice
        if self.response is not None:
            fc = self._resp_buf.fcounts
            if self.exchange_mode == 'sorted':
                lat.exchange_ordered_mixed(self._occ_dev.order, self._occ_dev.sorted_bin, self.n, self.counts,
                                           self.map_exch_count, self.map_exch_field, fc, self.map_fexch_count,
                                           self.map_fexch_field)
            else:
                if self.map_exch_count.numel():
                    lat.exchange_atomic(self.bin_lin, self.n, self.counts, self.map_exch_count, self.map_exch_field)
                lat.exchange_atomic_f64(self.bin_lin, self.n, fc, self.map_fexch_count, self.map_fexch_field)
            return
        if self.map_exch_count.numel():
            if (self.motility is not None or self.mechanics is not None) and self.exchange_mode == 'sorted':
                lat.exchange_ordered(self._occ_dev.order, self._occ_dev.sorted_bin, self.n, self.counts,
                                     self.map_exch_count, self.map_exch_field)
            elif self.exchange_mode == 'sorted':
                lat.exchange_sorted(self.occ, self.counts, self.map_exch_count, self.map_exch_field)
            else:
                lat.exchange_atomic(self.bin_lin, self.n, self.counts, self.map_exch_count,
                                    self.map_exch_field)

    def _overlap_ok(self):
        """Whether :meth:`capture` can overlap a step's exchange with the next step's
        kinetics (and the uniform probe with the gather)."""
        lat = self.lattice
        return (lat is not None and self.cells is None and not self.overlap_kinetics and not self.fuse_coupling
                and self.device.type == 'cuda' and not (lat.pad_top or lat.pad_bot))

    def _captured_steps_overlapped(self, dt, steps, stamps):
        """The body of an overlapped capture (see :meth:`capture`).  Step k's exchange
        scatter reads the counts buffer its own kinetics wrote, and runs on a side stream
        while step k+1's kinetics writes the other buffer; the uniform probe runs on a
        second side stream beside the gather.  Every read of the planes (probe, gather,
        passes) waits for the previous exchange, so each step sees exactly the state a
        sequential step would."""
        lat = self.lattice
        if self._x_stream is None:
            self._x_stream = torch.cuda.Stream(self.device)
            self._p_stream = torch.cuda.Stream(self.device)
        sx, sp = self._x_stream, self._p_stream
        bufs = (self.counts, self._counts_alt)
        pending = None
        for k in range(steps):
            stamp = None
            if stamps is not None:
                stamp = (lambda tag, k=k: native.check(native._lib.vk_timestamp(
                    native.ptr(stamps), 3 * k + tag, native.stream_handle()), 'vk_timestamp'))
                stamp(0)
            self.counts = bufs[(steps - 1 - k) % 2]   # the last step writes the colony's own buffer
            self.kinetics(dt)
            if stamp is not None:
                stamp(1)
            main = torch.cuda.current_stream(self.device)
            if pending is not None:
                main.wait_event(pending)             # the previous step's exchange landed
            sp.wait_stream(main)
            with torch.cuda.stream(sp):
                mm = lat.uniform_summary(None)       # the probe, beside the gather
            self.gather_external()                   # pre-step field (one-step lag)
            main.wait_stream(sp)
            lat.diffuse(dt, summary=mm)
            sx.wait_stream(main)
            with torch.cuda.stream(sx):
                self._step_exchange()                # this step's counts buffer
                pending = torch.cuda.Event()
                pending.record()
            self._finish_step(dt)
            if stamp is not None:
                stamp(2)
        torch.cuda.current_stream(self.device).wait_event(pending)

    def capture(self, dt: float = 1.0, steps: int = 1, stamps=None, steps_per_launch: int = 1, overlap=False):
        """Capture ``steps`` timesteps into one HIP graph (torch.cuda.CUDAGraph)
        and return a function that replays them.

        A small colony's step is a few short launches, and issuing them from
        Python costs more than running them (C2: 40 µs per step issued, 4.5 µs
        replayed). Replaying a captured graph leaves the host out of the loop.
        Only steps that take no host decision can be captured: no division (the
        host reads back the new agent count), no row band (its halo exchange
        is a host-driven collective), no NonSpatialEnvironment. A single-GPU
        lattice step qualifies (with ``overlap_kinetics`` too: the side stream
        forks from and joins the captured stream inside each step): the pass plan
        depends only on Δt, and the uniform-plane skip is read by the kernels
        from device memory. Capture records the launches without running them,
        so the colony state is unchanged until the first replay. The graph
        holds the buffers and the agent count of capture time: set_agents()
        values may change between replays (they are copied in place), but a
        re-binning of moved agents invalidates it (replay raises).  A motile
        colony (``motility=``) moves and re-bins its agents inside the graph:
        each replay continues the walk (the Philox counter lives on the device).
        So does a colony with ``mechanics=`` and no cells.
        ``steps_per_launch`` > 1 (a held colony without division) captures
        :meth:`step_many` launches of that many steps instead.
        ``stamps`` (optional, a device int64 tensor of 3 * steps) records each
        replayed step's segment boundaries (:meth:`step`'s ``stamp``) at
        [3k, 3k + 1, 3k + 2] -- vk_timestamp ticks, vk_wall_clock_khz per ms.
        ``overlap`` (a single-GPU lattice colony without division): within the graph,
        step k's exchange scatter runs on a side stream beside step k+1's kinetics (the
        two alternate between two counts buffers), and the uniform probe beside the
        gather.  The results are the sequential steps' bit for bit, and ``counts`` holds
        the last replayed step's counts.  Off by default: at C4 the overlapped kernels
        slow each other and each cross-stream dependency adds ~6 us, 1.518 against
        1.515 ms per step (profiles/r04/r04k)."""
        if self._channels():
            raise ValueError('Colony.capture: a colony with channels removes its outflow on the host every step '
                             '(the agent count changes) and cannot be replayed from one graph')
        lat = self.lattice
        if self.cells is not None or self.environment == 'nonspatial' or (lat is not None and not whole_plane(lat)):
            raise ValueError('Colony.capture: division, row bands and NonSpatialEnvironment take host decisions '
                             'per step and cannot be replayed from one graph (a row band: capture_banded)')
        if steps < 1:
            raise ValueError('Colony.capture: steps >= 1')
        spl = int(steps_per_launch)
        if spl > 1 and (stamps is not None or steps % spl):
            raise ValueError('Colony.capture: steps_per_launch must divide steps (and takes no stamps)')
        if spl > 1 and self.response is not None:
            raise ValueError('Colony.capture: steps_per_launch is not available for a colony with a response')
        if spl > 1:
            self._step_buffers(spl)                 # allocated before the capture (graphs hold the pointers)
        if overlap and self.motility is not None:
            raise ValueError('Colony.capture: overlap is not available for a motile colony')
        if overlap and self.mechanics is not None:
            raise ValueError('Colony.capture: overlap is not available for a colony with mechanics')
        if overlap and self.response is not None:
            raise ValueError('Colony.capture: overlap is not available for a colony with a response')
        overlap = bool(overlap) and self._overlap_ok() and spl == 1
        if overlap and (self._counts_alt is None or self._counts_alt.shape != self.counts.shape):
            self._counts_alt = torch.zeros_like(self.counts)
        counts0 = self.counts
        for stage in STOCHASTIC_STAGES:
            if stage.polymerase is not None and getattr(self, stage.engine) is not None:
                getattr(self, stage.engine).plan(dt)    # the sub-interval plan is uploaded before the capture
        graph = torch.cuda.CUDAGraph()
        t0, s0 = self.time, self.step_index
        layout, n = self._layout, self.n
        with torch.cuda.graph(graph):
            for k in range(steps // spl if spl > 1 else 0):
                self.step_many(dt, spl)
            if overlap:
                self._captured_steps_overlapped(dt, steps, stamps)
            for k in range(steps if spl == 1 and not overlap else 0):
                stamp = None
                if stamps is not None:
                    stamp = (lambda tag, k=k: native.check(native._lib.vk_timestamp(
                        native.ptr(stamps), 3 * k + tag, native.stream_handle()), 'vk_timestamp'))
                self.step(dt, stamp=stamp)
        self.time, self.step_index = t0, s0      # capture ran nothing
        if spl > 1:
            # step_many pointed flux / counts / nsteps at the last step's rows of the
            # step buffers, which is where every replay leaves them
            self.flux, self.counts, self.nsteps = (self.flux_steps[spl - 1], self.counts_steps[spl - 1],
                                                   self.nsteps_steps[spl - 1])
        else:
            self.counts = counts0

        def replay():
            # the graph holds raw device pointers and the agent count of capture time
            if self._layout != layout or self.n != n:
                raise RuntimeError('Colony.capture: the colony was re-laid out (agents moved or counted '
                                   'anew) after capture; capture again')
            graph.replay()
            self.time += dt * steps
            self.step_index += steps

        replay.graph = graph      # keep the graph (and its memory pool) alive with the replayer
        replay.stamps = stamps
        return replay

    def capture_banded(self, dt: float = 1.0, halo_exchange=None, allreduce=None):
        """Row-banded lattice colony (multi-GPU): capture each step's launch
        sequences between its collectives as HIP graphs and return a function
        that runs one step -- the collectives (halo exchange, the uniform-plane
        all-reduce) are issued eagerly, everything else is replayed.

        One step of :meth:`step` on a band is, in stream order: kinetics and the
        gather (while the first halo exchange runs on the communication
        stream), the uniform-plane probe, its all-reduce, then per halo block a
        halo exchange (the first one already done) and the block's fused
        passes, and the exchange scatter after the last block.  The segments
        between the collectives become graphs: [kinetics + gather + probe],
        then one graph per halo block (the last with the scatter).  The
        kernels and their arguments are the eager step's, so the results are
        bit-identical (tests/test_distributed_gpu.py).  As with :meth:`capture`,
        re-binned agents invalidate the graphs."""
        from lens_amd.lattice import n_substeps
        lat = self.lattice
        if lat is None or not (lat.pad_top or lat.pad_bot):
            raise ValueError('Colony.capture_banded: a row-banded lattice colony (use capture() otherwise)')
        if self.cells is not None or self.overlap_kinetics:
            raise ValueError('Colony.capture_banded: division and side-stream overlap take host decisions per step')
        if halo_exchange is None:
            raise ValueError('Colony.capture_banded: a row band needs its halo_exchange callback')
        n_sub = n_substeps(dt, lat.diffusion_dt)
        coeff_dt = lat.diffusion * min(dt, lat.diffusion_dt)
        lo_min = lat.row_lo if lat.edge_top else 0
        hi_max = lat.row_hi if lat.edge_bot else lat.rows_local
        blocks, j = [], 0
        while j < n_sub:
            cnt = min(lat.halo, n_sub - j)
            blocks.append((j, cnt))
            j += cnt
        layout, n = self._layout, self.n
        t0, s0 = self.time, self.step_index
        g_kin = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_kin):
            self.kinetics_and_gather(dt)                 # + the pre-step field (one-step lag)
            lat.uniform_summary(None)                    # the probe; its all-reduce is eager
        # the first block's interior needs no halo: it is its own graph, replayed while
        # the first halo exchange is in flight; the block's edges follow the halo
        # the overlap decision is taken once, here: g_blocks[0] holds only the edge
        # strips when the interior is split off, so step() must not re-read
        # self.overlap_halo / self._comm_stream (a later toggle would drop the interior)
        comm = self._comm_stream if self.overlap_halo else None
        g_interior = None
        if comm is not None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                j0, c0 = blocks[0]
                split = lat._run_part(j0, c0, n_sub, coeff_dt, lat.uniform, lo_min, hi_max, native.VK_PART_INTERIOR)
            g_interior = g if split else None
        g_blocks = []
        for b, (j, cnt) in enumerate(blocks):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                if b == 0 and g_interior is not None:
                    lat._run_part(j, cnt, n_sub, coeff_dt, lat.uniform, lo_min, hi_max, native.VK_PART_EDGES)
                else:
                    lat._run_block(j, cnt, n_sub, coeff_dt, lat.uniform, lo_min, hi_max)
                if b == len(blocks) - 1:
                    self._step_exchange()
            g_blocks.append(g)
        self.time, self.step_index = t0, s0             # capture ran nothing

        def step():
            if self._layout != layout or self.n != n:
                raise RuntimeError('Colony.capture_banded: the colony was re-laid out after capture; capture again')
            main = torch.cuda.current_stream(self.device)
            halo_done = None
            if comm is not None:
                halo_done = lat.exchange_first_halo(dt, halo_exchange, comm)
            g_kin.replay()
            if allreduce is not None:
                allreduce(lat.uniform)
            if halo_done is not None:
                if g_interior is not None:
                    g_interior.replay()                  # beside the halo exchange
                main.wait_event(halo_done)
            else:
                halo_exchange(lat.state_buffer(0), blocks[0][1])
            for b, (j, cnt) in enumerate(blocks):
                if b:
                    halo_exchange(lat.state_buffer(j), cnt)
                g_blocks[b].replay()
            self.time += dt
            self.step_index += 1

        step.graphs = (g_kin, g_blocks)
        step.interior_graph = g_interior
        return step

    def _flagella_counts(self):
        """The counts deriver of the flagella protein (derive_counts.py:42-51): ``target``
        from the current concentration and the current mmol_to_counts."""
        fm = self.motility.flagella
        native.check(native._lib.vk_flagella_counts(
            self.n, self.flag_expr.data_ptr() + fm.count_row * self.ld * 8, native.ptr(self.m2c),
            self.flag_int.data_ptr() + native.VK_FLAGI_TARGET * self.ld * 4, native.ptr(self._flag_flags),
            native.stream_handle()), 'vk_flagella_counts')

    def _flagella_check(self):
        """Raises if a derived flagella count ever left 0..32 (one host read: called where
        the host reads from the device anyway)."""
        if self._flag_flags is not None and int(self._flag_flags.item()):
            raise FloatingPointError('a derived flagella count left 0..32 (concentration * mmol_to_counts was '
                                     'negative, not a number or 33 and more): the motor holds 32 flagella')

    def _ssa_complex(self):
        """The species whose count is the flagella count (FlagellaModel(complexes=...)), or None."""
        m = self.motility
        return m.flagella.complexes if m is not None and m.flagella is not None else None

    def _ssa_flagella(self):
        """target := the agent's count of the flagella complex, 0..32 (vk_ssa_flagella_target)."""
        row = self.stochastic.index(self._ssa_complex())
        flagella_target(self.n, self.ssa[row], self.flag_int[native.VK_FLAGI_TARGET], self._flag_flags)

    def _ssa_check(self):
        """Raises if a stochastic step ever set a status bit (one host read: called where the
        host reads from the device anyway, and by check_status)."""
        if self._ssa is None:
            return
        for stage in _REPORT_ORDER:
            if getattr(self, stage.engine) is None:
                continue
            st = getattr(self, stage.status)[:self.n]
            bad = torch.nonzero(st).flatten()
            if bad.numel():
                a = int(bad[0])
                raise FloatingPointError('agent %d: %s step status %d (%s)' % (
                    a, stage.label, int(st[a]), stage.describe(int(st[a]))))

    def _finish_step(self, dt):
        if self._flag_expression is not None:
            # the expression process from the step-start state (ode_expression.py:265-303), then
            # its counts deriver -- in front of DeriveGlobals (core/process.py:75-103), so with
            # the mmol_to_counts the previous step left; both before vk_cell_step touches m2c
            self._flag_expression.step(dt, self.flag_expr, self.n, update=self._flag_expr_update, accumulate=True)
            self._flagella_counts()
        if self._tx is not None:
            # transcription in front of translation, editing the ssa counts in place: the ribosomes
            # below see the transcripts this step finished (the sequential order is this engine's).
            # The factor levels are counts / mmol_to_counts with the m2c the previous step left
            # (vk_cell_step below has not touched it yet, as _flagella_counts reads it)
            self._tx.step(dt, self.rnap_slots, self.rnap_count, self.tx_molecules, self.ssa, self.m2c, self.ssa_key,
                          self.n, events=self.tx_events, status=self._tx_status,
                          step_counter=self._ssa.step_counter, advance=False)
        if self._tl is not None:
            # translation first, editing the ssa counts in place: the network below then sees the
            # proteins this step completed (the sequential order is this engine's; the reference
            # applies both processes' updates to the step-start state).  It draws under the step
            # word the ssa launch advances, and under a domain of its own
            self._tl.step(dt, self.ribosome_slots, self.ribosome_count, self.tl_molecules, self.ssa, self.ssa_key,
                          self.n, events=self.tl_events, status=self._tl_status,
                          step_counter=self._ssa.step_counter, advance=False)
        if self._deg is not None:
            # degradation after translation and before the network, in the compartment's process
            # order (the sequential order is this engine's, as above): the transcripts lose what the
            # endoRNAses degrade, the nucleotides return to transcription's pools.  The levels are
            # counts / mmol_to_counts with the m2c the previous step left, as transcription's
            self._deg.step(dt, self.ssa, self.deg_partial, self.tx_molecules, self.m2c, self.n,
                           degraded=self.deg_degraded, status=self._deg_status)
        if self._ssa is not None:
            # the stochastic network over the step, every agent on her own clock and by her own
            # key; then the flagella count the NEXT step's motor reads (the reference's
            # FlagellaActivity sees the counts the previous step left).  Before division, which
            # splits the post-step counts
            self._ssa.step(dt, self.ssa, self.ssa_key, self.n, events=self.ssa_events, status=self._ssa_status)
            if self._ssa_complex() is not None:
                self._ssa_flagella()
        if self.cells is not None:
            self.grow_and_divide(dt)
        elif self._channels():
            self.remove(self.outflow)    # the mother machine's outflow (with cells: planned with division)
        self.time += dt
        self.step_index += 1

    def set_cell_mass(self, mass):
        """Per-agent masses (fg) for agents 0..n-1 with their derived volume,
        length, surface area and mmol_to_counts (DeriveGlobals on each).  In the
        ``'tree_mass'`` model the values are the agents' ``initial_mass``: the mass row is
        TreeMass of them over the current counts, by the host's fold."""
        cm = self.cells
        mass = np.ascontiguousarray(mass, dtype=np.float64)[:self.n]
        if cm.model == 'tree_mass':
            if mass.shape != (self.n,):
                raise ValueError('set_cell_mass: one initial mass per agent')
            self.initial_mass[:self.n].copy_(torch.from_numpy(mass))
            counts = self.ssa[:, :self.n].cpu().numpy()
            mass = np.ascontiguousarray(cm.tree_mass(None, self._tree.pairs(counts), mass))     # elementwise
        vol, m2c, length, area = cm.derive(mass)          # numpy: the same IEEE ops elementwise
        rows = self.cell[:, :self.n].cpu().numpy()
        rows[native.VK_CELL_MASS], rows[native.VK_CELL_VOLUME] = mass, vol
        rows[native.VK_CELL_LENGTH], rows[native.VK_CELL_SURFACE_AREA] = length, area
        self.cell[:, :self.n].copy_(torch.from_numpy(rows))
        self.m2c[:self.n].copy_(torch.from_numpy(np.ascontiguousarray(m2c)))

    # -- growth, derivers, division (a10-a13) ------------------------------------
    def grow_and_divide(self, dt: float):
        """Growth process + TreeMass/DeriveGlobals, then division.  Returns the
        number of mothers that divided."""
        cm, n = self.cells, self.n
        if n == 0 and self.router is None:
            return 0
        if n:
            p = cm.vk_params(dt, self.step_index)
            u = None
            if cm.model == 'growth_protein' and cm.rng == 'stream':
                u = torch.from_numpy(cm.host_uniforms(n)).to(self.device)
            if self.response is not None:
                # an agent frozen before this step neither grows nor raises its division flag
                self._resp.cells(False, n, self.frozen, self.cell, self.m2c, self.divide, self._resp_buf)
            if self._tree is not None:
                # TreeMass folds the weighted rows of the counts this step left (the network,
                # translation, transcription and degradation above have run)
                native.check(cell_step_tree(p, n, self.ld, self.cell, self.m2c, u, self.lin_root, self.lin_depth,
                                            self.lin_path, self.divide, self.ssa, self._tree, self.initial_mass),
                             'vk_cell_step_tree')
            else:
                native.check(native._lib.vk_cell_step(
                    ctypes.byref(p), n, self.ld, native.ptr(self.cell), native.ptr(self.m2c), native.ptr(u),
                    native.ptr(self.lin_root), native.ptr(self.lin_depth), native.ptr(self.lin_path),
                    native.ptr(self.divide), native.stream_handle()), 'vk_cell_step')
            if self.response is not None:
                self._resp.cells(True, n, self.frozen, self.cell, self.m2c, self.divide, self._resp_buf)
        # the mother machine: the agents the contact launch flagged leave with this plan, and a
        # flagged mother leaves no daughters.  One host read either way; the flags the host
        # checks ride on it (the contact launch's too-long flag, the flagella count flag)
        plan = plan_population(n, self.divide, self.outflow if self._channels() else None, self.device)
        if n and self.mechanics is not None:
            self._mech.check()
        if n and self.motility is not None:
            self._flagella_check()
        if self.router is not None:
            # collective every step, also with no agents: the global order of every rank's
            # survivors and daughters (AgentRouter.division_ordinals); then, if any rank
            # divided, daughters that left this band move to their owner
            new_ord, n_div = self.router.division_ordinals(self.ordinal[:n], self.divide[:n] != 0, plan.src,
                                                           plan.kind, plan.n_out)
            if plan.n_out != n:
                regather(self, dataclasses.replace(plan, ordinal=new_ord))
            elif n_div:
                self.ordinal[:n] = new_ord
                self.refresh_bins()
        elif plan.n_out != n or plan.n_removed:
            regather(self, plan)
        return plan.n_daughters // 2

    def _channels(self):
        """Whether this colony is a mother machine (mechanics with channels)."""
        return self.mechanics is not None and self.mechanics.channels is not None

    def remove(self, mask):
        """Take the agents a with ``mask[a] != 0`` out of the colony (``mask``: a device
        int32 or bool tensor over agents [0, n)).  The others keep their order; every
        per-agent array is gathered once into the same capacity (vk_population_plan with
        no divide flags, then vk_divide_gather with the set divider), and bins and
        occupancies are rebuilt as after a division.  Returns the number removed (one
        host read).  ``col.remove(col.dead[:col.n] != 0)`` drops a response colony's dead."""
        lat = self.lattice
        if self.router is not None or (lat is not None and not whole_plane(lat)):
            raise ValueError('Colony.remove: a colony with a router or a banded lattice keeps its agents '
                             '(their global order lives on other ranks)')
        n, dev = self.n, self.device
        if not torch.is_tensor(mask) or mask.device.type != dev.type or mask.dim() != 1 or mask.shape[0] < n or \
                mask.dtype not in (torch.int32, torch.bool):
            raise ValueError('Colony.remove: mask must be a device int32 or bool tensor over agents [0, n)')
        plan = plan_population(n, None, mask[:n].to(torch.int32).contiguous(), dev)
        if plan.n_removed:
            regather(self, plan, declared=False)
        return plan.n_removed

    def agent_ids(self):
        """Phylogeny ids of agents 0..n-1 (meta_division.py:15-18)."""
        if self.cells is None:
            return [str(a) for a in range(self.n)]
        return lineage_ids(self.roots, self.lin_root[:self.n].cpu().numpy(),
                           self.lin_depth[:self.n].cpu().numpy(), self.lin_path[:self.n].cpu().numpy())

    def check_status(self):
        st = self.status[:self.n]
        bad = torch.nonzero(st).flatten()
        if bad.numel():
            a = int(bad[0])
            raise FloatingPointError('agent %d: kernel status %d' % (a, int(st[a])))
        if self.mechanics is not None:
            self._mech.check()
        if self.motility is not None:
            self._flagella_check()
        self._ssa_check()

    # -- views ----------------------------------------------------------------------
    def species(self, port, name):
        return self.conc[self.table.species.index((port, name)), :self.n]

    def snapshot(self):
        """Host copy of the emitted state ({port: {state: ndarray[n]}})."""
        out = {}
        c = self.conc[:, :self.n].cpu().numpy()
        keys = self.table.species if self.response is None else self._resp_layout.keys
        for s, (port, name) in enumerate(keys):
            out.setdefault(port, {})[name] = c[s].copy()
        if self.response is not None:
            # counts deriver (derive_counts.py:42-51) on the expression's states, post-step
            m2c = self.m2c[:self.n].cpu().numpy()
            out['cell_counts'] = {keys[r][1]: np.trunc(c[r] * m2c) for r in self._resp_layout.expr_rows.tolist()}
        f = self.flux[:, :self.n].cpu().numpy()
        out['fluxes'] = {rid: f[r].copy() for r, rid in enumerate(self.table.reaction_ids)}
        if self.cells is not None:
            c = self.cell[:, :self.n].cpu().numpy()
            out['global'] = {name: c[row].copy() for name, row in (
                ('mass', native.VK_CELL_MASS), ('volume', native.VK_CELL_VOLUME),
                ('length', native.VK_CELL_LENGTH), ('surface_area', native.VK_CELL_SURFACE_AREA),
                ('angle', native.VK_CELL_ANGLE))}
            out['global']['width'] = np.full(self.n, self.cells.width)
            out['global']['mmol_to_counts'] = self.m2c[:self.n].cpu().numpy().copy()
            out.setdefault('internal', {})['protein'] = c[native.VK_CELL_PROTEIN].copy()
        if self.motility is not None:
            m = self.motil[:, :self.n].cpu().numpy()
            out['motility'] = {name: m[row].copy() for row, name in enumerate(MOTIL_ROW_NAMES)}
            if self.motility.flagella is not None:
                f = self.flag[:, :self.n].cpu().numpy()
                fi = self.flag_int[:, :self.n].cpu().numpy()
                out['flagella'] = {name: f[row].copy() for row, name in enumerate(FLAG_ROW_NAMES)}
                out['flagella'].update({name: fi[row].copy() for row, name in enumerate(FLAGI_ROW_NAMES)})
                out['flagella']['mask'] = out['flagella']['mask'].view(np.uint32)     # bit i: flagellum i is CW
                if self._flag_expression is not None:
                    e = self.flag_expr[:, :self.n].cpu().numpy()
                    out['flagella_expression'] = {name: e[row].copy() for row, name in
                                                  enumerate(self.motility.flagella.expression_names)}
            if self.cells is not None:
                out['motile_key'] = self.motile_key[:self.n].cpu().numpy().copy()
        if self.mechanics is not None:
            angle = self.cell[native.VK_CELL_ANGLE] if self.cells is not None else self.mech_angle
            out['mechanics'] = {'angle': angle[:self.n].cpu().numpy().copy(),
                                'location': self.location[:, :self.n].cpu().numpy().copy()}
        if self.response is not None:
            out.setdefault('global', {})['dead'] = self.dead[:self.n].cpu().numpy().copy()
        if self.stochastic is not None:
            x = self.ssa[:, :self.n].cpu().numpy()
            out['stochastic'] = {name: x[row].copy() for row, name in enumerate(self.stochastic.rows)}
            out['ssa_key'] = self.ssa_key[:self.n].cpu().numpy().copy()
            out['ssa_events'] = self.ssa_events[:self.n].cpu().numpy().copy()
        for stage in _POLYMERASE_STAGES:
            pol = stage.polymerase
            if getattr(self, pol.model) is None:
                continue
            m = getattr(self, pol.molecules)[:, :self.n].cpu().numpy()
            out[pol.model + '_molecules'] = {name: m[row].copy() for row, name in
                                             enumerate(getattr(self, pol.model).molecule_ids)}
            out[pol.count] = getattr(self, pol.count)[:self.n].cpu().numpy().copy()
            out[pol.model + '_events'] = getattr(self, stage.events)[:self.n].cpu().numpy().copy()
        if self.degradation is not None:
            out['degraded_transcripts'] = self.deg_degraded[:self.n].cpu().numpy().copy()
        return out


# the optional state the table of stages names: None on a colony that lacks the stage, like the
# class-level declarations above
for _stage in STOCHASTIC_STAGES:
    for _name in stage_attributes(_stage):
        setattr(Colony, _name, None)
