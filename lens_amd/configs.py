"""Network configurations and synthetic colony generators.

The dictionaries are in the reference's ConvenienceKinetics configuration
schema (``reactions`` / ``kinetic_parameters`` / ``initial_state`` /
``ports``), so any reference config drops straight in.

* :func:`glc_lct_config` -- get_glc_lct_config (vivarium/processes/convenience_kinetics.py:448-524),
  the network the reference fixture convenience_kinetics.csv is produced with.
* :func:`glc_lct_transport_config` -- get_glc_lct_transport (:357-445).
* :func:`toy_config` -- get_toy_config (:527-571).
* :func:`glc_ac_config` -- glucose uptake + a synthetic acetate secretion
  (BASELINE configs 3-4; SURVEY.md §8d C3: no acetate reaction exists in
  the reference, so this one is ours, written in the reference schema).
* :func:`heterogeneous_colony` -- SURVEY.md §8d C2 distributions.
* :func:`synthetic_network` -- SURVEY.md §8d C5-style random network.
"""

from __future__ import annotations

import copy
import math

import numpy as np

SEED = 20261015


def glc_lct_config():
    reactions = {
        'EX_glc__D_e': {
            'stoichiometry': {
                ('internal', 'g6p_c'): 1.0,
                ('external', 'glc__D_e'): -1.0,
                ('internal', 'pep_c'): -1.0,
                ('internal', 'pyr_c'): 1.0,
            },
            'is reversible': False,
            'catalyzed by': [('internal', 'EIIglc')],
        },
        'EX_lcts_e': {
            'stoichiometry': {
                ('external', 'lcts_e'): -1.0,
                ('internal', 'lcts_p'): 1.0,
            },
            'is reversible': False,
            'catalyzed by': [('internal', 'LacY')],
        },
    }
    kinetics = {
        'EX_glc__D_e': {
            ('internal', 'EIIglc'): {
                ('external', 'glc__D_e'): 1e0,
                ('internal', 'pep_c'): None,
                'kcat_f': 6e1,
            }
        },
        'EX_lcts_e': {
            ('internal', 'LacY'): {
                ('external', 'lcts_e'): 1e0,
                'kcat_f': 6e1,
            }
        },
    }
    initial_state = {
        'internal': {
            'EIIglc': 1.8e-3, 'g6p_c': 0.0, 'pep_c': 1.8e-1,
            'pyr_c': 0.0, 'LacY': 0, 'lcts_p': 0.0,
        },
        'external': {'glc__D_e': 10.0, 'lcts_e': 10.0},
    }
    ports = {
        'internal': ['g6p_c', 'pep_c', 'pyr_c', 'EIIglc', 'LacY', 'lcts_p'],
        'external': ['glc__D_e', 'lcts_e'],
    }
    return {'reactions': reactions, 'kinetic_parameters': kinetics,
            'initial_state': initial_state, 'ports': ports}


def glc_lct_transport_config():
    reactions = {
        'LCTSt3ipp': {
            'stoichiometry': {
                ('internal', 'h_c'): 1.0, ('external', 'h_p'): -1.0,
                ('internal', 'lcts_c'): 1.0, ('external', 'lcts_p'): -1.0},
            'is reversible': False,
            'catalyzed by': [('internal', 'LacY')]},
        'GLCptspp': {
            'stoichiometry': {
                ('internal', 'g6p_c'): 1.0, ('external', 'glc__D_e'): -1.0,
                ('internal', 'pep_c'): -1.0, ('internal', 'pyr_c'): 1.0},
            'is reversible': False,
            'catalyzed by': [('internal', 'EIIglc')]},
        'GLCt2pp': {
            'stoichiometry': {
                ('internal', 'glc__D_c'): 1.0, ('external', 'glc__D_p'): -1.0,
                ('internal', 'h_c'): 1.0, ('external', 'h_p'): -1.0},
            'is reversible': False,
            'catalyzed by': [('internal', 'GalP')]},
    }
    kinetics = {
        'LCTSt3ipp': {('internal', 'LacY'): {
            ('external', 'h_p'): None, ('external', 'lcts_p'): 1e0, 'kcat_f': 7.8e2}},
        'GLCptspp': {('internal', 'EIIglc'): {
            ('external', 'glc__D_e'): 1e0, ('internal', 'pep_c'): 1e0, 'kcat_f': 7.5e4}},
        'GLCt2pp': {('internal', 'GalP'): {
            ('external', 'glc__D_p'): 1e0, ('external', 'h_p'): None, 'kcat_f': 1.5e2}},
    }
    initial_state = {
        'internal': {'EIIglc': 1.8e-3, 'g6p_c': 0.0, 'pep_c': 1.8e-1,
                     'pyr_c': 0.0, 'LacY': 0, 'lcts_p': 0.0},
        'external': {'glc__D_e': 10.0, 'lcts_e': 10.0},
    }
    return {'reactions': reactions, 'kinetic_parameters': kinetics,
            'initial_state': initial_state}


def toy_config():
    return {
        'reactions': {'reaction1': {
            'stoichiometry': {('internal', 'A'): 1, ('external', 'B'): -1},
            'is reversible': False,
            'catalyzed by': [('internal', 'enzyme1')]}},
        'kinetic_parameters': {'reaction1': {('internal', 'enzyme1'): {
            ('external', 'B'): 0.2, 'kcat_f': 5e1}}},
        'initial_state': {'internal': {'A': 1.0, 'enzyme1': 1e-1},
                          'external': {'B': 10.0}},
        'ports': {'internal': ['A', 'enzyme1'], 'external': ['B']},
    }


def glc_ac_config():
    """Glucose PTS uptake (glc_lct's EX_glc__D_e) + acetate overflow secretion."""
    cfg = glc_lct_config()
    reactions = {'EX_glc__D_e': cfg['reactions']['EX_glc__D_e']}
    kinetics = {'EX_glc__D_e': cfg['kinetic_parameters']['EX_glc__D_e']}
    reactions['EX_ac_e'] = {
        'stoichiometry': {('internal', 'g6p_c'): -1.0, ('external', 'ac_e'): 2.0},
        'is reversible': False,
        'catalyzed by': [('internal', 'AckA')],
    }
    kinetics['EX_ac_e'] = {('internal', 'AckA'): {('internal', 'g6p_c'): 5e-1, 'kcat_f': 2e1}}
    initial_state = {
        'internal': {'EIIglc': 1.8e-3, 'g6p_c': 0.0, 'pep_c': 1.8e-1, 'pyr_c': 0.0,
                     'AckA': 1.0e-3},
        'external': {'glc__D_e': 10.0, 'ac_e': 0.0},
    }
    return {'reactions': reactions, 'kinetic_parameters': kinetics,
            'initial_state': initial_state}


# ---------------------------------------------------------------------------
# colony generators (SoA numpy; the engine uploads them)
# ---------------------------------------------------------------------------

def initial_conc(table, initial_state, n_agents):
    """[n_species, n] float64 from a reference initial_state dict (missing -> 0)."""
    conc = np.zeros((table.n_species, n_agents), dtype=np.float64)
    for s, (port, name) in enumerate(table.species):
        conc[s, :] = float(initial_state.get(port, {}).get(name, 0.0))
    return conc


def heterogeneous_colony(table, config, n_agents, seed=SEED, sigma=0.25):
    """per-agent kcat/Km x lognormal(0, sigma); EIIglc ~ U(0.9,2.7)e-3,
    LacY ~ U(0, 2e-3); internal x U(0.5,1.5); glc__D_e ~ U(0.1,10), lcts_e ~ U(0,10)."""
    rng = np.random.default_rng(seed)
    params = np.repeat(table.param_defaults[:, None], n_agents, axis=1)
    params = params * rng.lognormal(0.0, sigma, size=params.shape)
    conc = initial_conc(table, config['initial_state'], n_agents)
    for s, (port, name) in enumerate(table.species):
        if port == 'external':
            continue
        conc[s] *= rng.uniform(0.5, 1.5, n_agents)
    draws = {
        ('internal', 'EIIglc'): lambda: rng.uniform(0.9e-3, 2.7e-3, n_agents),
        ('internal', 'LacY'): lambda: rng.uniform(0.0, 2e-3, n_agents),
        ('external', 'glc__D_e'): lambda: rng.uniform(0.1, 10.0, n_agents),
        ('external', 'lcts_e'): lambda: rng.uniform(0.0, 10.0, n_agents),
    }
    for key, draw in draws.items():
        if key in table.species:
            conc[table.species.index(key)] = draw()
    return np.ascontiguousarray(params), np.ascontiguousarray(conc)


def gaussian_bump_field(n_bins, base=10.0, amp=5.0, sigma_frac=0.125):
    nx, ny = n_bins
    x = (np.arange(nx) + 0.5)[:, None] - nx / 2
    y = (np.arange(ny) + 0.5)[None, :] - ny / 2
    sig = sigma_frac * min(nx, ny)
    return base + amp * np.exp(-(x * x + y * y) / (2 * sig * sig))


def synthetic_network(n_species=50, n_reactions=40, n_enzymes=10, seed=SEED,
                      n_external=4):
    """C5-style random network in the reference schema: irreversible reactions
    with 1-3 substrates and 1-2 products, Km log-U[1e-3, 1e1], kcat log-U[1e-1, 1e4]."""
    rng = np.random.default_rng(seed)
    internal = [('internal', 'm%02d' % i) for i in range(n_species - n_external)]
    external = [('external', 'x%02d' % i) for i in range(n_external)]
    mols = internal + external
    enzymes = [('internal', 'E%02d' % i) for i in range(n_enzymes)]
    reactions, kinetics = {}, {}
    for r in range(n_reactions):
        rid = 'R%03d' % r
        ns = int(rng.integers(1, 4))
        npd = int(rng.integers(1, 3))
        pick = rng.choice(len(mols), ns + npd, replace=False)
        subs = [mols[i] for i in pick[:ns]]
        prods = [mols[i] for i in pick[ns:]]
        st = {m: -float(rng.integers(1, 3)) for m in subs}
        st.update({m: float(rng.integers(1, 3)) for m in prods})
        enz = enzymes[int(rng.integers(0, n_enzymes))]
        reactions[rid] = {'stoichiometry': st, 'is reversible': False, 'catalyzed by': [enz]}
        p = {m: float(10 ** rng.uniform(-3, 1)) for m in subs}
        p['kcat_f'] = float(10 ** rng.uniform(-1, 4))
        kinetics[rid] = {enz: p}
    # an enzyme's partition holds the substrates of every reaction it catalyses
    # (kinetic_rate_laws.py:84-95), so each of its rate laws needs their Kms
    for rid, spec in reactions.items():
        enz = spec['catalyzed by'][0]
        p = kinetics[rid][enz]
        for other in reactions.values():
            if enz in other['catalyzed by']:
                for m, c in other['stoichiometry'].items():
                    if c < 0 and m not in p:
                        p[m] = float(10 ** rng.uniform(-3, 1))
    initial = {'internal': {k[1]: float(rng.uniform(0.1, 2.0)) for k in internal},
               'external': {k[1]: float(rng.uniform(1.0, 10.0)) for k in external}}
    for e in enzymes:
        initial['internal'][e[1]] = float(10 ** rng.uniform(-4, -2))
    return {'reactions': reactions, 'kinetic_parameters': kinetics, 'initial_state': initial}


def mother_machine(n_agents=3, bounds=(20.0, 20.0), n_bins=(10, 10), channel_space=1.5, channel_height=None,
                   spacer_thickness=0.1, seed=SEED):
    """The reference's mother machine (vivarium/experiments/mother_machine.py):
    get_mother_machine_config's values and mother_machine_body_config's placement --
    one cell of length 2, width 1 and angle pi / 2 at the bottom (y = 0.01) of
    ``n_agents`` of the channels, at ``x = k * space - space / 2``, k = 1 ..
    n_spaces - 1, in shuffled order (a seeded NumPy permutation stands in for the
    reference's ``random.shuffle``).  Returns a dict: ``bounds``, ``n_bins``,
    ``channels`` (the ContactModel's ``channels=``), ``location`` [2, n], ``angle``
    [n], ``length``, ``width``, ``volume`` (fL) and ``mass`` (fg at DeriveGlobals'
    density of 1100 g/L: the CellModel's ``initial_mass``), ``growth_rate``,
    ``division_volume``, ``jitter_force``, and the diffusion field's ``molecules``,
    ``diffusion`` and ``gradient``.  The ``gradient`` goes as it is to
    ``Lattice(..., gradient=)``, which fills the planes as the reference's make_gradient does."""
    bounds = (float(bounds[0]), float(bounds[1]))
    if channel_height is None:
        channel_height = 0.7 * bounds[1]
    n_spaces = math.floor(bounds[0] / channel_space)
    if not n_agents < n_spaces:
        raise ValueError('more agents than mother machine spaces')
    width, length = 1.0, 2.0
    radius = width / 2
    # volume_from_length (vivarium/library/cell_geometry): the capsule's caps and cylinder
    volume = (4 / 3) * math.pi * radius ** 3 + math.pi * radius ** 2 * (length - width)
    possible = np.array([[k * channel_space - channel_space / 2, 0.01] for k in range(1, n_spaces)])
    order = np.random.default_rng(seed).permutation(len(possible))
    location = np.ascontiguousarray(possible[order[:n_agents]].T)
    return {
        'bounds': bounds, 'n_bins': tuple(n_bins),
        'channels': {'channel_height': float(channel_height), 'channel_space': float(channel_space),
                     'spacer_thickness': float(spacer_thickness)},
        'location': location, 'angle': np.full(n_agents, math.pi / 2),
        'length': length, 'width': width, 'volume': volume, 'mass': volume * 1100.0,
        'growth_rate': 0.006, 'division_volume': 2.6, 'jitter_force': 1e-3,
        'molecules': ['glc'], 'diffusion': 5e-3,
        'gradient': {'type': 'gaussian', 'molecules': {'glc': {'center': [0.5, 0.5], 'deviation': 3}}},
    }


def chemotaxis_static(gradient='exponential', n_agents=1, seed=SEED, n_bins=(10, 10), **motility):
    """The reference's chemotaxis experiment (vivarium/experiments/chemotaxis.py:70-136): a
    static field of ``glc__D_e`` over bounds [1000, 3000] um centred at [0.5, 0.0] --
    exponential with scale 4.0 and base 1.3e2, or linear with base 1e-1 and slope 1.0 -- and
    ``n_agents`` agents at [0.5, 0.1] x bounds whose receptors start adapted to the field
    there (``initial_ligand = StaticField.value``).  Returns a dict: ``field`` (the
    StaticField, a ``Colony(environment=)``), ``motility`` (the MotilityModel; further keyword
    arguments such as ``substeps`` or ``flagella`` go to it), ``location`` [2, n] and
    ``bounds``.  The field and the sensing are the reference's; the kinematics are not."""
    from lens_amd.motility import MotilityModel
    from lens_amd.static_field import StaticField
    ligand, bounds, center = 'glc__D_e', [1000, 3000], [0.5, 0.0]
    if gradient == 'exponential':
        spec = {'center': center, 'scale': 4.0, 'base': 1.3e2}
    elif gradient == 'linear':
        spec = {'base': 1e-1, 'center': center, 'slope': 1.0}
    else:
        raise ValueError("chemotaxis_static: gradient must be 'exponential' or 'linear' (got %r)" % (gradient,))
    field = StaticField([ligand], bounds, {'type': gradient, 'molecules': {ligand: spec}}, n_bins=n_bins)
    x, y = 0.5 * bounds[0], 0.1 * bounds[1]
    motility.setdefault('ligand_id', ligand)
    motility.setdefault('initial_ligand', field.value(ligand, x, y))
    motility.setdefault('seed', seed)
    location = np.ascontiguousarray(np.repeat(np.array([[x], [y]]), int(n_agents), axis=1))
    return {'field': field, 'motility': MotilityModel(**motility), 'location': location, 'bounds': bounds}


def chemotaxis_variable_flagella(n_flagella=5, **motility):
    """The reference's ChemotaxisVariableFlagella compartment (vivarium/compartments/
    chemotaxis_flagella.py:55-91) as a MotilityModel: the receptor cluster at ligand
    ``MeAsp``, initial ligand 1e-2 mM, and FlagellaActivity with ``n_flagella`` (one
    count, or one per agent) in the place of the coarse motor.  Further keyword
    arguments (``substeps``, ``seed``, ...) go to the MotilityModel."""
    from lens_amd.motility import FlagellaModel, MotilityModel
    motility.setdefault('ligand_id', 'MeAsp')
    motility.setdefault('initial_ligand', 1e-2)
    return MotilityModel(flagella=FlagellaModel(n_flagella), **motility)


def flagella_expression():
    """The reference's flagella expression configuration (get_flagella_expression,
    vivarium/processes/ode_expression.py:360-400): its four numbers and the protein
    map, both states starting at zero.  At these rates the transcript settles at 5e-5 mM
    and the protein gains 4e-9 mM/s: 2 flagella after 630 s, 7 after a 2520-s cell cycle at
    the initial volume and 14 at the doubled cell's."""
    return {
        'transcription_rates': {'flag_RNA': 1e-6},
        'translation_rates': {'flagella': 8e-5},
        'degradation_rates': {'flag_RNA': 2e-2},
        'protein_map': {'flagella': 'flag_RNA'},
        'initial_state': {'internal': {'flagella': 0.0, 'flag_RNA': 0.0}},
    }


def chemotaxis_ode_expression_flagella(expression=None, division='merged', **motility):
    """The reference's ChemotaxisODEExpressionFlagella compartment (vivarium/compartments/
    chemotaxis_flagella.py:94-173; the ``ode_expression`` agent type of its chemotaxis
    experiment) as what a Colony takes: ``{'cells': CellModel, 'motility': MotilityModel}``
    for ``Colony(..., **chemotaxis_ode_expression_flagella())``.  GrowthProtein at growth
    rate 0.000275 from 1339 fg; the receptor cluster at ligand ``MeAsp``, initial ligand
    1e-2 mM; FlagellaActivity starting without flagella, their count derived from
    ``expression`` (default :func:`flagella_expression`); the motile state divided as the
    reference's Store does (``division='merged'``).  Further keyword arguments
    (``substeps``, ``seed``, ...) go to the MotilityModel."""
    from lens_amd.cells import CellModel
    from lens_amd.motility import FlagellaModel, MotilityModel
    motility.setdefault('ligand_id', 'MeAsp')
    motility.setdefault('initial_ligand', 1e-2)
    flagella = FlagellaModel(0, expression=flagella_expression() if expression is None else expression)
    return {'cells': CellModel(growth_rate=0.000275, initial_mass=1339.0),
            'motility': MotilityModel(flagella=flagella, division=division, **motility)}


AMINO_ACIDS = {
    'A': 'Alanine', 'R': 'Arginine', 'N': 'Asparagine', 'D': 'Aspartate', 'C': 'Cysteine', 'E': 'Glutamate',
    'Q': 'Glutamine', 'G': 'Glycine', 'H': 'Histidine', 'I': 'Isoleucine', 'L': 'Leucine', 'K': 'Lysine',
    'M': 'Methionine', 'F': 'Phenylalanine', 'P': 'Proline', 'S': 'Serine', 'T': 'Threonine', 'W': 'Tryptophan',
    'Y': 'Tyrosine', 'V': 'Valine'}


def flagella_translation(data, operons=None, sequences=None, seed=SEED, **model):
    """The translation process of the reference's flagella agent
    (vivarium/compartments/flagella_expression.py:110-117) as a
    :class:`~lens_amd.translation.TranslationModel`, from a dict of the shape of
    tests/golden/flagella_translation.json: ``transcripts`` [(operon, product)],
    ``transcript_affinities`` (one per transcript), ``elongation_rate``,
    ``polymerase_occlusion`` and ``sequences`` ({product: 'MSK...'}) or, where the real ones
    are not at hand, ``estimated_length`` ({product: residues}), from which seeded uniform
    random sequences over the 20 amino acids are drawn -- the size and the shape of the
    reference's model, not its proteins.  ``operons`` keeps only those operons' transcripts:
    the whole chromosome has 15 operons and 49 products, more than the 64 active species a
    StochasticModel holds beside the free ribosome (as passive rows they all fit:
    :func:`flagella_gene_expression`).  Templates are the reference's
    generate_template: one terminator at the sequence's end, the product its only product.
    An operon's transcript is the species ``<operon>_RNA`` of the stochastic table.
    Further keyword arguments (``max_ribosomes``, ``release``, ``seed`` of the draws, ...)
    go to the TranslationModel."""
    from lens_amd.translation import TranslationModel
    sequences = sequences if sequences is not None else data.get('sequences')
    rng = np.random.default_rng(seed)
    symbols = sorted(AMINO_ACIDS)
    if sequences is None:
        sequences = {p: ''.join(symbols[i] for i in rng.integers(0, len(symbols), int(length)))
                     for p, length in sorted(data['estimated_length'].items())}
    keys = [(o, p) for o, p in map(tuple, data['transcripts']) if operons is None or o in operons]
    affinity = {tuple(k): a for k, a in zip(data['transcripts'], data['transcript_affinities'])}
    templates = {k: {'id': k, 'position': 0, 'direction': 1, 'sites': [], 'terminators': [
        {'position': len(sequences[k[1]]), 'strength': 1.0, 'products': [k[1]]}]} for k in keys}
    model.setdefault('seed', seed)
    # the reference keeps transcripts and proteins in two stores; in one table the operon fliL
    # and the protein fliL need two names
    model.setdefault('transcript_species', {o: o + '_RNA' for o, _ in keys})
    return TranslationModel({k: sequences[k[1]] for k in keys}, templates, {k: affinity[k] for k in keys},
                            data['elongation_rate'], data['polymerase_occlusion'], AMINO_ACIDS,
                            list(AMINO_ACIDS.values()), **model)


def _transcription_model(data, templates, sequence, affinities, **model):
    from lens_amd.transcription import TranscriptionModel
    domains = data.get('domains')
    if isinstance(domains, list):                # JSON has no int keys: the fixtures hold a list
        domains = {d['id']: d for d in domains}
    return TranscriptionModel(sequence, templates, data.get('genes', {}), affinities,
                              data.get('transcription_factors') or sorted(
                                  {f for t in templates.values() for s in t.get('sites', []) for f in s['thresholds']}),
                              model.pop('elongation_rate', data.get('elongation_rate', 10.0)),
                              model.pop('polymerase_occlusion', data.get('polymerase_occlusion', 5)),
                              domains=domains, **model)


def _affinity_dict(pairs):
    """``promoter_affinities`` of a fixture ([[promoter, state, ...], affinity] pairs) as the
    reference's dict of tuples."""
    return pairs if isinstance(pairs, dict) else {tuple(k): v for k, v in pairs}


# The engine's own two-promoter chromosome of toy_transcription(): the shape of the reference's
# toy (two promoters, directions +1 and -1, one site each, two terminators each with strengths
# 0.5 and 1.0), not its data.
TOY_CHROMOSOME = {
    'sequence': 'GGATCCTAGCATTGCAAGTCCGATAGGCTTAACG',
    'genes': {'oP': ['gP'], 'oPQ': ['gP', 'gQ'], 'oR': ['gR'], 'oRS': ['gR', 'gS']},
    'promoters': {
        'pP': {'id': 'pP', 'position': 2, 'direction': 1, 'sites': [{'thresholds': {'tfP': 0.2}}],
               'terminators': [{'position': 7, 'strength': 0.5, 'products': ['oP']},
                               {'position': 13, 'strength': 1.0, 'products': ['oPQ']}]},
        'pR': {'id': 'pR', 'position': -2, 'direction': -1, 'sites': [{'thresholds': {'tfR': 0.4}}],
               'terminators': [{'position': -8, 'strength': 0.5, 'products': ['oR']},
                               {'position': -14, 'strength': 1.0, 'products': ['oRS']}]}},
    'promoter_affinities': [[['pP', None], 1.0], [['pP', 'tfP'], 10.0], [['pR', None], 1.0], [['pR', 'tfR'], 10.0]],
    'transcription_factors': ['tfP', 'tfR'],
}


def toy_transcription(data=None, **model):
    """A toy chromosome as a :class:`~lens_amd.transcription.TranscriptionModel`: two promoters,
    directions +1 and -1, one site each, two terminators each with strengths 0.5 and 1.0, at
    ``elongation_rate`` 10 and ``polymerase_occlusion`` 5 (the reference's docstring example,
    vivarium/processes/transcription.py:158-173).  ``data``: a dict of the shape of
    tests/golden/toy_chromosome.json (the reference's ``toy_chromosome_config``, thresholds as
    magnitudes in mM); without one, the engine's own :data:`TOY_CHROMOSOME` of the same shape.
    Further keyword arguments (``max_rnaps``, ``seed``, ...) go to the TranscriptionModel."""
    data = copy.deepcopy(TOY_CHROMOSOME if data is None else data)
    return _transcription_model(data, data['promoters'], data['sequence'], _affinity_dict(data['promoter_affinities']),
                                **model)


def flagella_transcription(data, operons=None, sequence=None, seed=SEED, **model):
    """The transcription process of the reference's flagella agent
    (vivarium/compartments/flagella_expression.py:100-108) as a
    :class:`~lens_amd.transcription.TranscriptionModel`, from a dict of the shape of
    tests/golden/flagella_transcription.json: ``promoters`` (thresholds in mM, after the
    reference's apply_thresholds), ``genes``, ``transcription_factors``, ``promoter_affinities``
    ([[promoter, state, ...], affinity] pairs), ``elongation_rate`` and ``polymerase_occlusion``.

    ``sequence``: the genome the promoters' positions index.  The E. coli genome is not part of
    the reference tree, so without one (and without ``data['sequence']``) a seeded uniform random
    genome is drawn over a COMPACT SYNTHETIC LAYOUT: the kept promoters lie one after the other,
    each on a span of her true length (|last terminator - promoter|) and in her true direction,
    her terminators at their true relative positions -- only the spans the promoters read exist, so
    the absolute positions differ from the fixture's.  That is the size and the shape of the
    reference's model, not its genes.

    ``operons`` keeps only the promoters that make one of those operons: the whole pipeline
    (15 transcripts, 49 proteins, complexes) does not fit the 64 active species of a
    StochasticModel (with passive rows it does: :func:`flagella_gene_expression`).  An
    operon's transcript is the species ``<operon>_RNA`` of the stochastic table, the name
    :func:`flagella_translation` reads.  Further keyword arguments (``max_rnaps``, ``seed`` of the
    draws, ...) go to the TranscriptionModel."""
    promoters = {k: copy.deepcopy(p) for k, p in data['promoters'].items()
                 if operons is None or any(o in operons for t in p['terminators'] for o in t['products'])}
    if not promoters:
        raise ValueError('flagella_transcription: no promoter makes any of the operons %r' % (operons,))
    sequence = sequence if sequence is not None else data.get('sequence')
    if sequence is None:
        rng = np.random.default_rng(seed)
        base = 1                                 # position 0 stays unread: a backward slice must not end at -1
        for p in promoters.values():
            direction = p['direction']
            span = (p['terminators'][-1]['position'] - p['position']) * direction
            start = base if direction == 1 else base + span
            for t in p['terminators']:
                t['position'] = start + (t['position'] - p['position'])
            p['position'] = start
            base += span + 1
        sequence = ''.join('ACGT'[i] for i in rng.integers(0, 4, base))
    affinities = {k: v for k, v in _affinity_dict(data['promoter_affinities']).items() if k[0] in promoters}
    model.setdefault('seed', seed)
    model.setdefault('transcript_species', {o: o + '_RNA' for p in promoters.values() for t in p['terminators']
                                            for o in t['products']})
    return _transcription_model(data, promoters, sequence, affinities, **model)


def _degradation_model(data, transcription, transcripts=None):
    from lens_amd.degradation import DegradationModel
    kms = {e: {t: km for t, km in per.items() if transcripts is None or t in transcripts}
           for e, per in data['michaelis_constants']['transcripts'].items()}
    return DegradationModel.from_transcription(transcription, data['catalytic_rates'], {'transcripts': kms})


def toy_degradation(data, **model):
    """The reference's ``TOY_CONFIG`` (vivarium/processes/degradation.py:30-50) as a
    :class:`~lens_amd.degradation.DegradationModel`, from a dict of the shape of
    tests/golden/toy_degradation.json.  Further keyword arguments go to the DegradationModel."""
    from lens_amd.degradation import DegradationModel
    return DegradationModel(data['sequences'], data['catalytic_rates'], data['michaelis_constants'], **model)


def flagella_degradation(data, transcription):
    """The RNA degradation process of the reference's flagella agent
    (vivarium/compartments/flagella_expression.py:119-128) as a
    :class:`~lens_amd.degradation.DegradationModel`, from a dict of the shape of
    tests/golden/flagella_degradation.json (``catalytic_rates``: endoRNAse 0.02;
    ``michaelis_constants``: 1e-23 mol / fL per operon).  The sequences are
    ``transcription.product_sequences()``, as the reference takes them from its Chromosome; of the
    fixture's operons only those the transcription model makes are kept.  The transcripts carry
    the species names of the transcription model (``<operon>_RNA``)."""
    return _degradation_model(data, transcription, set(transcription.product_sequences()))


# the rows whose '_divider' the reference's flagella agent overrides to 'set'
# (flagella_schema_override, vivarium/compartments/flagella_expression.py:73-90)
FLAGELLA_SET_DIVIDERS = ('CpxR', 'CRP', 'Fnr', 'endoRNAse')


def flagella_gene_expression(tx_data, tl_data, cx_data, deg_data, operons=None, seed=SEED, set_dividers=False, **kw):
    """The four expression processes of the reference's flagella agent (``GeneExpression`` as
    flagella_expression.py:93-137 configures it: Transcription, Translation, RnaDegradation,
    Complexation) as what a Colony takes: ``{'stochastic', 'transcription', 'translation',
    'degradation'}`` for ``Colony(..., **flagella_gene_expression(...))``, from the four fixtures
    tests/golden/flagella_{transcription,translation,complexation,degradation}.json.

    The reactions are the 7 complexation reactions only, and ``species`` holds the monomers and
    the complexes they name (37 rows that vk_ssa_step stages).  Every other row is ``passive``, in
    this order: the transcripts (``<operon>_RNA``, in the transcription model's product order),
    the translated proteins that no reaction names (in the translation model's order), the
    transcription factors a threshold names, the degradation enzymes, ``Ribosome``,
    ``RNA Polymerase``, and what else the initial state's proteins name.  ``initial`` is
    ``get_flagella_initial_state`` (flagella_expression.py:318-349) as the degradation fixture
    records it (its ``molecules`` are pools, not rows: ``Colony.set_transcription_molecules`` /
    ``set_translation_molecules``).  ``operons`` keeps only those operons' promoters and
    transcripts; ``None`` is the whole chromosome.  ``max_rnaps``, ``sequence`` and
    ``sequence_path`` go to the TranscriptionModel, ``max_ribosomes``, ``sequences`` and
    ``release`` to the TranslationModel, ``seed`` to all three, anything else to the
    StochasticModel.  ``set_dividers=True`` applies the reference's schema override
    (:data:`FLAGELLA_SET_DIVIDERS`): both daughters keep the mother's regulators and RNase; the
    default splits every row, as before."""
    from lens_amd.stochastic import StochasticModel
    tx_kw = {k: kw.pop(k) for k in ('max_rnaps', 'sequence', 'sequence_path') if k in kw}
    tl_kw = {k: kw.pop(k) for k in ('max_ribosomes', 'sequences', 'release') if k in kw}
    transcription = flagella_transcription(tx_data, operons=operons, seed=seed, **tx_kw)
    translation = flagella_translation(tl_data, operons=operons, seed=seed, **tl_kw)
    degradation = flagella_degradation(deg_data, transcription)
    species = list(cx_data['monomer_ids']) + list(cx_data['complex_ids'])
    proteins = deg_data['initial_state']['proteins']
    passive = []
    from lens_amd.transcription import UNBOUND_RNAP_KEY
    from lens_amd.translation import UNBOUND_RIBOSOME_KEY
    for name in (transcription.products + degradation.transcript_names() +
                 [s for s in translation.species() if s != UNBOUND_RIBOSOME_KEY] + transcription.factors_used() +
                 degradation.enzyme_order + [UNBOUND_RIBOSOME_KEY, UNBOUND_RNAP_KEY] + list(proteins)):
        if name not in species and name not in passive:
            passive.append(name)
    initial = {name: count for name, count in proteins.items()}
    initial.update({transcription.transcript_species.get(o, o): count
                    for o, count in deg_data['initial_state']['transcripts'].items()
                    if transcription.transcript_species.get(o, o) in passive})
    if set_dividers:
        kw['dividers'] = dict(kw.get('dividers') or {}, **{
            name: 'set' for name in FLAGELLA_SET_DIVIDERS if name in species or name in passive})
    stochastic = StochasticModel(species, cx_data['stoichiometry'], cx_data['rates'], initial=initial, seed=seed,
                                 passive=passive, **kw)
    return {'stochastic': stochastic, 'transcription': transcription, 'translation': translation,
            'degradation': degradation}


def flagella_molecular_weights(tl_data, transcription=None, complexes=None):
    """The ``mw`` properties the reference hangs on the flagella agent's stores, as
    ``{row name: g/mol}`` for ``CellModel(molecular_weights=...)``: ``tl_data['molecular_weight']``
    (tests/golden/flagella_translation.json: vivarium/data/molecular_weight.py for every
    translated protein) restricted to the names that will be rows of the count table, the
    products of ``tl_data['transcripts']``; ``complexes`` ({name: g/mol}, the same file's entries
    for the complexes: tests/golden/flagella_complex_weights.json) joins them as it is.
    The translation fixture holds the proteins' weights only, so WITHOUT ``complexes`` the
    heaviest nodes of the reference's cell -- ``flagella``, the motor, the motor switch, the
    export apparatus, ``flhDC`` and its transcript -- weigh nothing: pass that fixture's dict
    for the reference's cell.

    With a ``transcription`` model also the transcripts: the reference looks the OPERON's name up
    in the same dict (translation.py:389-393), so ``fliL``'s transcript weighs what the FliL
    protein weighs and ``flhDC``'s what the complex weighs -- a name collision in the reference,
    kept here, under the engine's ``<operon>_RNA`` row names.  An operon that names no protein or
    complex has no weight, as there."""
    weights = tl_data['molecular_weight']
    out = {p: float(weights[p]) for _, p in map(tuple, tl_data['transcripts']) if p in weights}
    out.update({str(name): float(w) for name, w in (complexes or {}).items()})
    if transcription is not None:
        named = dict({k: float(v) for k, v in weights.items()}, **out)
        for operon, species in transcription.transcript_species.items():
            if operon in named:
                out[species] = named[operon]
    return out


def gene_expression_cell(tl_data, transcription=None, complexes=None, **cell):
    """``GeneExpression``'s own cell (vivarium/compartments/gene_expression.py:62-77) as a
    :class:`~lens_amd.cells.CellModel`: no growth process, TreeMass from 1339 fg over
    :func:`flagella_molecular_weights`, DeriveGlobals, DivisionVolume.  It is the reference's
    cell only with ``complexes`` (see there).  Further keyword arguments
    (``division_volume``, ...) go to the CellModel."""
    from lens_amd.cells import CellModel
    cell.setdefault('initial_mass', 1339.0)
    return CellModel(model='tree_mass', molecular_weights=flagella_molecular_weights(tl_data, transcription, complexes),
                     **cell)


def chemotaxis_expression_flagella(tx, tl, cx, deg, division='merged', complexes=None, expression=None, **motility):
    """The reference's ChemotaxisExpressionFlagella compartment (vivarium/compartments/
    chemotaxis_flagella.py:176-260) as what a Colony takes, in the manner of
    :func:`chemotaxis_ode_expression_flagella`: the four expression models of
    :func:`flagella_gene_expression` on the fixtures ``tx``, ``tl``, ``cx``, ``deg`` with the
    reference's ``set`` dividers; ``cells``: GrowthProtein at growth rate 0.000275 from 1339 fg
    with TreeMass from its default 0 fg over the aggregate protein and then the table
    (:func:`flagella_molecular_weights`; ``complexes`` as there: without it the complexes weigh
    nothing); ``motility``: the receptor
    cluster at ligand ``MeAsp``, initial ligand 0.1 mM, and FlagellaActivity starting without
    flagella, their count the ``flagella`` complex's.  ``expression``: keyword arguments of
    :func:`flagella_gene_expression` (``operons``, ``seed``, ``max_rnaps``, ...); further
    keyword arguments (``substeps``, ``seed``, ...) go to the MotilityModel."""
    from lens_amd.cells import CellModel
    from lens_amd.motility import FlagellaModel, MotilityModel
    models = flagella_gene_expression(tx, tl, cx, deg, set_dividers=True, **(expression or {}))
    weights = flagella_molecular_weights(tl, models['transcription'], complexes)
    rows = set(models['stochastic'].rows)
    motility.setdefault('ligand_id', 'MeAsp')
    motility.setdefault('initial_ligand', 0.1)
    models['cells'] = CellModel('growth_protein', growth_rate=0.000275, initial_mass=1339.0,
                                molecular_weights={k: w for k, w in weights.items() if k in rows})
    models['motility'] = MotilityModel(flagella=FlagellaModel(0, complexes='flagella'), division=division, **motility)
    return models


def deepcopy_config(cfg):
    return copy.deepcopy(cfg)
