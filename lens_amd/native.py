"""ctypes binding of the C ABI in ``include/vk_kinetics.h``.

The shared library ``lens_amd/lib/libvk_kinetics.so`` is built in-tree by
``lens_amd/build.py`` (hipcc, gfx950).  There is no fallback: if the library
is missing or a call fails, a :class:`NativeError` is raised.

torch is imported before the library is loaded so that the HIP runtime torch
ships (SONAME ``libamdhip64.so.7``) is the one the library binds to -- device
pointers from torch tensors and torch's stream handles are then valid for
every vk_* call.
"""

from __future__ import annotations

import ctypes
import os

import numpy as np

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib')
LIB_PATH = os.environ.get('VK_KINETICS_LIB') or os.path.join(LIB_DIR, 'libvk_kinetics.so')   # env: A/B builds

VK_OK, VK_ERR_ARG, VK_ERR_HIP, VK_ERR_LIMIT, VK_ERR_NOMEM = 0, 1, 2, 3, 4
VK_AGENT_MAX_STEPS, VK_AGENT_H_UNDERFLOW, VK_AGENT_NONFINITE = 1, 2, 4

# every symbol include/vk_kinetics.h declares (tests check the exports)
EXPORTS = (
    'vk_abi_version', 'vk_last_error', 'vk_table_create', 'vk_table_destroy', 'vk_table_specialize',
    'vk_rate_fluxes', 'vk_step_euler', 'vk_step_dopri5', 'vk_step_dopri5_multi', 'vk_step_dopri5_gather', 'vk_field_uniform',
    'vk_diffuse', 'vk_diffuse_part', 'vk_diffuse_delta', 'vk_diffuse_coupled', 'vk_diffuse_plan', 'vk_diffuse_plan_lanes', 'vk_set_stencil_bands', 'vk_set_stencil_depth', 'vk_set_stencil_kernel', 'vk_set_stencil_mode',
    'vk_timestamp', 'vk_wall_clock_khz', 'vk_copy_stream', 'vk_gather', 'vk_exchange_sorted',
    'vk_exchange_atomic', 'vk_bin_sites', 'vk_cell_step', 'vk_divide_scratch_bytes', 'vk_divide_plan',
    'vk_divide_gather', 'vk_divide_lineage', 'vk_divide_locations', 'vk_kremling_step',
    'vk_expression_step', 'vk_motility_step', 'vk_occupancy_scratch_bytes', 'vk_occupancy_sort',
    'vk_exchange_ordered', 'vk_contact_scratch_bytes', 'vk_contact_step',
    'vk_response_begin', 'vk_response_end', 'vk_response_cells', 'vk_exchange_ordered_mixed',
    'vk_exchange_atomic_f64', 'vk_population_scratch_bytes', 'vk_population_plan', 'vk_contact_step_channels',
    'vk_flagella_step', 'vk_flagella_counts', 'vk_divide_flagella',
    'vk_ssa_step', 'vk_ssa_propensities', 'vk_divide_counts', 'vk_ssa_flagella_target',
    'vk_colonies_scratch_bytes', 'vk_colony_metrics',
    'vk_gradient_fill', 'vk_static_gather', 'vk_motility_step_static', 'vk_flagella_step_static',
    'vk_translation_step', 'vk_divide_ribosomes', 'vk_transcription_step', 'vk_rna_degradation_step',
    'vk_cell_step_tree',
)

VK_CELL_MASS, VK_CELL_VOLUME, VK_CELL_LENGTH, VK_CELL_SURFACE_AREA, VK_CELL_PROTEIN, VK_CELL_ANGLE = range(6)
VK_CELL_ROWS = 6
(VK_MOTIL_N_METHYL, VK_MOTIL_ACTIVITY, VK_MOTIL_CHEY_P, VK_MOTIL_CCW_MOTOR_BIAS, VK_MOTIL_CCW_TO_CW,
 VK_MOTIL_MOTOR_STATE, VK_MOTIL_ANGLE, VK_MOTIL_THRUST, VK_MOTIL_TORQUE) = range(9)
VK_MOTIL_ROWS = 9
VK_FLAG_CHEY, VK_FLAG_CHEY_P, VK_FLAG_CW_BIAS, VK_FLAG_MOTILE_STATE, VK_FLAG_PMF = range(5)
VK_FLAG_ROWS = 5
VK_FLAGI_TARGET, VK_FLAGI_HAVE, VK_FLAGI_MASK = range(3)
VK_FLAGI_ROWS = 3
VK_FLAGELLA_MERGED, VK_FLAGELLA_SPLIT_DICT = 0, 1
VK_DIVIDE_FLAGELLA_DOMAIN = 0x666c6167656c6c61     # mixed into the seed of vk_divide_flagella's draw
VK_SSA_MAX_SPECIES, VK_SSA_MAX_REACTIONS, VK_SSA_MAX_ORDER = 64, 32, 255
VK_SSA_DOMAIN = 0x7373615f73746570                 # mixed into the seed of vk_ssa_step's draws
VK_SSA_DIVIDE_DOMAIN = 0x7373615f64697669          # and of vk_divide_counts' coins
VK_SSA_MAX_EVENTS, VK_SSA_NONFINITE, VK_SSA_OVERFLOW, VK_SSA_BAD_KEY = 1, 2, 4, 8
VK_TL_MAX_SLOTS, VK_TL_MAX_TEMPLATES, VK_TL_MAX_MONOMERS, VK_TL_MAX_POSITION = 128, 64, 24, 0x00ffffff
VK_TL_DOMAIN = 0x746c5f5f73746570                  # mixed into the seed of vk_translation_step's draws
VK_TL_DIVIDE_DOMAIN = 0x746c5f5f64697669           # and of vk_divide_ribosomes' coins
VK_TL_SLOTS_FULL, VK_TL_BAD_KEY, VK_TL_NONFINITE, VK_TL_OVERFLOW, VK_TL_MAX_EVENTS = 1, 2, 4, 8, 16
VK_TL_RELEASE_REFERENCE, VK_TL_RELEASE_TEMPLATE = 0, 1
VK_TX_MAX_SLOTS, VK_TX_MAX_TEMPLATES, VK_TX_MAX_TERMINATORS, VK_TX_MAX_MONOMERS = 128, 64, 4, 4
VK_TX_MAX_SITES, VK_TX_MAX_FACTORS, VK_TX_MAX_AFFINITIES, VK_TX_MAX_POSITION = 4, 4, 1024, 0x003fffff
VK_TX_DOMAIN = 0x74785f5f73746570                  # mixed into the seed of vk_transcription_step's draws
VK_TX_DIVIDE_DOMAIN = 0x74785f5f64697669           # and, by the host, of the RNAP lists' division coins
VK_TX_SLOTS_FULL, VK_TX_BAD_KEY, VK_TX_NONFINITE, VK_TX_OVERFLOW, VK_TX_MAX_EVENTS = 1, 2, 4, 8, 16
VK_TX_SEQUENCE_AUTO, VK_TX_SEQUENCE_GLOBAL, VK_TX_SEQUENCE_LDS = 0, 1, 2
VK_DEG_MAX_TRANSCRIPTS, VK_DEG_MAX_ENZYMES, VK_DEG_MAX_PAIRS, VK_DEG_MAX_MONOMERS = 64, 8, 256, 4
VK_DEG_MAX_LENGTH = 0x003fffff
VK_DEG_NONFINITE, VK_DEG_OVERFLOW = 1, 2
VK_SSA_PASSIVE_DOMAIN = 0x7373615f70617373         # mixed by the host into the seed of the passive rows' division
(VK_COLONY_MASS, VK_COLONY_CELL_AREA, VK_COLONY_CX, VK_COLONY_CY, VK_COLONY_SXX, VK_COLONY_SYY, VK_COLONY_SXY,
 VK_COLONY_ANGLE, VK_COLONY_MAJOR, VK_COLONY_MINOR) = range(10)
VK_COLONY_ROWS = 10
VK_COLONIES_TOO_LONG, VK_COLONIES_GAVE_UP = 1, 2
VK_GRADIENT_UNIFORM, VK_GRADIENT_GAUSSIAN, VK_GRADIENT_LINEAR, VK_GRADIENT_EXPONENTIAL = range(4)
VK_GRADIENT_MAX = 8
VK_GROWTH_PROTEIN, VK_GROWTH_MASS, VK_GROWTH_TREE = 0, 1, 2
VK_TREE_MAX_WEIGHTED = 256
VK_RNG_STREAM, VK_RNG_PHILOX = 0, 1
VK_DIVIDE_SET, VK_DIVIDE_SPLIT, VK_DIVIDE_ZERO = 0, 1, 2
VK_UNIFORM_BLOCKS = 512
VK_PART_ALL, VK_PART_INTERIOR, VK_PART_EDGES = 0, 1, 2
VK_PLAN_COUPLED, VK_PLAN_COUPLED_AGENTS = 1, 2        # vk_diffuse_plan's coupled argument


class NativeError(RuntimeError):
    pass


_i32p = ctypes.POINTER(ctypes.c_int32)
_f64p = ctypes.POINTER(ctypes.c_double)
_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_f64 = ctypes.c_double


class VkTableDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        'n_species', 'n_dyn', 'n_reactions', 'n_rate_laws', 'n_params', 'n_ext',
        'n_sets', 'n_members', 'n_upd', 'n_exch')] + [
        ('rl_reaction', _i32p), ('rl_enzyme', _i32p), ('rl_kcat', _i32p),
        ('rl_num_ptr', _i32p), ('rl_den_ptr', _i32p), ('set_ptr', _i32p),
        ('mem_species', _i32p), ('mem_param', _i32p), ('upd_ptr', _i32p),
        ('upd_rxn', _i32p), ('upd_coeff', _f64p), ('ex_ptr', _i32p),
        ('ex_rxn', _i32p), ('ex_coeff', _f64p)]


class VkOdeOpts(ctypes.Structure):
    _fields_ = [('rtol', ctypes.c_double), ('atol', ctypes.c_double),
                ('max_steps', ctypes.c_int32), ('variant', ctypes.c_int32)]


class VkCellParams(ctypes.Structure):
    _fields_ = [('model', ctypes.c_int32), ('rng', ctypes.c_int32)] + [
        (n, ctypes.c_double) for n in (
            'factor', 'divide_protein', 'division_volume', 'protein_mw', 'avogadro', 'fg_per_g',
            'density', 'volume_to_fl', 'cap_volume', 'cap_area', 'two_r', 'width', 'sa_const',
            'sa_lin')] + [('seed', ctypes.c_uint64), ('step', ctypes.c_uint64)]


class VkKremlingParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in (
        'k1', 'k2', 'k3', 'K1', 'K2', 'K3', 'kd', 'm', 'n', 'x0', 'kg6p', 'Kg6p', 'kptsup', 'Kglc',
        'Keiiap', 'klac', 'Km_lac', 'Kieiia', 'kgly', 'kpyk', 'kpdh', 'kpts', 'km_pts', 'mw1', 'mw2',
        'mw3', 'Y1_sim', 'Y2_sim', 'Y3_sim', 'K', 'kb', 'ksyn', 'KI')]


class VkMotilityParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in (
        'n_Tar', 'n_Tsr', 'K_Tar_off', 'K_Tar_on', 'K_Tsr_off', 'K_Tsr_on', 'k_meth', 'k_demeth', 'adapt_rate',
        'CheR', 'CheB', 'k_y', 'k_s', 'k_z', 'gamma_Y', 'adapt_precision', 'mb_0', 'cw_to_ccw',
        'cw_to_ccw_leak', 'run_speed', 'tumble_sigma')] + [('seed', ctypes.c_uint64)]


class VkFlagellaParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in (
        'YP_ss', 'sigma2_Y', 'tau', 'K_d', 'H', 'omega', 'g_0', 'g_1', 'K_D', 'flagellum_thrust',
        'tumble_scaling', 'run_scaling')]


class VkGradientSpec(ctypes.Structure):
    """One analytic gradient (vk_gradient_spec): p0, p1 by type, cx, cy in um."""
    _fields_ = [('type', ctypes.c_int32), ('cx', ctypes.c_double), ('cy', ctypes.c_double),
                ('p0', ctypes.c_double), ('p1', ctypes.c_double)]


class VkContactParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('iterations', 'gx', 'gy', 'reserved')] + [
        (n, ctypes.c_double) for n in ('stiffness', 'max_length', 'width', 'length', 'max_push', 'max_turn',
                                       'jitter', 'jitter_angle')] + [('seed', ctypes.c_uint64)]


class VkContactChannels(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ('height', 'space', 'spacer')] + [
        ('n_lines', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class VkColoniesParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('gx', 'gy', 'min_cells', 'reserved')] + [
        (n, ctypes.c_double) for n in ('max_length', 'width', 'length', 'link_gap', 'mass')]


class VkResponseTable(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('n_mol', 'n_porin', 'n_det', 'n_save', 'n_expr', 'n_flux', 'n_ext',
                                              'reserved')] + [
        (n, _vp) for n in ('mol_int_row', 'mol_ext_row', 'porin_row', 'porin_perm', 'det_row', 'det_thr',
                           'save_row', 'expr_row')] + [('avogadro', ctypes.c_double), ('volume_fl', ctypes.c_double)]


class VkSsaNet(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('n_species', 'n_reactions', 'max_order', 'n_inv')] + [
        (n, _vp) for n in ('react_ptr', 'react_species', 'react_order', 'stoich_ptr', 'stoich_species',
                           'stoich_delta', 'rates', 'inv')]


class VkTlModel(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('n_templates', 'n_monomers', 'n_species', 'max_slots', 'occlusion',
                                              'release', 'ribosome_species', 'n_plan')] + [
        (n, _vp) for n in ('operon_species', 'seq_ptr', 'prod_ptr', 'prod_species', 'elongate', 'seq', 'affinity',
                           'interval')]


class VkTxModel(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('n_templates', 'n_monomers', 'n_species', 'max_slots', 'occlusion',
                                              'rnap_species', 'n_plan', 'n_affinities', 'atp_row', 'adp_row',
                                              'sequence', 'n_bases')] + [
        (n, _vp) for n in ('copy', 'n_term', 'term_pos', 'prod_ptr', 'prod_species', 'seq_ptr', 'site_ptr', 'thr_ptr',
                           'thr_species', 'aff_ptr', 'elongate', 'seq', 'seq2', 'term_strength', 'term_from',
                           'thr_value', 'affinity', 'interval')]


class VkDegModel(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('n_transcripts', 'n_enzymes', 'n_pairs', 'n_monomers', 'n_rows',
                                              'atp_row', 'adp_row', 'reserved')] + [
        (n, _vp) for n in ('transcript_row', 'enzyme_row', 'pair_ptr', 'pair_enzyme', 'composition', 'length', 'kcat',
                           'km')]


class VkPass(ctypes.Structure):
    """One pass of a diffusion call's plan (vk_diffuse_plan)."""
    _fields_ = [(n, ctypes.c_int32) for n in ('k', 'src', 'dst', 'f0', 'lo', 'hi', 'in_lo', 'in_hi', 'gap_lo',
                                              'gap_hi', 'kernel', 'couple', 'copy_back')]


_SIGS = {
    'vk_abi_version': ([], ctypes.c_int),
    'vk_last_error': ([], ctypes.c_char_p),
    'vk_table_create': ([ctypes.POINTER(VkTableDesc), ctypes.POINTER(_vp)], ctypes.c_int),
    'vk_table_destroy': ([_vp], ctypes.c_int),
    'vk_table_specialize': ([_vp, ctypes.c_char_p], ctypes.c_int),
    'vk_rate_fluxes': ([_vp, _i64, _i64, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_step_euler': ([_vp, _i64, _i64, _f64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_step_dopri5': ([_vp, _i64, _i64, _f64, ctypes.POINTER(VkOdeOpts), _vp, _vp, _vp, _vp,
                        _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_step_dopri5_multi': ([_vp, _i64, _i64, _f64, _i32, ctypes.POINTER(VkOdeOpts), _vp, _vp, _vp, _vp, _vp,
                              _i64, _vp, _i64, _vp, _vp, _i64, _vp], ctypes.c_int),
    'vk_step_dopri5_gather': ([_vp, _i64, _i64, _f64, ctypes.POINTER(VkOdeOpts), _vp, _vp, _vp, _vp, _vp, _vp,
                               _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp], ctypes.c_int),
    'vk_field_uniform': ([_vp, _i32, _i64, _i32, _i32, _i32, _vp, _vp, _vp], ctypes.c_int),
    'vk_diffuse': ([_vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                    _i32, _i32, _i32, _f64, _vp, _vp], ctypes.c_int),
    'vk_diffuse_part': ([_vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                         _i32, _i32, _i32, _f64, _vp, _i32, _i32, _vp], ctypes.c_int),
    'vk_diffuse_delta': ([_vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                          _i32, _i32, _i32, _f64, _vp, _vp], ctypes.c_int),
    'vk_diffuse_coupled': ([_vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _f64, _vp, _vp, _vp, _i32, _i64,
                            _i32p, _vp, _i64, _i32p, _vp, _i64, _f64, _vp], ctypes.c_int),
    'vk_diffuse_plan': ([_i32] * 12 + [ctypes.POINTER(VkPass), _i32, _i32p], ctypes.c_int),
    'vk_diffuse_plan_lanes': ([_i32] * 12 + [ctypes.POINTER(VkPass), _i32p, _i32p, _i32, _i32p], ctypes.c_int),
    'vk_set_stencil_bands': ([_i32, _i32], ctypes.c_int),
    'vk_set_stencil_depth': ([_i32], ctypes.c_int),
    'vk_set_stencil_kernel': ([_i32, _i32], ctypes.c_int),
    'vk_set_stencil_mode': ([_i32], ctypes.c_int),
    'vk_timestamp': ([_vp, _i32, _vp], ctypes.c_int),
    'vk_wall_clock_khz': ([], ctypes.c_int64),
    'vk_copy_stream': ([_vp, _vp, _i64, _vp], ctypes.c_int),
    'vk_gather': ([_vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _i64, _vp], ctypes.c_int),
    'vk_exchange_sorted': ([_vp, _i64, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _i32, _f64, _vp],
                           ctypes.c_int),
    'vk_exchange_atomic': ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _f64, _vp], ctypes.c_int),
    'vk_bin_sites': ([_vp, _i64, _i64, _i32, _i32, _f64, _f64, _i32, _vp, _vp, _vp], ctypes.c_int),
    'vk_cell_step': ([ctypes.POINTER(VkCellParams), _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
                     ctypes.c_int),
    'vk_cell_step_tree': ([ctypes.POINTER(VkCellParams), _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                           _i32, _vp, _vp, _i32, _vp, _vp], ctypes.c_int),
    'vk_divide_scratch_bytes': ([_i64], ctypes.c_int64),
    'vk_divide_plan': ([_vp, _i64, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_divide_gather': ([_i64, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp], ctypes.c_int),
    'vk_divide_lineage': ([_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_divide_locations': ([_i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp], ctypes.c_int),
    'vk_expression_step': ([_vp, _i64, _i64, _f64, _vp, _vp, _vp, _i32, _vp], ctypes.c_int),
    'vk_kremling_step': ([ctypes.POINTER(VkKremlingParams), _i64, _i64, _f64, _f64, _i32, _f64, _f64, _i32,
                          _vp, _vp, _f64, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_motility_step': ([ctypes.POINTER(VkMotilityParams), _i64, _i64, _f64, _i32, _vp, _vp, _vp, _vp, _i32, _i32,
                          _f64, _f64, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_flagella_step': ([ctypes.POINTER(VkMotilityParams), ctypes.POINTER(VkFlagellaParams), _i64, _i64, _f64, _i32,
                          _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _f64, _f64, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_gradient_fill': ([ctypes.POINTER(VkGradientSpec), _i32, _vp, _i64, _i64, _i32, _i32, _f64, _f64, _vp],
                         ctypes.c_int),
    'vk_static_gather': ([ctypes.POINTER(VkGradientSpec), _i32p, _i32p, _i32, _vp, _i64, _i64, _vp, _i64, _vp],
                         ctypes.c_int),
    'vk_motility_step_static': ([ctypes.POINTER(VkMotilityParams), _i64, _i64, _f64, _i32, _vp, _vp, _vp,
                                 ctypes.POINTER(VkGradientSpec), _i32, _i32, _f64, _f64, _vp, _vp, _vp, _vp],
                                ctypes.c_int),
    'vk_flagella_step_static': ([ctypes.POINTER(VkMotilityParams), ctypes.POINTER(VkFlagellaParams), _i64, _i64, _f64,
                                 _i32, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(VkGradientSpec), _i32, _i32, _f64, _f64,
                                 _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_flagella_counts': ([_i64, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_divide_flagella': ([_i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i32,
                            ctypes.c_uint64, ctypes.c_uint64, _i64, _vp], ctypes.c_int),
    'vk_ssa_step': ([ctypes.POINTER(VkSsaNet), _i64, _i64, _f64, _vp, _vp, ctypes.c_uint64, _vp, _i32, _vp, _vp, _vp],
                    ctypes.c_int),
    'vk_ssa_propensities': ([ctypes.POINTER(VkSsaNet), _i64, _i64, _vp, _vp, _vp], ctypes.c_int),
    'vk_divide_counts': ([_i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i32, ctypes.c_uint64,
                          ctypes.c_uint64, _i64, _vp], ctypes.c_int),
    'vk_ssa_flagella_target': ([_i64, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_translation_step': ([ctypes.POINTER(VkTlModel), _i64, _i64, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _vp,
                             _i32, _i32, _vp, _vp, _vp], ctypes.c_int),
    'vk_divide_ribosomes': ([_i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, ctypes.c_uint64,
                             ctypes.c_uint64, _vp], ctypes.c_int),
    'vk_transcription_step': ([ctypes.POINTER(VkTxModel), _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64,
                               _vp, _i32, _i32, _vp, _vp, _vp], ctypes.c_int),
    'vk_rna_degradation_step': ([ctypes.POINTER(VkDegModel), _i64, _i64, _f64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
                                ctypes.c_int),
    'vk_occupancy_scratch_bytes': ([_i64], ctypes.c_int64),
    'vk_occupancy_sort': ([_vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp], ctypes.c_int),
    'vk_exchange_ordered': ([_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _f64, _vp], ctypes.c_int),
    'vk_contact_scratch_bytes': ([_i64, _i64], ctypes.c_int64),
    'vk_contact_step': ([ctypes.POINTER(VkContactParams), _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32,
                         _f64, _f64, _vp, _vp, _vp, _i64, _vp], ctypes.c_int),
    'vk_contact_step_channels': ([ctypes.POINTER(VkContactParams), _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32,
                                  _i32, _f64, _f64, _vp, _vp, _vp, _i64, ctypes.POINTER(VkContactChannels), _vp, _vp],
                                 ctypes.c_int),
    'vk_colonies_scratch_bytes': ([_i64, _i64], ctypes.c_int64),
    'vk_colony_metrics': ([ctypes.POINTER(VkColoniesParams), _i64, _i64, _vp, _vp, _vp, _vp, _vp, _f64, _f64, _vp, _vp,
                           _vp, _vp, _vp, _vp, _vp, _i64, _vp], ctypes.c_int),
    'vk_population_scratch_bytes': ([_i64], ctypes.c_int64),
    'vk_population_plan': ([_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_response_begin': ([ctypes.POINTER(VkResponseTable), _i64, _i64, _f64] + [_vp] * 14, ctypes.c_int),
    'vk_response_end': ([ctypes.POINTER(VkResponseTable), _i64, _i64] + [_vp] * 15, ctypes.c_int),
    'vk_response_cells': ([_i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    'vk_exchange_ordered_mixed': ([_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _i32,
                                   _f64, _vp], ctypes.c_int),
    'vk_exchange_atomic_f64': ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _f64, _vp], ctypes.c_int),
}

_lib = None


def load(path: str = LIB_PATH):
    """Load (once) and return the library handle.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NativeError(
            '%s is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(there is no CPU fallback)' % path)
    import torch  # noqa: F401  -- bind to torch's HIP runtime (see module doc)
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, (args, res) in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    if lib.vk_abi_version() != 1:
        raise NativeError('ABI version mismatch')
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != VK_OK:
        msg = _lib.vk_last_error().decode(errors='replace') if _lib else ''
        raise NativeError('%s failed (status %d): %s' % (what, rc, msg))


def ptr(t) -> int:
    """Device pointer of a torch tensor (None -> NULL)."""
    return 0 if t is None else t.data_ptr()


def resolve_device(device=None):
    """torch.device with an explicit index: ``'cuda'`` -> ``cuda:<current>``.

    Tensors always report an indexed device, and ``cuda != cuda:0`` in torch,
    so every engine keeps the indexed form (Colony(device='cuda'))."""
    import torch
    if device is None:
        return torch.device('cuda', torch.cuda.current_device())
    d = torch.device(device)
    if d.type == 'cuda' and d.index is None:
        return torch.device('cuda', torch.cuda.current_device())
    return d


def stream_handle(stream=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


class DeviceTable:
    """Owns a vk_table compiled from a :class:`RateLawTable`."""

    def __init__(self, table):
        lib = load()
        self.table = table
        self._keep = []

        def ip(a):
            a = np.ascontiguousarray(a, dtype=np.int32)
            self._keep.append(a)
            return a.ctypes.data_as(_i32p)

        def dp(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            self._keep.append(a)
            return a.ctypes.data_as(_f64p)

        d = VkTableDesc()
        d.n_species, d.n_dyn, d.n_reactions = table.n_species, table.n_dyn, table.n_reactions
        d.n_rate_laws, d.n_params, d.n_ext = table.n_rate_laws, table.n_params, table.n_ext
        d.n_sets = len(table.set_ptr) - 1
        d.n_members = len(table.mem_species)
        d.n_upd = len(table.upd_rxn)
        d.n_exch = len(table.ex_rxn)
        for name in ('rl_reaction', 'rl_enzyme', 'rl_kcat', 'rl_num_ptr', 'rl_den_ptr', 'set_ptr',
                     'mem_species', 'mem_param', 'upd_ptr', 'upd_rxn', 'ex_ptr', 'ex_rxn'):
            setattr(d, name, ip(getattr(table, name)))
        d.upd_coeff = dp(table.upd_coeff)
        d.ex_coeff = dp(table.ex_coeff)
        h = _vp()
        check(lib.vk_table_create(ctypes.byref(d), ctypes.byref(h)), 'vk_table_create')
        self.handle = h
        self._keep = []

    def close(self):
        if getattr(self, 'handle', None) and _lib is not None:
            _lib.vk_table_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
