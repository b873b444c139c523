"""ctypes binding of libgapflow_hip.so (include/gapflow_hip.h).

There is deliberately no fallback: if the HIP library is missing or no MI355X is visible,
every compute entry point raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GPF_LIB_PATH', os.path.join(HERE, 'lib', 'libgapflow_hip.so'))

EOS_IDS = {'DH': 0, 'PL': 1, 'vdW': 2, 'MT': 3, 'cubic': 4, 'BWR': 5, 'Bayada': 6}
EOS_KEYS = {'DH': ['rho0', 'P0', 'C1', 'C2'], 'PL': ['rho0', 'P0', 'alpha'], 'vdW': ['M', 'T', 'a', 'b'],
            'MT': ['rho0', 'P0', 'K', 'n'], 'cubic': ['a', 'b', 'c', 'd'], 'BWR': ['T', 'gamma'],
            'Bayada': ['rho_l', 'rho_v', 'c_l', 'c_v']}
# defaults of the reference's EOS functions (pressure.py:79, 112, 140, 176, 208, 233): eos_pressure passes only the keys
# present in `properties` (pressure.py:73-76), so absent ones take these
EOS_DEFAULTS = {'DH': {'rho0': 877.7007, 'P0': 101325., 'C1': 3.5e8, 'C2': 1.23}, 'PL': {'rho0': 1.1853, 'P0': 101325., 'alpha': 0.},
                'vdW': {'M': 39.948, 'T': 100., 'a': 1.355, 'b': 0.03201}, 'MT': {'rho0': 700., 'P0': 0.101e6, 'K': 0.557e9, 'n': 7.33},
                'cubic': {'a': 15.2, 'b': -9.6, 'c': 3.35, 'd': -0.07}, 'BWR': {'gamma': 3.}, 'Bayada': {}}
PIEZO_IDS = {'Barus': 1, 'Roelands': 2, 'Dukler': 3, 'McAdams': 4}
PIEZO_KEYS = {'Barus': ['aB'], 'Roelands': ['mu_inf', 'p_ref', 'z'], 'Dukler': ['eta_v', 'rho_l', 'rho_v'],
              'McAdams': ['eta_v', 'rho_l', 'rho_v']}
# defaults of the reference's viscosity laws (viscosity.py:144, 168, 200, 231, 262, 288)
PIEZO_DEFAULTS = {'Barus': {'aB': 2.e-8}, 'Roelands': {'mu_inf': 1.e-3, 'p_ref': 1.96e8, 'z': 0.68},
                  'Dukler': {'eta_v': 3.9e-5, 'rho_l': 850., 'rho_v': 0.019}, 'McAdams': {'eta_v': 3.9e-5, 'rho_l': 850., 'rho_v': 0.019}}
THINNING_DEFAULTS = {'Eyring': {'tauE': 5.e5}, 'Carreau': {'mu_inf': 1.e-3, 'lam': 0.02, 'a': 2., 'N': 0.8}}
THINNING_IDS = {'Eyring': 1, 'Carreau': 2}
THINNING_KEYS = {'Eyring': ['tauE'], 'Carreau': ['mu_inf', 'lam', 'a', 'N']}
BC_P, BC_D, BC_N = 0, 1, 2
FIELD_Q, FIELD_TOPO, FIELD_EXTRA, FIELD_PRESSURE, FIELD_TAU_AVG, FIELD_WALL_LOWER, FIELD_WALL_UPPER = range(7)
FIELD_PRESSURE_VAR, FIELD_WALL_XZ_VAR, FIELD_WALL_YZ_VAR = 7, 8, 9
FIELD_DEFORMATION = 10
PROFILE_Z, PROFILE_U, PROFILE_V, PROFILE_TAU = 1, 2, 4, 8          # gpf_gap_profiles field_mask bits
PROFILE_GRADIENTS = 1
PROFILE_MODES = {'both': 0, 'top': 1, 'bottom': 2, 'none': 3}
PROBE_MAX = 256                     # gpf_probes_set: cells per handle
INTEGRAL_MAX_SECTIONS = 8           # gpf_integrals_set: flow cross-sections per direction
# what the host needs of the library's limits without loading it (sweeps and batch lengths are planned on the host); load()
# compares them with gpf_ensemble_limits, so a library built with other values does not load
SMALL_GRID_LDS_BYTES, SMALL_GRID_DOUBLES_PER_CELL = 150 * 1024, 16      # what one workgroup's LDS takes (csrc/api.hip)
LOG_CAPACITY = 4096                 # per-step records a handle's device log holds: the longest batch
# the ensembles' workspace tier (csrc/mid_layout.hpp; load() compares them with gpf_ensemble_limits2): the most cells of a member,
# ghost cells included, and the doubles its workspace in device memory holds per cell
MID_GRID_MAX_CELLS, MID_GRID_DOUBLES_PER_CELL = 16384, 19
ENSEMBLE_FORCE_WORKSPACE = 1        # gpf_ensemble_create2: flags
ENSEMBLE_TIERS = ('lds', 'workspace')       # gpf_ensemble_member_info: tier
EXTREMA_NAMES = ('p_max', 'p_min', 'rho_max', 'rho_min', 'h_min', 'u_max', 'v_max')     # gpf_extrema_*: the record's order
ELASTIC_SERIES_NAMES = ('d_sum', 'd2_sum', 'p_d', 'h_sum', 'd_max', 'd_min')     # gpf_elastic_series_*: the record's order; cells: d_max's, d_min's
# gpf_thinning_series_*: the record's order (eleven sums, three extrema); cells: eta_min's, eta_max's, rate_max's
THINNING_SERIES_NAMES = ('load', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top', 'tau0_xz_bot', 'tau0_yz_bot', 'tau0_xz_top', 'tau0_yz_top',
                         'eta_sum', 'rate_sum', 'eta_min', 'eta_max', 'rate_max')
THINNING_SERIES_EXTREMA = ('eta_min', 'eta_max', 'rate_max')
# gpf_changes_*: the record's order; cells: dmax_rho's, dmax_jx's, dmax_jy's
CHANGE_NAMES = ('d2_rho', 'd2_jx', 'd2_jy', 'q2_rho', 'q2_jx', 'q2_jy', 'dmass', 'dmax_rho', 'dmax_jx', 'dmax_jy', 'dt')
CHANGE_MAXIMA = ('dmax_rho', 'dmax_jx', 'dmax_jy')
INTEGRAL_SUMS = ('load', 'load_x', 'load_y', 'p_hx', 'p_hy', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top')
WEIGHTED_MAX_PLANES = 8             # gpf_weighted_set: weight planes per handle
WEIGHTED_INTEGRANDS = ('p', 'h', 'rho_h', 'jx_h', 'jy_h', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top')    # gpf_weighted_*: the record's order
STATS_FIELDS = ('p', 'rho', 'jx', 'jy')         # gpf_stats_*: field index, bit of the field mask
STATS_QUANTITIES = ('mean', 'm2', 'min', 'max')     # gpf_stats_read: quantity index
REGION_MAX = 8                      # gpf_regions_set: regions per handle
REGION_FIELDS = ('p', 'rho', 'h', 'jx', 'jy')       # gpf_region.field: GPF_REGION_*
REGION_INTS = ('cells', 'ix_min', 'ix_max', 'iy_min', 'iy_max')     # gpf_regions_*: the record's int64 part; its doubles: WEIGHTED_INTEGRANDS
LINE_MAX = 8                        # gpf_lines_set: lines per handle
LINE_FIELDS = ('rho', 'jx', 'jy', 'p', 'h', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top')       # gpf_lines_*: a point's nine values, in the record's order
LINE_AXES = ('x', 'y')              # gpf_line.along: GPF_LINE_X, GPF_LINE_Y
FRAME_FIELDS = LINE_FIELDS          # gpf_frame_spec.fields: bit f selects field f; a record keeps the mask's order
FRAME_REDUCE = ('sample', 'mean')   # gpf_frame_spec.reduce: GPF_FRAME_SAMPLE, GPF_FRAME_MEAN
FRAME_DTYPES = ('f8', 'f4')         # gpf_frame_spec.dtype: GPF_FRAME_F8, GPF_FRAME_F4
FRAME_MAX_STRIDE = 64               # gpf_frame_spec.sx, sy
FIELD_NCOMP = {FIELD_Q: 3, FIELD_TOPO: 3, FIELD_EXTRA: 1, FIELD_PRESSURE: 1, FIELD_TAU_AVG: 3,
               FIELD_WALL_LOWER: 6, FIELD_WALL_UPPER: 6, 7: 1, 8: 1, 9: 1, 10: 1}


class GpfConfig(C.Structure):
    _fields_ = [('Nx', C.c_int32), ('Ny', C.c_int32), ('dx', C.c_double), ('dy', C.c_double),
                ('U', C.c_double), ('V', C.c_double), ('eta', C.c_double), ('zeta', C.c_double),
                ('eos', C.c_int32), ('eos_par', C.c_double * 8),
                ('piezo', C.c_int32), ('piezo_par', C.c_double * 4),
                ('bc_rule', (C.c_int32 * 3) * 4), ('bc_value', C.c_double * 4),
                ('halo_lo', C.c_int32), ('halo_hi', C.c_int32),
                ('adaptive', C.c_int32), ('CFL', C.c_double), ('dt_fixed', C.c_double), ('tol', C.c_double),
                ('max_it', C.c_int64), ('mc_order', C.c_int32), ('device', C.c_int32),
                ('thinning', C.c_int32), ('thinning_par', C.c_double * 4)]


class GpfRegion(C.Structure):
    """gpf_region of include/gapflow_hip.h"""
    _fields_ = [('field', C.c_int32), ('box', C.c_int32 * 4), ('lo', C.c_double), ('hi', C.c_double)]


class GpfLine(C.Structure):
    """gpf_line of include/gapflow_hip.h"""
    _fields_ = [('along', C.c_int32), ('i0', C.c_int32), ('i1', C.c_int32)]


class GpfFrameSpec(C.Structure):
    """gpf_frame_spec of include/gapflow_hip.h"""
    _fields_ = [('fields', C.c_int32), ('ix0', C.c_int32), ('ix1', C.c_int32), ('iy0', C.c_int32), ('iy1', C.c_int32),
                ('sx', C.c_int32), ('sy', C.c_int32), ('reduce', C.c_int32), ('dtype', C.c_int32)]


class GpfScalars(C.Structure):
    _fields_ = [('step', C.c_int64), ('simtime', C.c_double), ('dt', C.c_double), ('ekin', C.c_double),
                ('ekin_old', C.c_double), ('residual', C.c_double), ('v_max', C.c_double), ('v_sound', C.c_double),
                ('mass', C.c_double), ('invalid', C.c_int32), ('converged', C.c_int32)]


# name -> (restype, argtypes); every symbol declared in include/gapflow_hip.h
_DP = C.POINTER(C.c_double)
_VPP = C.POINTER(C.c_void_p)
SIGNATURES = {
    'gpf_create': (C.c_int, [C.POINTER(GpfConfig), _VPP]),
    'gpf_destroy': (C.c_int, [C.c_void_p]),
    'gpf_set_stream': (C.c_int, [C.c_void_p, C.c_void_p]),
    'gpf_last_error': (C.c_char_p, []),
    'gpf_device_count': (C.c_int, []),
    'gpf_upload': (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_size_t]),
    'gpf_download': (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_size_t]),
    'gpf_update_closures': (C.c_int, [C.c_void_p]),
    'gpf_pre_run': (C.c_int, [C.c_void_p]),
    'gpf_step': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(GpfScalars), C.c_int64, C.POINTER(C.c_int64)]),
    'gpf_step_unfused': (C.c_int, [C.c_void_p]),
    'gpf_step_timed': (C.c_int, [C.c_void_p, C.c_int64, _DP, _DP]),
    'gpf_scalars': (C.c_int, [C.c_void_p, C.POINTER(GpfScalars)]),
    'gpf_set_ekin_old': (C.c_int, [C.c_void_p, C.c_double]),
    'gpf_set_dt': (C.c_int, [C.c_void_p, C.c_double]),
    'gpf_slab_message': (C.c_int, [C.c_void_p, _VPP, C.POINTER(C.c_size_t)]),
    'gpf_step_local': (C.c_int, [C.c_void_p, C.c_int]),
    'gpf_step_commit': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    'gpf_state': (C.c_int, [C.c_void_p, C.POINTER(GpfScalars)]),
    'gpf_viscous_stress': (C.c_int, [C.c_int64] + [C.c_void_p] * 6 + [C.c_double] * 3 + [C.c_int] + [C.c_void_p] * 3),
    'gpf_eos': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'gpf_viscosity': (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_double, C.c_double, C.c_void_p]),
    'gpf_elastic_setup': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_int]),
    'gpf_elastic_update': (C.c_int, [C.c_void_p]),
    'gpf_elastic_slab_setup': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_int]),
    'gpf_elastic_slab_buffer': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    'gpf_elastic_slab_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    'gpf_elastic_slab_convolve': (C.c_int, [C.c_void_p]),
    'gpf_elastic_slab_finish': (C.c_int, [C.c_void_p]),
    'gpf_elastic_slab_apply': (C.c_int, [C.c_void_p]),
    'gpf_p2p_export': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'gpf_p2p_connect': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    'gpf_p2p_set_timeout': (C.c_int, [C.c_void_p, C.c_double]),
    'gpf_upload_beyond': (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_size_t]),
    'gpf_stream_probe': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, _DP]),
    'gpf_step_p2p': (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    'gpf_stage_message': (C.c_int, [C.c_void_p]),
    'gpf_stage_absorb': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    'gpf_close_step_local': (C.c_int, [C.c_void_p]),
    'gpf_close_step_commit': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(GpfScalars)]),
    'gpf_set_seam_topo': (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_size_t]),
    'gpf_predictor_corrector': (C.c_int, [C.c_int, C.c_int, _DP, _DP, _DP, C.c_int, _DP, _DP]),
    'gpf_source': (C.c_int, [C.c_int, C.c_int, _DP, _DP, _DP, _DP, _DP, _DP]),
    'gpf_open_step': (C.c_int, [C.c_void_p]),
    'gpf_stage_closures': (C.c_int, [C.c_void_p]),
    'gpf_stage_advance': (C.c_int, [C.c_void_p, C.c_int]),
    'gpf_close_step': (C.c_int, [C.c_void_p, C.POINTER(GpfScalars)]),
    'gpf_gp_fit': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _DP, _DP, C.c_double, _DP, C.c_double, _DP, _DP, _DP]),
    'gpf_gp_set_model': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), _DP, _DP, _DP,
                                   C.c_double, _DP, C.c_double, C.c_double]),
    'gpf_gp_clear_model': (C.c_int, [C.c_void_p, C.c_int]),
    'gpf_gp_factorisation': (C.c_char_p, []),
    'gpf_plan_note': (C.c_char_p, [C.c_void_p]),
    'gpf_row_coefficients': (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_size_t]),
    'gpf_step_variant': (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    'gpf_gp_set_scales': (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_double]),
    'gpf_gp_variance': (C.c_int, [C.c_void_p, C.c_int, C.c_int, _DP]),
    'gpf_gp_pass_counts': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_gp_nll_open': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _DP, _DP, C.c_double, C.POINTER(C.c_void_p)]),
    'gpf_gp_nll_eval': (C.c_int, [C.c_void_p, _DP, _DP, _DP, C.POINTER(C.c_int)]),
    'gpf_gp_nll_close': (C.c_int, [C.c_void_p]),
    'gpf_gap_profiles_op': (C.c_int, [C.c_int64, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                                                                              C.c_void_p]),
    'gpf_gap_profiles': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'gpf_checkpoint_size': (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    'gpf_checkpoint_save': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    'gpf_checkpoint_load': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'gpf_checkpoint_pack_probe': (C.c_int, [C.c_void_p, C.c_int, _DP]),
    'gpf_profile_store_probe': (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, _DP]),
    'gpf_probes_set': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    'gpf_probes_clear': (C.c_int, [C.c_void_p]),
    'gpf_probes_read': (C.c_int, [C.c_void_p, _DP, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_probes_time': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_integrals_set': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32)]),
    'gpf_integrals_clear': (C.c_int, [C.c_void_p]),
    'gpf_integrals_read': (C.c_int, [C.c_void_p, _DP, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_integrals_now': (C.c_int, [C.c_void_p, _DP, C.c_int64]),
    'gpf_integrals_in_batch': (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    'gpf_integrals_time': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_weighted_set': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_weighted_clear': (C.c_int, [C.c_void_p]),
    'gpf_weighted_read': (C.c_int, [C.c_void_p, _DP, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_weighted_now': (C.c_int, [C.c_void_p, _DP, C.c_int64]),
    'gpf_weighted_time': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_extrema_set': (C.c_int, [C.c_void_p, C.c_int64]),
    'gpf_extrema_clear': (C.c_int, [C.c_void_p]),
    'gpf_extrema_read': (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_extrema_now': (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_int32)]),
    'gpf_extrema_time': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_slab_series_set': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32),
                                      C.c_int64]),
    'gpf_slab_series_clear': (C.c_int, [C.c_void_p]),
    'gpf_slab_series_message': (C.c_int, [C.c_void_p, _VPP, C.POINTER(C.c_size_t)]),
    'gpf_slab_series_begin': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'gpf_slab_series_local': (C.c_int, [C.c_void_p, C.c_int64]),
    'gpf_slab_series_fold': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64]),
    'gpf_slab_series_end': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    'gpf_slab_series_read': (C.c_int, [C.c_void_p, C.c_int, _DP, C.POINTER(C.c_int32), _DP, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_slab_series_now_local': (C.c_int, [C.c_void_p]),
    'gpf_slab_series_now_fold': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _DP, C.c_int64, _DP, C.POINTER(C.c_int32)]),
    'gpf_elastic_series_set': (C.c_int, [C.c_void_p, C.c_int64]),
    'gpf_elastic_series_clear': (C.c_int, [C.c_void_p]),
    'gpf_elastic_series_read': (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_elastic_series_now': (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_int32)]),
    'gpf_elastic_series_time': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_thinning_series_set': (C.c_int, [C.c_void_p, C.c_int64]),
    'gpf_thinning_series_clear': (C.c_int, [C.c_void_p]),
    'gpf_thinning_series_read': (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_thinning_series_now': (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_int32)]),
    'gpf_thinning_series_time': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_changes_set': (C.c_int, [C.c_void_p, C.c_int64]),
    'gpf_changes_clear': (C.c_int, [C.c_void_p]),
    'gpf_changes_read': (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_changes_now': (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_int32)]),
    'gpf_changes_time': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_stats_set': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int]),
    'gpf_stats_clear': (C.c_int, [C.c_void_p]),
    'gpf_stats_info': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _DP, _DP]),
    'gpf_stats_read': (C.c_int, [C.c_void_p, C.c_int, C.c_int, _DP, C.c_size_t]),
    'gpf_stats_time': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_regions_set': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(GpfRegion)]),
    'gpf_regions_clear': (C.c_int, [C.c_void_p]),
    'gpf_regions_read': (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_regions_now': (C.c_int, [C.c_void_p, _DP, C.POINTER(C.c_int64), C.c_int64]),
    'gpf_regions_time': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_lines_set': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(GpfLine), C.c_int64]),
    'gpf_lines_clear': (C.c_int, [C.c_void_p]),
    'gpf_lines_read': (C.c_int, [C.c_void_p, _DP, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_lines_now': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(GpfLine), _DP, C.c_int64]),
    'gpf_lines_time': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_frames_set': (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(GpfFrameSpec), C.c_int64]),
    'gpf_frames_clear': (C.c_int, [C.c_void_p]),
    'gpf_frames_read': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_frames_now': (C.c_int, [C.c_void_p, C.POINTER(GpfFrameSpec), C.c_void_p, C.c_int64]),
    'gpf_frames_shape': (C.c_int, [C.c_void_p, C.POINTER(GpfFrameSpec), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    'gpf_frames_time': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _DP]),
    'gpf_ensemble_create': (C.c_int, [_VPP, C.c_int, _VPP]),
    'gpf_ensemble_step': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64)]),
    'gpf_ensemble_log': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(GpfScalars), C.c_int64, C.POINTER(C.c_int64)]),
    'gpf_ensemble_destroy': (C.c_int, [C.c_void_p]),
    'gpf_ensemble_limits': (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    'gpf_ensemble_create2': (C.c_int, [_VPP, C.c_int, C.c_int, _VPP]),
    'gpf_ensemble_limits2': (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    'gpf_ensemble_member_info': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    'gpf_ensemble_integrals_set': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32)]),
    'gpf_ensemble_integrals_clear': (C.c_int, [C.c_void_p]),
    'gpf_ensemble_integrals_read': (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_ensemble_extrema_set': (C.c_int, [C.c_void_p, C.c_int64]),
    'gpf_ensemble_extrema_clear': (C.c_int, [C.c_void_p]),
    'gpf_ensemble_extrema_read': (C.c_int, [C.c_void_p, C.c_int, _DP, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_ensemble_probes_set': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    'gpf_ensemble_probes_clear': (C.c_int, [C.c_void_p]),
    'gpf_ensemble_probes_read': (C.c_int, [C.c_void_p, C.c_int, _DP, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'gpf_resample': (C.c_int, [C.c_void_p, C.c_void_p]),
    'gpf_resample_time': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _DP]),
}

_lib = None


class GapflowHipError(RuntimeError):
    pass


def _pin_hip_runtime():
    """Make sure ONE HIP runtime serves this process.

    PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Whichever copy is
    mapped first wins, and a process that maps /opt/rocm's first cannot initialise torch.cuda afterwards
    ("No HIP GPUs are available").  The slab path needs torch.distributed next to this library, so when
    torch is installed its bundled runtime is mapped first -- without importing torch."""
    import sys
    if os.environ.get('GPF_SYSTEM_HIP') == '1':
        return
    if 'torch' in sys.modules:
        libdir = os.path.join(os.path.dirname(sys.modules['torch'].__file__), 'lib')
        for var, name in (('GPF_ROCBLAS_PATH', 'librocblas.so'), ('GPF_HIPFFT_PATH', 'libhipfft.so')):
            if os.path.exists(os.path.join(libdir, name)):
                os.environ.setdefault(var, os.path.join(libdir, name))
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], 'lib')
    cand = os.path.join(libdir, 'libamdhip64.so')
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
        # rocBLAS (GP variance solve) must come from the same bundle, or a later `import torch` crashes
        for var, name in (('GPF_ROCBLAS_PATH', 'librocblas.so'), ('GPF_HIPFFT_PATH', 'libhipfft.so')):
            if os.path.exists(os.path.join(libdir, name)):
                os.environ.setdefault(var, os.path.join(libdir, name))


def _preload_rocsolver():
    """Unless GPF_USE_ROCSOLVER=0: map rocBLAS and the rocSOLVER that lies NEXT TO it now, before this process makes its first HIP
    call (rocSOLVER's dpotrf / dpotrs are the default factorisation of the GP kernel matrices).  Round 2 recorded a dlopen of rocSOLVER that did not return within 500 s when issued after the HIP runtime was up,
    and an abort when two rocBLAS images met (profiles/r03_rocsolver/README.md): the library itself only ever binds to
    images already mapped or to the copy beside its rocBLAS (csrc/gp_kernels.hip: roclibs), and this puts them there early."""
    if os.environ.get('GPF_USE_ROCSOLVER') == '0':
        return
    path = os.environ.get('GPF_ROCBLAS_PATH')
    try:
        blas = C.CDLL(path if path and os.path.exists(path) else 'librocblas.so.5', mode=C.RTLD_GLOBAL)
    except OSError:
        return                          # no rocBLAS here: the GP entry points will say so when they are called
    info = _DlInfo()
    libdl = C.CDLL(None)
    libdl.dladdr.argtypes, libdl.dladdr.restype = [C.c_void_p, C.POINTER(_DlInfo)], C.c_int
    if not libdl.dladdr(C.cast(blas.rocblas_create_handle, C.c_void_p), C.byref(info)) or not info.dli_fname:
        return
    here = os.path.dirname(info.dli_fname.decode())
    for name in ('librocsolver.so.0', 'librocsolver.so'):
        if os.path.exists(os.path.join(here, name)):
            try:
                C.CDLL(os.path.join(here, name), mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


class _DlInfo(C.Structure):
    _fields_ = [('dli_fname', C.c_char_p), ('dli_fbase', C.c_void_p), ('dli_sname', C.c_char_p), ('dli_saddr', C.c_void_p)]


def load():
    """Load libgapflow_hip.so once; raises if it has not been built (python -m gapflow_amd.build)."""
    global _lib
    if _lib is None:
        _pin_hip_runtime()
        _preload_rocsolver()
        if not os.path.exists(LIB_PATH):
            raise GapflowHipError(
                f"{LIB_PATH} not found: build it with `python -m gapflow_amd.build` (needs hipcc). "
                "gapflow_amd has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        lds, per_cell, steps = C.c_int64(SMALL_GRID_LDS_BYTES), C.c_int32(SMALL_GRID_DOUBLES_PER_CELL), C.c_int64(LOG_CAPACITY)
        if 'gpf_ensemble_limits' in SIGNATURES:     # (tools/ensemble_time.py --solo-only drops the ensemble entries to time an older build)
            lib.gpf_ensemble_limits(C.byref(lds), C.byref(per_cell), C.byref(steps))
        if (lds.value, per_cell.value, steps.value) != (SMALL_GRID_LDS_BYTES, SMALL_GRID_DOUBLES_PER_CELL, LOG_CAPACITY):
            raise GapflowHipError(f"{LIB_PATH} was built with other limits (LDS bytes, doubles per cell, log capacity) = "
                                  f"{(lds.value, per_cell.value, steps.value)} than gapflow_amd/_lib.py states")
        mid_cells, mid_per_cell = C.c_int64(MID_GRID_MAX_CELLS), C.c_int32(MID_GRID_DOUBLES_PER_CELL)
        if 'gpf_ensemble_limits2' in SIGNATURES:
            lib.gpf_ensemble_limits2(C.byref(mid_cells), C.byref(mid_per_cell))
        if (mid_cells.value, mid_per_cell.value) != (MID_GRID_MAX_CELLS, MID_GRID_DOUBLES_PER_CELL):
            raise GapflowHipError(f"{LIB_PATH} was built with other workspace-tier limits (cells, doubles per cell) = "
                                  f"{(mid_cells.value, mid_per_cell.value)} than gapflow_amd/_lib.py states")
        _lib = lib
    return _lib


def check(code):
    if code != 0:
        raise GapflowHipError(f"libgapflow_hip error {code}: {load().gpf_last_error().decode()}")


def require_device():
    lib = load()
    if lib.gpf_device_count() < 1:
        raise GapflowHipError("no HIP device visible: gapflow_amd runs its hot path on an MI355X only "
                              "(there is no CPU fallback)")
    return lib


def as_dp(a):
    return a.ctypes.data_as(_DP)


def f64c(a):
    return np.ascontiguousarray(a, dtype=np.float64)
