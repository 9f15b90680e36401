"""ctypes binding of libdqmc_hip.so (include/dqmc_hip.h).

The product path has no CPU fallback: if the HIP library is missing or cannot be
loaded, importing the symbols fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DQMC_HIP_LIB selects another build of the same library (diagnostic / A-B builds), never a fallback
LIB_PATH = os.environ.get("DQMC_HIP_LIB") or os.path.join(_HERE, "libdqmc_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dqmc_hip.h")

OK, ERR_INVALID, ERR_HIP, ERR_NO_DEVICE, ERR_STATE, ERR_RNG = 0, -1, -2, -3, -4, -5
ATTRACTIVE, REPULSIVE = 0, 1
BIN_SECTIONS = ("greens", "correlations", "pairing", "susceptibilities", "user")  # DQMC_BIN_*
BIN_TIME_DISPLACED, RED_TIME_DISPLACED = 5, 4  # DQMC_BIN_TIME_DISPLACED, DQMC_RED_TIME_DISPLACED (enums of their own)
TD_GREENS, TD_DENSITY = 1, 2                   # DQMC_TD_*
BIN_SIGN, RED_SIGN = 6, 5                      # DQMC_BIN_SIGN (+ a section's DQMC_RED_* index), DQMC_RED_SIGN
# DQMC_BIN_MOMENTUM_*: the momentum-space binners, above every other DQMC_BIN_* value
BIN_MOMENTUM = {"momentum_correlations": 11, "momentum_susceptibilities": 12, "momentum_time_displaced": 13}
RED_THERMODYNAMICS, BIN_THERMODYNAMICS = 6, 14  # DQMC_RED_THERMODYNAMICS, DQMC_BIN_THERMODYNAMICS
# DQMC_BIN_RESPONSE_*: the pair-channel and current response binners, behind the thermodynamics one
BIN_RESPONSE = {"response_pairing": 15, "response_pairing_susceptibility": 16, "response_current": 17}
# the elements of a thermodynamics sample, in the order of include/dqmc_hip.h (DQMC_THERMO_ELEMENTS of them)
THERMO_FIELDS = ("n_up", "n_dn", "n", "D", "m2", "E_kin", "E_int", "E", "N2", "Mz2")
ENT_MAX_SITES, ENT_MAX_SUBSYSTEMS = 128, 64  # DQMC_ENT_MAX_SITES, DQMC_ENT_MAX_SUBSYSTEMS
K_FAMILIES = ("gemm", "qr", "trsm", "sweep", "misc", "flush")


class DQMCError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libdqmc_hip error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [
        ("n_sites", C.c_int32), ("model_kind", C.c_int32), ("slices", C.c_int32), ("safe_mult", C.c_int32),
        ("n_walkers", C.c_int32), ("device_id", C.c_int32), ("check_propagation_error", C.c_int32),
        ("check_sign_problem", C.c_int32), ("delta_tau", C.c_double), ("U", C.c_double),
        ("eT", C.POINTER(C.c_double)), ("eTinv", C.POINTER(C.c_double)), ("eT2", C.POINTER(C.c_double)),
        ("eTinv2", C.POINTER(C.c_double)),
    ]


class MagStats(C.Structure):
    _fields_ = [("max", C.c_double), ("min", C.c_double), ("sum", C.c_double), ("count", C.c_int64)]


class Stats(C.Structure):
    _fields_ = [("prop_local", C.c_int64), ("acc_local", C.c_int64), ("imaginary_probability", MagStats),
                ("negative_probability", MagStats), ("propagation_error", MagStats)]


class GlobalStats(C.Structure):
    _fields_ = [("prop_global", C.c_int64), ("acc_global", C.c_int64), ("moves_drawn", C.c_uint64)]


GLOBAL_KINDS = ("all", "site")  # DQMC_GLOBAL_FLIP_ALL, DQMC_GLOBAL_FLIP_SITE


class McParams(C.Structure):
    _fields_ = [("n_sites", C.c_int32), ("z", C.c_int32), ("n_walkers", C.c_int32), ("device_id", C.c_int32),
                ("n_bonds", C.c_int32), ("series_capacity", C.c_int32), ("neighs", C.POINTER(C.c_int64)),
                ("bonds", C.POINTER(C.c_int64))]


class McStats(C.Structure):
    _fields_ = [("energy", C.c_int64), ("magnetization", C.c_int64), ("sum_E", C.c_double), ("sum_E2", C.c_double),
                ("sum_absM", C.c_double), ("sum_M2", C.c_double), ("n_meas", C.c_int64), ("prop_local", C.c_int64),
                ("acc_local", C.c_int64), ("uniforms_used", C.c_uint64), ("n_series", C.c_int64)]


class McGlobalStats(C.Structure):
    _fields_ = [("prop_global", C.c_int64), ("acc_global", C.c_int64), ("sum_cluster_size", C.c_int64),
                ("moves_drawn", C.c_uint64)]


class McExchangeStats(C.Structure):
    _fields_ = [("prop_exchange", C.c_int64), ("acc_exchange", C.c_int64), ("replica", C.c_int64),
                ("rounds", C.c_uint64)]


class McUpdateStats(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_colours", C.c_int32), ("sweeps_drawn", C.c_uint64)]


MC_UPDATE_KINDS = ("sequential", "checkerboard")  # DQMC_MC_UPDATE_*


class McBinned(C.Structure):
    _fields_ = [("mean", C.c_double * 4), ("varN", C.c_double * 4), ("varN0", C.c_double * 4), ("tau", C.c_double * 4),
                ("covN", C.c_double * 2), ("count", C.c_int64), ("level", C.c_int32)]


class McFss(C.Structure):
    _fields_ = [("n_meas", C.c_int64), ("n_k", C.c_int32), ("sum_M4", C.c_double), ("sum_S", C.c_double * 8)]


class McFssBinned(C.Structure):
    _fields_ = [("mean", C.c_double * 10), ("varN", C.c_double * 10), ("varN0", C.c_double * 10),
                ("tau", C.c_double * 10), ("covN", C.c_double * 9), ("count", C.c_int64), ("level", C.c_int32),
                ("n_k", C.c_int32)]


class QsParams(C.Structure):
    _fields_ = [("n_sites", C.c_int32), ("z", C.c_int32), ("q", C.c_int32), ("n_walkers", C.c_int32),
                ("device_id", C.c_int32), ("n_bonds", C.c_int32), ("series_capacity", C.c_int32),
                ("n_colours", C.c_int32), ("neighs", C.POINTER(C.c_int64)), ("bonds", C.POINTER(C.c_int64)),
                ("e_q30", C.POINTER(C.c_int64)), ("c_q30", C.POINTER(C.c_int32)), ("s_q30", C.POINTER(C.c_int32)),
                ("colour", C.POINTER(C.c_int32))]


class QsStats(C.Structure):
    _fields_ = [("energy_q30", C.c_int64), ("mx_q30", C.c_int64), ("my_q30", C.c_int64), ("sum_E", C.c_double),
                ("sum_E2", C.c_double), ("sum_absM", C.c_double), ("sum_M2", C.c_double), ("sum_M4", C.c_double),
                ("n_meas", C.c_int64), ("prop_local", C.c_int64), ("acc_local", C.c_int64),
                ("sweeps_drawn", C.c_uint64), ("confs_drawn", C.c_uint64), ("n_series", C.c_int64),
                ("n_colours", C.c_int32)]


class QsClusterStats(C.Structure):
    _fields_ = [("prop_global", C.c_int64), ("acc_global", C.c_int64), ("sum_cluster_size", C.c_int64),
                ("moves_drawn", C.c_uint64)]


class QsExchangeStats(C.Structure):
    _fields_ = [("prop_exchange", C.c_int64), ("acc_exchange", C.c_int64), ("replica", C.c_int64),
                ("rounds", C.c_uint64)]


class QsBinned(C.Structure):
    _fields_ = [("mean", C.c_double * 6), ("varN", C.c_double * 6), ("varN0", C.c_double * 6), ("tau", C.c_double * 6),
                ("covN", C.c_double * 3), ("count", C.c_int64), ("level", C.c_int32)]


class QsScaling(C.Structure):
    _fields_ = [("n_meas", C.c_int64), ("n_k", C.c_int32), ("sum_S", C.c_double * 8)]


class QsScalingBinned(C.Structure):
    _fields_ = [("mean", C.c_double * 9), ("varN", C.c_double * 9), ("varN0", C.c_double * 9), ("tau", C.c_double * 9),
                ("covN", C.c_double * 8), ("count", C.c_int64), ("level", C.c_int32), ("n_k", C.c_int32)]


class QsStiffness(C.Structure):
    _fields_ = [("n_meas", C.c_int64), ("n_dir", C.c_int32), ("sum_T", C.c_double * 4), ("sum_J", C.c_double * 4),
                ("sum_J2", C.c_double * 4)]


class QsStiffnessBinned(C.Structure):
    _fields_ = [("mean", C.c_double * 8), ("varN", C.c_double * 8), ("varN0", C.c_double * 8), ("tau", C.c_double * 8),
                ("covN", C.c_double * 4), ("count", C.c_int64), ("level", C.c_int32), ("n_dir", C.c_int32)]


class SacParams(C.Structure):
    _fields_ = [("n_problems", C.c_int32), ("n_tau", C.c_int32), ("n_deltas", C.c_int32), ("n_omega", C.c_int32),
                ("n_replicas", C.c_int32), ("device_id", C.c_int32), ("window", C.c_int32),
                ("theta", C.POINTER(C.c_double))]


class SacStats(C.Structure):
    _fields_ = [("chi2", C.c_double), ("sum_chi2", C.c_double), ("sum_chi2_sq", C.c_double), ("min_chi2", C.c_double),
                ("max_drift", C.c_double), ("n_meas", C.c_int64), ("prop", C.c_int64), ("acc", C.c_int64),
                ("prop_exchange", C.c_int64), ("acc_exchange", C.c_int64), ("replica", C.c_int64),
                ("moves_drawn", C.c_uint64), ("rounds", C.c_uint64), ("window", C.c_int32)]


_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)
_H = C.c_void_p

# name -> (restype, argtypes); every symbol declared in include/dqmc_hip.h
SIGNATURES = {
    "dqmc_create": (C.c_int, [C.POINTER(Params), C.POINTER(_H)]),
    "dqmc_destroy": (C.c_int, [_H]),
    "dqmc_last_error": (C.c_char_p, [_H]),
    "dqmc_device_count": (C.c_int, []),
    "dqmc_set_conf": (C.c_int, [_H, C.c_int32, C.c_void_p]),
    "dqmc_get_conf": (C.c_int, [_H, C.c_int32, C.c_void_p]),
    "dqmc_get_conf_bits": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_uint64)]),
    "dqmc_set_conf_bits": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_uint64)]),
    "dqmc_set_uniforms": (C.c_int, [_H, C.c_int32, _dp, C.c_size_t]),
    "dqmc_seed": (C.c_int, [_H, C.c_int32, C.c_uint64]),
    "dqmc_uniforms_used": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_uint64)]),
    "dqmc_get_state": (C.c_int, [_H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "dqmc_prepare": (C.c_int, [_H]),
    "dqmc_build_stack": (C.c_int, [_H]),
    "dqmc_propagate": (C.c_int, [_H]),
    "dqmc_sweep_spatial": (C.c_int, [_H]),
    "dqmc_update": (C.c_int, [_H]),
    "dqmc_sweep": (C.c_int, [_H, C.c_int32]),
    "dqmc_update_until_measure": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_synchronize": (C.c_int, [_H]),
    "dqmc_get_greens_eff": (C.c_int, [_H, C.c_int32, _dp]),
    "dqmc_set_greens_eff": (C.c_int, [_H, C.c_int32, _dp]),
    "dqmc_get_greens": (C.c_int, [_H, C.c_int32, _dp]),
    "dqmc_calculate_greens_at": (C.c_int, [_H, C.c_int32, C.c_int32, _dp]),
    "dqmc_replay_greens": (C.c_int, [_H, C.c_int32]),
    "dqmc_wrap_greens": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "dqmc_get_stats": (C.c_int, [_H, C.c_int32, C.POINTER(Stats)]),
    "dqmc_logdet": (C.c_int, [_H, _dp, C.POINTER(C.c_int32)]),
    "dqmc_global_move": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "dqmc_set_global_rate": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "dqmc_get_global_stats": (C.c_int, [_H, C.c_int32, C.POINTER(GlobalStats)]),
    "dqmc_set_sign_weighting": (C.c_int, [_H, C.c_int32]),
    "dqmc_get_sign_weighting": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_get_sign": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_get_sign_failures": (C.c_int, [_H, _i64p]),
    "dqmc_sign_sums_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_get_sign_sums": (C.c_int, [_H, _dp]),
    "dqmc_export_sign_sums": (C.c_int, [_H, C.c_void_p]),
    "dqmc_accumulate_greens": (C.c_int, [_H]),
    "dqmc_accumulator_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_reset_accumulators": (C.c_int, [_H]),
    "dqmc_get_accumulators": (C.c_int, [_H, _dp]),
    "dqmc_export_accumulators": (C.c_int, [_H, C.c_void_p]),
    "dqmc_set_pair_directions": (C.c_int, [_H, C.POINTER(C.c_int32), C.c_int32]),
    "dqmc_accumulate_correlations": (C.c_int, [_H]),
    "dqmc_correlations_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_get_correlations": (C.c_int, [_H, _dp]),
    "dqmc_export_correlations": (C.c_int, [_H, C.c_void_p]),
    "dqmc_set_local_targets": (C.c_int, [_H, C.POINTER(C.c_int32), C.c_int32]),
    "dqmc_accumulate_pairing": (C.c_int, [_H]),
    "dqmc_pairing_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_get_pairing": (C.c_int, [_H, _dp]),
    "dqmc_export_pairing": (C.c_int, [_H, C.c_void_p]),
    "dqmc_ut_build_stack": (C.c_int, [_H]),
    "dqmc_ut_get_stack": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "dqmc_ut_greens": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32]),
    "dqmc_ut_get": (C.c_int, [_H, C.c_int32, C.c_int32, _dp]),
    "dqmc_ut_export": (C.c_int, [_H, C.c_int32, C.c_void_p]),
    "dqmc_greens_iterator_begin": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "dqmc_greens_iterator_next": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_combined_iterator_begin": (C.c_int, [_H, C.c_int32]),
    "dqmc_combined_iterator_next": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_accumulate_susceptibilities": (C.c_int, [_H, C.c_int32]),
    "dqmc_set_current_targets": (C.c_int, [_H, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_double)]),
    "dqmc_current_targets_fast_path": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_current_targets_plan": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_set_time_displaced": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "dqmc_time_displaced_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_get_time_displaced": (C.c_int, [_H, _dp]),
    "dqmc_export_time_displaced": (C.c_int, [_H, C.c_void_p]),
    "dqmc_time_displaced_plan": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_susceptibilities_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_get_susceptibilities": (C.c_int, [_H, _dp]),
    "dqmc_export_susceptibilities": (C.c_int, [_H, C.c_void_p]),
    "dqmc_binner_enable": (C.c_int, [_H, C.c_int32, C.c_int64]),
    "dqmc_binner_size": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_int32), _i64p]),
    "dqmc_binner_reliable_level": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32)]),
    "dqmc_binner_get_level": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _i64p]),
    "dqmc_binner_finish": (C.c_int, [_H, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]),
    "dqmc_binner_export_moments": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p]),
    "dqmc_binner_user_create": (C.c_int, [_H, C.c_int64, C.c_int64]),
    "dqmc_binner_user_push": (C.c_int, [_H, C.c_void_p]),
    "dqmc_set_momenta": (C.c_int, [_H, C.c_int32, _dp, _dp]),
    "dqmc_momenta_plan": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_set_tau_covariance": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "dqmc_tau_covariance_plan": (C.c_int, [_H, _i64p]),
    "dqmc_tau_covariance_get": (C.c_int, [_H, _i64p, _dp, _dp, _dp]),
    "dqmc_user_covariance": (C.c_int, [_H, C.c_int64, C.c_int32, C.c_int32]),
    "dqmc_user_covariance_push": (C.c_int, [_H, C.c_void_p]),
    "dqmc_user_covariance_plan": (C.c_int, [_H, _i64p]),
    "dqmc_user_covariance_get": (C.c_int, [_H, _i64p, _dp, _dp, _dp]),
    "dqmc_set_pair_channels":(C.c_int, [_H, C.c_int32, _dp]),
    "dqmc_response_plan": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_set_thermodynamics": (C.c_int, [_H, _dp]),
    "dqmc_accumulate_thermodynamics": (C.c_int, [_H]),
    "dqmc_thermodynamics_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_get_thermodynamics": (C.c_int, [_H, _dp]),
    "dqmc_export_thermodynamics": (C.c_int, [_H, C.c_void_p]),
    "dqmc_set_entanglement": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "dqmc_entanglement_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_accumulate_entanglement": (C.c_int, [_H]),
    "dqmc_get_entanglement": (C.c_int, [_H, _dp, C.c_size_t]),
    "dqmc_get_entanglement_sample": (C.c_int, [_H, _dp, C.c_size_t]),
    "dqmc_set_entanglement_sums": (C.c_int, [_H, _dp, C.c_size_t]),
    "dqmc_set_current_time_displaced": (C.c_int, [_H, C.c_int32]),
    "dqmc_current_time_displaced_plan": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_current_time_displaced_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_get_current_time_displaced": (C.c_int, [_H, _dp]),
    "dqmc_set_current_time_displaced_sums": (C.c_int, [_H, _dp]),
    "dqmc_comm_unique_id": (C.c_int, [C.c_void_p]),
    "dqmc_comm_init": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_H)]),
    "dqmc_comm_destroy": (C.c_int, [_H]),
    "dqmc_reduce": (C.c_int, [_H, _H]),
    "dqmc_reduce_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_reduce_export": (C.c_int, [_H, _dp]),
    "dqmc_reduce_import": (C.c_int, [_H, _dp]),
    "dqmc_get_reduced": (C.c_int, [_H, C.c_int32, _dp]),
    "dqmc_get_reduced_stats": (C.c_int, [_H, C.POINTER(Stats)]),
    "dqmc_state_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_state_export": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "dqmc_state_import": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "dqmc_vmul": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp]),
    "dqmc_udt_pivot": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, _i64p, C.c_int32]),
    "dqmc_logdet_matrices": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int64, _dp, C.c_int64, _dp,
                             C.POINTER(C.c_int32)]),
    "dqmc_impose_unit_signs": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_rdivp": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _i64p]),
    "dqmc_calculate_greens": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "dqmc_set_checkerboard": (C.c_int, [_H, C.c_int32, C.c_int32, _dp, C.POINTER(C.c_int32), _dp, _dp,
                              C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "dqmc_checkerboard_plan": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_checkerboard_apply": (C.c_int, [_H, C.c_int32, C.c_int32, _dp, _dp, C.c_int32, _dp]),
    "dqmc_qr_fallbacks": (C.c_int, [_H, C.POINTER(C.c_int64)]),
    "dqmc_kron_hopping": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_set_triangular_factors": (C.c_int, [_H, _dp]),
    "dqmc_set_square_tp_factors": (C.c_int, [_H, _dp]),
    "dqmc_device_errors": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_udt_one_launch_sites": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_launch_plan": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_build_commit": (C.c_char_p, []),
    "dqmc_build_source_hash": (C.c_char_p, []),
    "dqmc_get_global_last": (C.c_int, [_H, C.c_int32, _dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "dqmc_mc_create": (C.c_int, [C.POINTER(McParams), C.POINTER(_H)]),
    "dqmc_mc_destroy": (C.c_int, [_H]),
    "dqmc_mc_last_error": (C.c_char_p, [_H]),
    "dqmc_mc_set_beta": (C.c_int, [_H, C.c_int32, C.c_double]),
    "dqmc_mc_seed": (C.c_int, [_H, C.c_int32, C.c_uint64]),
    "dqmc_mc_rand_conf": (C.c_int, [_H, C.c_int32]),
    "dqmc_mc_set_conf": (C.c_int, [_H, C.c_int32, C.c_void_p]),
    "dqmc_mc_get_conf": (C.c_int, [_H, C.c_int32, C.c_void_p]),
    "dqmc_mc_get_conf_bits": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_uint64)]),
    "dqmc_mc_sweep": (C.c_int, [_H, C.c_int32, C.c_int64, C.c_int64, C.c_int32]),
    "dqmc_mc_get_stats": (C.c_int, [_H, C.c_int32, C.POINTER(McStats)]),
    "dqmc_mc_get_series": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                           C.POINTER(C.c_int64)]),
    "dqmc_mc_reset_accumulators": (C.c_int, [_H]),
    "dqmc_mc_set_global_rate": (C.c_int, [_H, C.c_int32]),
    "dqmc_mc_global_move": (C.c_int, [_H, C.c_int32]),
    "dqmc_mc_get_global_stats": (C.c_int, [_H, C.c_int32, C.POINTER(McGlobalStats)]),
    "dqmc_mc_set_exchange": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "dqmc_mc_exchange": (C.c_int, [_H]),
    "dqmc_mc_get_exchange_stats": (C.c_int, [_H, C.c_int32, C.POINTER(McExchangeStats)]),
    "dqmc_mc_exchange_fused": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_mc_set_update": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "dqmc_mc_get_update": (C.c_int, [_H, C.c_int32, C.POINTER(McUpdateStats)]),
    "dqmc_mc_synchronize": (C.c_int, [_H]),
    "dqmc_mc_binner_enable": (C.c_int, [_H, C.c_int64]),
    "dqmc_mc_binner_size": (C.c_int, [_H, C.POINTER(C.c_int32), _i64p]),
    "dqmc_mc_binner_reliable_level": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_mc_binner_get_level": (C.c_int, [_H, C.c_int32, C.c_int32, _dp, _dp, _dp, _i64p]),
    "dqmc_mc_binner_finish": (C.c_int, [_H, C.c_int32, C.c_int32, C.POINTER(McBinned)]),
    "dqmc_mc_set_fss": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "dqmc_mc_get_fss": (C.c_int, [_H, C.c_int32, C.POINTER(McFss)]),
    "dqmc_mc_fss_binner_get_level": (C.c_int, [_H, C.c_int32, C.c_int32, _dp, _dp, _dp, _i64p]),
    "dqmc_mc_fss_binner_finish": (C.c_int, [_H, C.c_int32, C.c_int32, C.POINTER(McFssBinned)]),
    "dqmc_mc_state_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_mc_state_export": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "dqmc_mc_state_import": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "dqmc_qs_state_size": (C.c_int, [_H, C.POINTER(C.c_size_t)]),
    "dqmc_qs_state_export": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "dqmc_qs_state_import": (C.c_int, [_H, C.c_void_p, C.c_size_t]),
    "dqmc_qs_create": (C.c_int, [C.POINTER(QsParams), C.POINTER(_H)]),
    "dqmc_qs_destroy": (C.c_int, [_H]),
    "dqmc_qs_last_error": (C.c_char_p, [_H]),
    "dqmc_qs_seed": (C.c_int, [_H, C.c_int32, C.c_uint64]),
    "dqmc_qs_set_beta": (C.c_int, [_H, C.c_int32, C.c_double]),
    "dqmc_qs_rand_conf": (C.c_int, [_H, C.c_int32]),
    "dqmc_qs_set_conf": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_uint8)]),
    "dqmc_qs_get_conf": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_uint8)]),
    "dqmc_qs_set_colouring": (C.c_int, [_H, C.POINTER(C.c_int32), C.c_int32]),
    "dqmc_qs_sweep": (C.c_int, [_H, C.c_int32, C.c_int64, C.c_int64, C.c_int32]),
    "dqmc_qs_get_stats": (C.c_int, [_H, C.c_int32, C.POINTER(QsStats)]),
    "dqmc_qs_get_series": (C.c_int, [_H, C.c_int32, _i64p, _i64p, _i64p, _i64p]),
    "dqmc_qs_reset_accumulators": (C.c_int, [_H]),
    "dqmc_qs_synchronize": (C.c_int, [_H]),
    "dqmc_qs_set_cluster_rate": (C.c_int, [_H, C.c_int32]),
    "dqmc_qs_cluster_move": (C.c_int, [_H, C.c_int32]),
    "dqmc_qs_get_cluster_stats": (C.c_int, [_H, C.c_int32, C.POINTER(QsClusterStats)]),
    "dqmc_qs_set_exchange": (C.c_int, [_H, C.c_int32, C.c_int32]),
    "dqmc_qs_exchange": (C.c_int, [_H]),
    "dqmc_qs_get_exchange_stats": (C.c_int, [_H, C.c_int32, C.POINTER(QsExchangeStats)]),
    "dqmc_qs_binner_enable": (C.c_int, [_H, C.c_int64]),
    "dqmc_qs_binner_size": (C.c_int, [_H, C.POINTER(C.c_int32), _i64p]),
    "dqmc_qs_binner_reliable_level": (C.c_int, [_H, C.POINTER(C.c_int32)]),
    "dqmc_qs_binner_get_level": (C.c_int, [_H, C.c_int32, C.c_int32, _dp, _dp, _dp, _i64p]),
    "dqmc_qs_binner_finish": (C.c_int, [_H, C.c_int32, C.c_int32, C.POINTER(QsBinned)]),
    "dqmc_qs_set_scaling": (C.c_int, [_H, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "dqmc_qs_get_scaling": (C.c_int, [_H, C.c_int32, C.POINTER(QsScaling)]),
    "dqmc_qs_scaling_binner_get_level": (C.c_int, [_H, C.c_int32, C.c_int32, _dp, _dp, _dp, _i64p]),
    "dqmc_qs_scaling_binner_finish": (C.c_int, [_H, C.c_int32, C.c_int32, C.POINTER(QsScalingBinned)]),
    "dqmc_qs_set_stiffness": (C.c_int, [_H, C.c_int32, C.c_int32, C.POINTER(C.c_int8), _i64p, _i64p, _dp]),
    "dqmc_qs_get_stiffness": (C.c_int, [_H, C.c_int32, C.POINTER(QsStiffness)]),
    "dqmc_qs_get_stiffness_sample": (C.c_int, [_H, C.c_int32, _i64p, _i64p]),
    "dqmc_qs_stiffness_binner_get_level": (C.c_int, [_H, C.c_int32, C.c_int32, _dp, _dp, _dp, _i64p]),
    "dqmc_qs_stiffness_binner_finish": (C.c_int, [_H, C.c_int32, C.c_int32, C.POINTER(QsStiffnessBinned)]),
    "dqmc_sac_create": (C.c_int, [C.POINTER(SacParams), C.POINTER(_H)]),
    "dqmc_sac_destroy": (C.c_int, [_H]),
    "dqmc_sac_last_error": (C.c_char_p, [_H]),
    "dqmc_sac_set_problem": (C.c_int, [_H, C.c_int32, _dp, _dp, _dp, C.c_double]),
    "dqmc_sac_set_theta": (C.c_int, [_H, C.c_int32, _dp]),
    "dqmc_sac_seed": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_uint64]),
    "dqmc_sac_set_conf": (C.c_int, [_H, C.c_int32, C.c_int32, C.POINTER(C.c_uint16)]),
    "dqmc_sac_get_conf": (C.c_int, [_H, C.c_int32, C.c_int32, C.POINTER(C.c_uint16)]),
    "dqmc_sac_set_window": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32]),
    "dqmc_sac_set_exchange": (C.c_int, [_H, C.c_int32]),
    "dqmc_sac_sweep": (C.c_int, [_H, C.c_int32, C.c_int64, C.c_int64, C.c_int32]),
    "dqmc_sac_get_stats": (C.c_int, [_H, C.c_int32, C.c_int32, C.POINTER(SacStats)]),
    "dqmc_sac_get_histogram": (C.c_int, [_H, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]),
    "dqmc_sac_reset_accumulators": (C.c_int, [_H]),
    "dqmc_timing_enable": (C.c_int, [_H, C.c_int32]),
    "dqmc_timing_get": (C.c_int, [_H, _dp, _i64p]),
    "dqmc_mfma_f64_peak": (C.c_int, [C.c_int32, C.c_int32, _dp]),
}

_lib = None


def lib():
    """Load libdqmc_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libdqmc_hip.so not found at %s — build it with __graft_entry__.build() "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)  # AttributeError if the export is missing
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(rc, handle=None):
    if rc != 0:
        msg = lib().dqmc_last_error(handle)
        raise DQMCError(rc, msg.decode() if msg else "")


def dptr(a):
    return a.ctypes.data_as(_dp)


def i64ptr(a):
    return a.ctypes.data_as(_i64p)
