"""ctypes binding of libhedgehog_mc.so (include/hedgehog_mc.h).

The product path has no CPU fallback: if the HIP library is missing or no HIP device is present,
every compute call raises `HedgehogMCError`.
"""
from __future__ import annotations

import ctypes as C
import os

HH_MAX_PARTIALS = 8
HH_LSM_PHASE_POW, HH_LSM_PHASE_INIT, HH_LSM_PHASE_STEP = 1, 2, 3
HH_TILE_PATHS = 256
HH_ACC_LEN = 16
HH_MAX_MODELS = 16
HH_ACC_SUM, HH_ACC_SUMSQ, HH_ACC_DSUM, HH_ACC_NPATHS = 0, 1, 2, 10

HH_LOGNORMAL, HH_HESTON = 0, 1
HH_EULER_MARUYAMA, HH_EXACT_LAW, HH_BROADIE_KAYA, HH_QE = 0, 1, 2, 3
HH_NOISE_GENERATE, HH_NOISE_REPLAY = 0, 1
HH_REPLAY_TILE_MAJOR, HH_REPLAY_PATH_MAJOR = 0, 1
HH_PATH_SPOT, HH_PATH_LOG = 0, 1
HH_PAYOFF_VANILLA, HH_PAYOFF_ASIAN_ARITH, HH_PAYOFF_ASIAN_GEOM = 0, 1, 2
HH_PAYOFF_BARRIER, HH_PAYOFF_DIGITAL_CASH, HH_PAYOFF_DIGITAL_ASSET = 3, 4, 5
HH_BARRIER_UP_OUT, HH_BARRIER_UP_IN, HH_BARRIER_DOWN_OUT, HH_BARRIER_DOWN_IN = 0, 1, 2, 3
HH_STAT_SUM_S, HH_STAT_SUM_X, HH_STAT_MAX_S, HH_STAT_MIN_S, HH_STAT_S_T = 0, 1, 2, 3, 4
HH_PAYOFF_LOOKBACK_FLOAT, HH_PAYOFF_LOOKBACK_FIXED = 6, 7
HH_STAT_CMAX_S, HH_STAT_CMIN_S = 5, 6
HH_EXTREMES_MONITORED, HH_EXTREMES_BRIDGE = 0, 1
HH_PATH_STATS = 5
HH_PATH_STATS_BRIDGE = 7
HH_TANGENT_K_MAX, HH_TANGENT_K_MIN, HH_TANGENT_SUM_KS = 5, 6, 7  # enum hh_tangent_date_row
HH_TANGENT_DSUM_S, HH_TANGENT_DSUM_X, HH_TANGENT_DMAX_S, HH_TANGENT_DMIN_S, HH_TANGENT_DS_T = 0, 1, 2, 3, 4
HH_BASIS_V0, HH_BASIS_KAPPA, HH_BASIS_THETA, HH_BASIS_SIGMA = 0, 1, 2, 3
HH_TANGENT_DATE_ROWS, HH_TANGENT_ROWS_PER_SLOT, HH_TANGENT_MAX_BASIS = 3, 5, 4
HH_MAX_PATH_PAYOFFS = 1024
HH_JUMP_MAX_MEAN = 64.0
HH_JUMP_MAX_COUNT = 255
HH_VG_MAX_ATTEMPTS = 64
HH_QE_MAX_PSI = 1e9
HH_MAX_ASSETS = 8
HH_LV_MAX_NODES = 8192
HH_INDEX_WEIGHTED_SUM, HH_INDEX_GEOMETRIC, HH_INDEX_BEST_OF, HH_INDEX_WORST_OF = 0, 1, 2, 3
HH_SOBOL_MAX_DIMS = 4096
HH_SOBOL_INCREMENTAL, HH_SOBOL_BRIDGE = 0, 1

HH_OK, HH_ERR_INVALID, HH_ERR_UNSUPPORTED, HH_ERR_HIP, HH_ERR_NOMEM, HH_ERR_RCCL, HH_ERR_DEVICE_TIMEOUT = 0, -1, -2, -3, -4, -5, -6
HH_MGPU_AUTO, HH_MGPU_HOST_SUM, HH_MGPU_RCCL = 0, 1, 2
HH_MGPU_REDUCE_HOST, HH_MGPU_REDUCE_RCCL = 0, 1
HH_MGPU_OPT_ENQUEUE = 1
HH_MGPU_ENQUEUE_SERIAL, HH_MGPU_ENQUEUE_THREADS = 0, 1

_dp = C.POINTER(C.c_double)


class hh_model(C.Structure):
    _fields_ = [(n, C.c_double) for n in
                ("S0", "V0", "kappa", "theta", "sigma", "rho", "r_drift", "discount", "T", "strike",
                 "cp")] + \
               [(n, _dp) for n in
                ("dS0", "dV0", "dkappa", "dtheta", "dsigma", "dr_drift", "ddiscount", "dstrike")]


class hh_config(C.Structure):
    _fields_ = [
        ("dynamics", C.c_int32), ("strategy", C.c_int32), ("antithetic", C.c_int32),
        ("em_split", C.c_int32), ("compat_sqrt_alpha", C.c_int32), ("noise_mode", C.c_int32),
        ("replay_layout", C.c_int32), ("seeds_on_device", C.c_int32),
        ("replay_on_device", C.c_int32), ("terminal_on_device", C.c_int32),
        ("n_steps", C.c_uint32), ("n_partials", C.c_uint32),
        ("n_paths", C.c_uint64), ("path_offset", C.c_uint64),
        ("seeds", C.c_void_p), ("replay", C.c_void_p),
        ("bk_n_sigma", C.c_double), ("bk_cf_tol", C.c_double), ("bk_atol", C.c_double),
        ("bk_moment_h", C.c_double),
        ("bk_newton_maxiter", C.c_int32), ("bk_bisect_maxiter", C.c_int32),
        ("bk_root_form", C.c_int32), ("bk_bracket_form", C.c_int32), ("bk_caps", C.c_int32), ("reserved0", C.c_int32),
        ("seeds_len", C.c_uint64), ("replay_len", C.c_uint64),
    ]


class hh_result(C.Structure):
    _fields_ = [
        ("price", C.c_double), ("std_error", C.c_double),
        ("sum_payoff", C.c_double), ("sumsq_payoff", C.c_double),
        ("dprice", C.c_double * HH_MAX_PARTIALS),
        ("n_paths_done", C.c_uint64),
        ("bk_newton_fail", C.c_uint64), ("bk_bisect_fallback", C.c_uint64),
        ("bk_maxguess_fallback", C.c_uint64), ("bk_cf_terms", C.c_uint64),
        ("kernel_ms", C.c_double), ("total_ms", C.c_double),
    ]


class hh_lsm_result(C.Structure):
    _fields_ = [("price", C.c_double), ("std_error", C.c_double), ("n_paths_total", C.c_uint64),
                ("rows_regressed", C.c_uint32), ("rows_skipped", C.c_uint32),
                ("kernel_ms", C.c_double), ("total_ms", C.c_double),
                ("form", C.c_int32), ("persistent_fallbacks", C.c_int32)]


class hh_bounds_result(C.Structure):
    """hh_lsm_upper_bound's result: the dual upper bound, its standard error, the sizes and the two kernels' times."""
    _fields_ = [("upper", C.c_double), ("upper_se", C.c_double), ("n_outer", C.c_uint64),
                ("n_inner", C.c_uint32), ("reserved", C.c_uint32),
                ("nested_ms", C.c_double), ("outer_ms", C.c_double), ("total_ms", C.c_double)]


class hh_path_payoff(C.Structure):
    _fields_ = [("kind", C.c_int32), ("barrier_type", C.c_int32), ("strike", C.c_double), ("cp", C.c_double),
                ("barrier", C.c_double), ("rebate", C.c_double), ("cash", C.c_double)]


class hh_jump(C.Structure):
    """The Merton jump parameters: intensity λ, mean μ_J and standard deviation σ_J of one jump in log S."""
    _fields_ = [("lambda_", C.c_double), ("mu_j", C.c_double), ("sigma_j", C.c_double)]


class hh_vg(C.Structure):
    """The Variance Gamma parameters: drift θ of the time-changed Brownian motion and variance rate ν of the gamma clock."""
    _fields_ = [("theta", C.c_double), ("nu", C.c_double)]


class hh_qe(C.Structure):
    """The quadratic-exponential step's options: the branch threshold ψ_c (0: the default 1.5) and the martingale switch."""
    _fields_ = [("psi_c", C.c_double), ("martingale", C.c_int32), ("reserved", C.c_int32)]


class hh_assets(C.Structure):
    """Several correlated lognormal assets and the index kind: spots, volatilities, weights and the row-major
    correlation matrix with row stride HH_MAX_ASSETS."""
    _fields_ = [("n_assets", C.c_uint32), ("index_kind", C.c_int32),
                ("spots", C.c_double * HH_MAX_ASSETS), ("sigmas", C.c_double * HH_MAX_ASSETS),
                ("weights", C.c_double * HH_MAX_ASSETS), ("corr", C.c_double * (HH_MAX_ASSETS * HH_MAX_ASSETS))]


HH_LSM_MAX_BASIS = 45
HH_LSM_STATES_LOG_ASSETS = 0
HH_LSM_STATES_LOG_SPOT_VARIANCE = 1


class hh_lsm_states(C.Structure):
    """How a column's m state rows give the exercise value and the regressors of the several-variable induction (enum
    hh_lsm_states_kind): log-states of assets, the index kind and weights, cp and strike."""
    _fields_ = [("kind", C.c_int32), ("n_states", C.c_uint32), ("index_kind", C.c_int32), ("reserved", C.c_int32),
                ("cp", C.c_double), ("strike", C.c_double), ("weights", C.c_double * HH_MAX_ASSETS)]


class hh_localvol(C.Structure):
    """A local-volatility surface: σ at (times[j], x_lo + i·h), row-major [n_times][n_x], in host memory."""
    _fields_ = [("times", _dp), ("vols", _dp), ("x_lo", C.c_double), ("h", C.c_double),
                ("n_times", C.c_uint32), ("n_x", C.c_uint32)]


HH_SOURCE_EULER, HH_SOURCE_JUMP, HH_SOURCE_QE, HH_SOURCE_BATES, HH_SOURCE_LOCALVOL, HH_SOURCE_VG = range(6)


class hh_path_source(C.Structure):
    """A member of the log-spot path family (enum hh_path_source_kind) and the structs its kernel reads; the others NULL."""
    _fields_ = [("kind", C.c_int32), ("jump", C.POINTER(hh_jump)), ("qe", C.POINTER(hh_qe)),
                ("localvol", C.POINTER(hh_localvol)), ("vg", C.POINTER(hh_vg))]


HH_BK_ROOT_SECANT, HH_BK_ROOT_ORDER2 = 0, 1
HH_BK_BRACKET_MIDPOINT, HH_BK_BRACKET_ROOTS = 0, 1
HH_BK_CAPS_AS_WRITTEN, HH_BK_CAPS_ROOTS_DEFAULT = 0, 1
HH_OPT_LSM_FORM = 1
HH_OPT_BK_TERM_CACHE = 2
HH_OPT_GRID_FORM = 3
HH_OPT_LSM_SPIN_TICKS = 4
HH_OPT_FUSE_REDUCE = 5
HH_OPT_GRID_ORDER = 6
HH_OPT_FINISH_SPIN_TICKS = 7
HH_OPT_FINISH_TILE_FIRST = 8
HH_GRID_FORM_PER_DATE, HH_GRID_FORM_BATCHED = 0, 1
HH_CM_GRAD_LEN = 8  # enum hh_cm_grad: S0, V0, kappa, theta, sigma, rho, r_drift, discount
HH_LSM_FORM_PER_DATE, HH_LSM_FORM_PERSISTENT, HH_LSM_FORM_AUTO = 0, 1, 2
HH_CRR_MAX_STEPS, HH_CRR_FORM_A_MAX_STEPS = 32768, 2047
HH_CRR_EUROPEAN, HH_CRR_AMERICAN_FORWARD, HH_CRR_AMERICAN_SPOT = 0, 1, 2
HH_FD_MAX_SPACE, HH_FD_MAX_TIME, HH_FD_FORM_A_MAX_SPACE = 4096, 65536, 1024
HH_FD_EUROPEAN, HH_FD_AMERICAN = 0, 1


class HedgehogMCError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"hedgehog_mc error {code}: {msg}")
        self.code = code


LIB_PATH = os.environ.get("HEDGEHOG_MC_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "lib", "libhedgehog_mc.so")  # env: A/B builds

# every symbol include/hedgehog_mc.h declares: (name, restype, argtypes)
_vp = C.c_void_p
SYMBOLS = [
    ("hh_abi_version", C.c_int, []),
    ("hh_ctx_create", C.c_int, [C.POINTER(_vp), C.c_int]),
    ("hh_ctx_destroy", None, [_vp]),
    ("hh_ctx_set_stream", C.c_int, [_vp, _vp]),
    ("hh_ctx_reset_stream", C.c_int, [_vp]),
    ("hh_last_error", C.c_char_p, [_vp]),
    ("hh_ctx_set_option", C.c_int, [_vp, C.c_int32, C.c_int64]),
    ("hh_ctx_check_last", C.c_int, [_vp]),
    ("hh_mc_solve", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.POINTER(hh_result), _vp]),
    ("hh_mc_accumulate", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), _vp, _vp]),
    ("hh_mc_solve_multi", C.c_int, [_vp, C.POINTER(hh_model), C.c_uint32, C.POINTER(hh_config), C.POINTER(hh_result), _vp]),
    ("hh_mc_accumulate_multi", C.c_int, [_vp, C.POINTER(hh_model), C.c_uint32, C.POINTER(hh_config), _vp, _vp]),
    ("hh_mc_finalize", C.c_int, [C.POINTER(hh_model), C.POINTER(hh_config), _vp, C.POINTER(hh_result)]),
    ("hh_mc_accumulate_basket", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), _vp, _vp, C.c_uint32, _vp, _vp]),
    ("hh_mc_solve_basket", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), _vp, _vp, C.c_uint32, _vp, _vp]),
    ("hh_carr_madan", C.c_int, [_vp, C.POINTER(hh_model), C.c_int32, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    ("hh_carr_madan_basket", C.c_int, [_vp, C.POINTER(hh_model), C.c_int32, C.c_int32, C.c_double, C.c_double,
                                       _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp]),
    ("hh_carr_madan_basket_grad", C.c_int, [_vp, C.POINTER(hh_model), C.c_int32, C.c_int32, C.c_double,
                                            C.c_double, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp]),
    ("hh_crr_solve", C.c_int, [_vp, C.c_int32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp]),
    ("hh_fd_solve", C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("hh_lsm_grid_elems", C.c_size_t, [C.c_uint64, C.c_uint32, C.c_int32]),
    ("hh_lsm_solve", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_int32, C.c_double, C.POINTER(hh_lsm_result), _vp, _vp, _vp]),
    ("hh_lsm_solve_grid", C.c_int, [_vp, C.POINTER(hh_model), _vp, C.c_uint64, C.c_uint32, C.c_int32, C.c_double, C.POINTER(hh_lsm_result), _vp, _vp]),
    ("hh_heston_exact_grid", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), _vp, _vp, C.c_int32, C.POINTER(hh_result)]),
    ("hh_euler_grid", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_int32, _vp, _vp, C.c_int32, C.POINTER(hh_result)]),
    ("hh_lsm_solve_euler", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_int32, C.c_int32, C.c_double,
                                     C.POINTER(hh_lsm_result), _vp, _vp, _vp]),
    ("hh_mc_path_grid", C.c_int, [_vp, C.POINTER(hh_path_source), C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32, _vp,
                                  C.c_int32, C.POINTER(hh_result)]),
    ("hh_lsm_solve_path", C.c_int, [_vp, C.POINTER(hh_path_source), C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32,
                                    C.c_int32, C.c_double, C.POINTER(hh_lsm_result), _vp, _vp, _vp]),
    ("hh_mc_path_stats", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32, C.c_int32, _vp, C.c_int32,
                                   C.POINTER(hh_result)]),
    ("hh_mc_solve_path", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32, C.c_int32,
                                   C.POINTER(hh_path_payoff), C.c_uint32, C.POINTER(hh_result), _vp, _vp]),
    ("hh_mc_path_stats_ex", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32, C.c_int32, C.c_int32, _vp,
                                      C.c_int32, C.POINTER(hh_result)]),
    ("hh_mc_solve_path_ex", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32, C.c_int32, C.c_int32,
                                      C.POINTER(hh_path_payoff), C.c_uint32, C.POINTER(hh_result), _vp, _vp]),
    ("hh_path_tangent_rows", C.c_size_t, [C.c_uint32]),
    ("hh_mc_path_stats_tangent", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32, C.c_int32, _vp,
                                           C.c_int32, _vp, C.POINTER(hh_result)]),
    ("hh_mc_solve_path_tangent", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32, C.c_int32,
                                           C.POINTER(hh_path_payoff), C.c_uint32, C.POINTER(hh_result), _vp]),
    ("hh_mc_path_stats_coupled", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32, C.c_int32, _vp,
                                           C.c_int32, C.POINTER(hh_result)]),
    ("hh_mc_solve_path_coupled", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32, C.c_int32,
                                           C.POINTER(hh_path_payoff), C.c_uint32, C.POINTER(hh_result), C.POINTER(hh_result),
                                           _vp, _vp]),
    ("hh_mc_solve_jump", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_jump), C.POINTER(hh_config), C.POINTER(hh_result),
                                   _vp]),
    ("hh_mc_solve_path_jump", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_jump), C.POINTER(hh_config), C.c_uint32,
                                        C.c_int32, C.POINTER(hh_path_payoff), C.c_uint32, C.POINTER(hh_result), _vp, _vp]),
    ("hh_carr_madan_jump", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_jump), C.c_double, C.c_double,
                                     _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp]),
    ("hh_mc_solve_vg", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_vg), C.POINTER(hh_config), C.POINTER(hh_result), _vp]),
    ("hh_mc_path_stats_vg", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_vg), C.POINTER(hh_config), C.c_uint32, C.c_int32,
                                      _vp, C.c_int32, C.POINTER(hh_result)]),
    ("hh_mc_solve_path_vg", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_vg), C.POINTER(hh_config), C.c_uint32,
                                      C.c_int32, C.POINTER(hh_path_payoff), C.c_uint32, C.POINTER(hh_result), _vp, _vp]),
    ("hh_carr_madan_vg", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_vg), C.c_double, C.c_double,
                                   _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp]),
    ("hh_mc_path_stats_qe", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_qe), C.POINTER(hh_config), C.c_uint32,
                                      C.c_int32, _vp, C.c_int32, _vp, C.POINTER(hh_result)]),
    ("hh_mc_solve_path_qe", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_qe), C.POINTER(hh_config), C.c_uint32,
                                      C.c_int32, C.POINTER(hh_path_payoff), C.c_uint32, C.POINTER(hh_result), _vp, _vp, _vp]),
    ("hh_mc_path_stats_bates", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_qe), C.POINTER(hh_jump), C.POINTER(hh_config),
                                         C.c_uint32, C.c_int32, _vp, C.c_int32, _vp, C.POINTER(hh_result)]),
    ("hh_mc_solve_path_bates", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_qe), C.POINTER(hh_jump), C.POINTER(hh_config),
                                         C.c_uint32, C.c_int32, C.POINTER(hh_path_payoff), C.c_uint32, C.POINTER(hh_result),
                                         _vp, _vp, _vp]),
    ("hh_carr_madan_bates", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_jump), C.c_double, C.c_double,
                                      _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp]),
    ("hh_mc_path_stats_assets", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_assets), C.POINTER(hh_config), C.c_uint32,
                                          C.c_int32, _vp, C.c_int32, C.POINTER(hh_result)]),
    ("hh_mc_solve_path_assets", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_assets), C.POINTER(hh_config), C.c_uint32,
                                          C.c_int32, C.POINTER(hh_path_payoff), C.c_uint32, C.POINTER(hh_result), _vp, _vp]),
    ("hh_assets_rows_elems", C.c_size_t, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int32]),
    ("hh_assets_path_rows", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_assets), C.POINTER(hh_config), C.c_uint32, _vp,
                                      C.c_int32, C.POINTER(hh_result)]),
    ("hh_lsm_solve_states", C.c_int, [_vp, C.POINTER(hh_lsm_states), _vp, C.c_uint64, C.c_uint32, C.c_int32, C.c_double,
                                      C.POINTER(hh_lsm_result), _vp, _vp, _vp]),
    ("hh_lsm_solve_assets", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_assets), C.POINTER(hh_config), C.c_uint32,
                                      C.c_int32, C.c_double, C.POINTER(hh_lsm_result), _vp, _vp, _vp]),
    ("hh_mc_path_states", C.c_int, [_vp, C.POINTER(hh_path_source), C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32, _vp,
                                    C.c_int32, C.POINTER(hh_result)]),
    ("hh_lsm_solve_path_states", C.c_int, [_vp, C.POINTER(hh_path_source), C.POINTER(hh_model), C.POINTER(hh_config),
                                           C.c_uint32, C.c_int32, C.c_double, C.POINTER(hh_lsm_result), _vp, _vp, _vp, _vp]),
    ("hh_lsm_policy_elems", C.c_size_t, [C.c_uint32, C.c_uint32, C.c_int32]),
    ("hh_lsm_fit_states", C.c_int, [_vp, C.POINTER(hh_lsm_states), _vp, C.c_uint64, C.c_uint32, C.c_int32, C.c_double,
                                    C.POINTER(hh_lsm_result), _vp, _vp, _vp]),
    ("hh_lsm_fit_path_states", C.c_int, [_vp, C.POINTER(hh_path_source), C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32,
                                         C.c_int32, C.c_double, C.POINTER(hh_lsm_result), _vp]),
    ("hh_lsm_policy_value", C.c_int, [_vp, C.POINTER(hh_lsm_states), _vp, C.c_int32, _vp, C.c_uint64, C.c_uint32, C.c_double,
                                      C.POINTER(hh_lsm_result), _vp, _vp]),
    ("hh_lsm_policy_value_path", C.c_int, [_vp, C.POINTER(hh_path_source), C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32,
                                           _vp, C.c_int32, C.c_double, C.POINTER(hh_lsm_result)]),
    ("hh_lsm_upper_bound", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_uint32, _vp, C.c_int32, C.c_double,
                                     C.c_uint32, C.c_uint64, C.POINTER(hh_bounds_result), _vp, _vp, _vp]),
    ("hh_mc_path_stats_lv", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_localvol), C.POINTER(hh_config), C.c_uint32,
                                      C.c_int32, C.c_int32, _vp, C.c_int32, C.POINTER(hh_result)]),
    ("hh_mc_solve_path_lv", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_localvol), C.POINTER(hh_config), C.c_uint32,
                                      C.c_int32, C.c_int32, C.POINTER(hh_path_payoff), C.c_uint32, C.POINTER(hh_result),
                                      _vp, _vp]),
    ("hh_lsm_shard_xchg_elems", C.c_size_t, [C.c_uint32, C.c_int32]),
    ("hh_lsm_shard_begin", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_int32, C.c_double, _vp]),
    ("hh_lsm_shard_phase", C.c_int, [_vp, C.c_int32, C.c_uint32, _vp, _vp]),
    ("hh_lsm_shard_finish", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("hh_lsm_finalize", C.c_int, [_vp, C.POINTER(hh_lsm_result)]),
    ("hh_lsm_debug_read", C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_int32, _vp]),
    ("hh_replay_elems", C.c_size_t, [C.c_uint64, C.c_uint32, C.c_int32]),
    ("hh_replay_pack", C.c_int, [_vp, C.c_int32, C.c_uint64, C.c_uint32, _vp, C.c_int32, _vp]),
    ("hh_wiener_fill", C.c_int, [_vp, C.c_int32, C.c_double, C.c_double, C.c_uint32, C.c_uint64, _vp, C.c_int32, _vp]),
    ("hh_sobol_directions", C.c_int, [C.c_uint32, _vp]),
    ("hh_sobol_points", C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, _vp]),
    ("hh_sobol_fill", C.c_int, [_vp, C.c_int32, C.c_double, C.c_double, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                                C.c_uint32, C.c_int32, C.c_int32, _vp]),
    ("hh_seeds_fingerprint", C.c_uint64, [_vp, C.c_uint64]),
    ("hh_seeds_cache", C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, C.POINTER(_vp)]),
    ("hh_seeds_cache_stats", C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("hh_device_malloc", C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    ("hh_device_free", C.c_int, [_vp, _vp]),
    ("hh_memcpy_h2d", C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    ("hh_memcpy_d2h", C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    ("hh_ctx_synchronize", C.c_int, [_vp]),
    ("hh_ctx_enable_timing", C.c_int, [_vp, C.c_int32]),
    ("hh_ctx_read_timings", C.c_int, [_vp, _vp, C.c_int32, C.POINTER(C.c_int32)]),
    ("hh_bk_decisions", C.c_int, [_vp, C.c_uint64, _vp, _vp]),
    ("hh_mgpu_create", C.c_int, [C.POINTER(_vp), C.POINTER(C.c_int), C.c_int, C.c_int]),
    ("hh_mgpu_destroy", None, [_vp]),
    ("hh_mgpu_last_error", C.c_char_p, [_vp]),
    ("hh_mgpu_n_devices", C.c_int, [_vp]),
    ("hh_mgpu_reduce_mode", C.c_int, [_vp]),
    ("hh_mgpu_ctx", _vp, [_vp, C.c_int]),
    ("hh_mgpu_selftest", C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("hh_mgpu_rccl_info", C.c_int, [_vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("hh_mgpu_set_option", C.c_int, [_vp, C.c_int32, C.c_int64]),
    ("hh_mgpu_enqueue_stats", C.c_int, [_vp, _vp, C.POINTER(C.c_double)]),
    ("hh_mgpu_shard_range", None, [C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("hh_mgpu_solve", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.POINTER(hh_result), _vp]),
    ("hh_mgpu_solve_shards", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.POINTER(hh_result), _vp]),
    ("hh_mgpu_solve_basket", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), _vp, _vp, C.c_uint32, _vp]),
    ("hh_mgpu_solve_multi", C.c_int, [_vp, C.POINTER(hh_model), C.c_uint32, C.POINTER(hh_config), C.POINTER(hh_result)]),
    ("hh_mgpu_lsm_solve", C.c_int, [_vp, C.POINTER(hh_model), C.POINTER(hh_config), C.c_int32, C.c_double,
                                    C.POINTER(hh_lsm_result), _vp, _vp]),
]

_lib = None


def load_library(path: str | None = None):
    """Load the C-ABI library (once). Raises HedgehogMCError when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise HedgehogMCError(HH_ERR_HIP, f"{path} not found — build it with "
                              "`python -c 'import __graft_entry__ as g; g.build()'`; "
                              "there is no CPU fallback")
    if not os.environ.get("HEDGEHOG_MC_NO_TORCH"):
        try:  # share PyTorch's HIP runtime (same libamdhip64 soname) when torch is the allocator
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the C-ABI itself
            pass
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class Context:
    """Owns one hh_ctx (one device, one stream)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = load_library()
        h = _vp()
        rc = self.lib.hh_ctx_create(C.byref(h), int(device))
        if rc != HH_OK:
            raise HedgehogMCError(rc, f"hh_ctx_create(device={device}) failed — no HIP device? "
                                  "(the product path has no CPU fallback)")
        self.handle = h
        self.device = int(device)
        if stream is not None:
            self.set_stream(stream)

    def check(self, rc: int):
        if rc != HH_OK:
            raise HedgehogMCError(rc, self.lib.hh_last_error(self.handle).decode(errors="replace"))

    def set_stream(self, stream: int | None):
        """Launch on an external hipStream_t handle (0 = the default stream); None = own stream."""
        if stream is None:
            self.check(self.lib.hh_ctx_reset_stream(self.handle))
        else:
            self.check(self.lib.hh_ctx_set_stream(self.handle, _vp(stream)))

    def set_option(self, option: int, value: int):
        self.check(self.lib.hh_ctx_set_option(self.handle, int(option), int(value)))

    def synchronize(self):
        self.check(self.lib.hh_ctx_synchronize(self.handle))

    def check_last(self):
        """After asynchronous solves (accumulate): waits for the stream; raises HH_ERR_DEVICE_TIMEOUT when a record
        reduction inside a simulation kernel gave up since the last check (the context has been reset by then)."""
        self.check(self.lib.hh_ctx_check_last(self.handle))

    def seeds_on_device(self, seeds, fingerprint: int = 0) -> int:
        """Device address of this seed vector in the context's content-addressed cache (hh_seeds_cache): valid
        until a later call misses — ask right before every solve."""
        p = _vp()
        self.check(self.lib.hh_seeds_cache(self.handle, _vp(seeds.ctypes.data), seeds.size, int(fingerprint), C.byref(p)))
        return p.value

    def seeds_cache_stats(self):
        h, u, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self.check(self.lib.hh_seeds_cache_stats(self.handle, C.byref(h), C.byref(u), C.byref(e)))
        return {"hits": h.value, "uploads": u.value, "evictions": e.value}

    def enable_timing(self, on: bool = True):
        self.check(self.lib.hh_ctx_enable_timing(self.handle, int(on)))

    def read_timings(self):
        """ms of each simulation-kernel launch since the last read (syncs the stream)."""
        buf = (C.c_double * 256)()
        n = C.c_int32(0)
        self.check(self.lib.hh_ctx_read_timings(self.handle, buf, 256, C.byref(n)))
        return [buf[i] for i in range(n.value)]

    # a few recycled device buffers by exact size (the sample buffers of repeated solves)
    _POOL_MAX = 4

    def pool_take(self, nbytes: int):
        pool = self.__dict__.setdefault("_pool", [])
        for i, (p, n) in enumerate(pool):
            if n == nbytes:
                del pool[i]
                return p
        return None

    def pool_put(self, ptr: int, nbytes: int) -> bool:
        pool = self.__dict__.setdefault("_pool", [])
        if len(pool) >= self._POOL_MAX:
            old_p, _ = pool.pop(0)
            self.lib.hh_device_free(self.handle, _vp(old_p))
        pool.append((ptr, nbytes))
        return True

    def close(self):
        if getattr(self, "handle", None):
            for p, _ in self.__dict__.get("_pool", []):
                self.lib.hh_device_free(self.handle, _vp(p))
            self.__dict__["_pool"] = []
            self.lib.hh_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """Device memory of a Context (hh_device_malloc / hh_device_free), released with the object."""

    def __init__(self, ctx: Context, nbytes: int, pooled: bool = False):
        self.ctx, self.nbytes, self._pooled = ctx, int(nbytes), pooled
        self.ptr = ctx.pool_take(self.nbytes) if pooled else None
        if self.ptr is None:
            p = _vp()
            ctx.check(ctx.lib.hh_device_malloc(ctx.handle, max(self.nbytes, 8), C.byref(p)))
            self.ptr = p.value

    def upload(self, arr):
        assert arr.flags.c_contiguous and arr.nbytes <= self.nbytes
        self.ctx.check(self.ctx.lib.hh_memcpy_h2d(self.ctx.handle, _vp(self.ptr), _vp(arr.ctypes.data), arr.nbytes))
        return self

    def download(self, arr):
        assert arr.flags.c_contiguous and arr.nbytes <= self.nbytes
        self.ctx.check(self.ctx.lib.hh_memcpy_d2h(self.ctx.handle, _vp(arr.ctypes.data), _vp(self.ptr), arr.nbytes))
        return arr

    def free(self):
        if getattr(self, "ptr", None) and getattr(self.ctx, "handle", None):
            self.ctx.lib.hh_device_free(self.ctx.handle, _vp(self.ptr))
        self.ptr = None

    def recycle(self):
        """Hand the memory back to the context's pool (hipMalloc / hipFree cost 0.1-0.3 ms each and
        synchronise: a solve that allocates its sample buffer afresh pays more than the download)."""
        if getattr(self, "ptr", None) and getattr(self.ctx, "handle", None) and self.ctx.pool_put(self.ptr, self.nbytes):
            self.ptr = None
        else:
            self.free()

    def __del__(self):  # pragma: no cover
        try:
            self.recycle() if getattr(self, "_pooled", False) else self.free()
        except Exception:
            pass


class BorrowedContext(Context):
    """The hh_ctx of one device of a MultiGpu (hh_mgpu_ctx): same methods, never destroyed here."""

    def __init__(self, lib, handle, device):
        self.lib, self.handle, self.device = lib, handle, int(device)

    def close(self):
        for p, _ in self.__dict__.get("_pool", []):
            self.lib.hh_device_free(self.handle, _vp(p))
        self.__dict__["_pool"] = []
        self.handle = None


class MultiGpu:
    """Owns one hh_mgpu: one hh_ctx per listed device, driven from this host thread; the accumulator
    vectors are combined inside the library (RCCL all-reduce, or the host's ordered sum)."""

    def __init__(self, devices, flags: int = HH_MGPU_AUTO):
        self.lib = load_library()
        self.devices = [int(d) for d in devices]
        arr = (C.c_int * len(self.devices))(*self.devices)
        h = _vp()
        rc = self.lib.hh_mgpu_create(C.byref(h), arr, len(self.devices), int(flags))
        if rc != HH_OK:
            raise HedgehogMCError(rc, f"hh_mgpu_create(devices={self.devices}, flags={flags}) failed "
                                  "(no HIP device, a bad ordinal, or RCCL required but unavailable)")
        self.handle = h
        self._ctxs = [BorrowedContext(self.lib, _vp(self.lib.hh_mgpu_ctx(h, i)), d)
                      for i, d in enumerate(self.devices)]

    @property
    def n_devices(self) -> int:
        return self.lib.hh_mgpu_n_devices(self.handle)

    @property
    def reduce_mode(self) -> int:
        return self.lib.hh_mgpu_reduce_mode(self.handle)

    def last_error(self) -> str:
        return self.lib.hh_mgpu_last_error(self.handle).decode(errors="replace")

    def selftest(self):
        """(ranks counted by an all-reduce of ones through the solve's own exchange, reduce mode it ran in)"""
        n, mode = C.c_int32(0), C.c_int32(0)
        self.check(self.lib.hh_mgpu_selftest(self.handle, C.byref(n), C.byref(mode)))
        return n.value, mode.value

    def rccl_info(self):
        """{"library": path the collective entry points were bound from ("" = none), "version", "from_env", "usable"}"""
        buf = C.create_string_buffer(512)
        ver, env = C.c_int32(0), C.c_int32(0)
        rc = self.lib.hh_mgpu_rccl_info(self.handle, buf, 512, C.byref(ver), C.byref(env))
        return {"library": buf.value.decode(errors="replace"), "version": ver.value, "from_env": bool(env.value),
                "usable": rc == HH_OK}

    def set_option(self, option: int, value: int):
        self.check(self.lib.hh_mgpu_set_option(self.handle, int(option), int(value)))

    def enqueue_stats(self):
        """(per-shard host µs, whole-phase host µs) of the last solve's enqueue phase."""
        per = (C.c_double * len(self.devices))()
        whole = C.c_double(0.0)
        self.check(self.lib.hh_mgpu_enqueue_stats(self.handle, per, C.byref(whole)))
        return list(per), whole.value

    def ctx(self, i: int) -> Context:
        return self._ctxs[i]

    def check(self, rc: int):
        if rc != HH_OK:
            raise HedgehogMCError(rc, self.last_error())

    def shard_range(self, n_paths: int, g: int, tile_aligned: bool = False):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.lib.hh_mgpu_shard_range(int(n_paths), len(self.devices), int(g), int(tile_aligned),
                                     C.byref(a), C.byref(b))
        return a.value, b.value

    def solve(self, model, cfg, terminal=None) -> hh_result:
        res = hh_result()
        self.check(self.lib.hh_mgpu_solve(self.handle, C.byref(model), C.byref(cfg), C.byref(res),
                                          terminal.ctypes.data if terminal is not None else None))
        return res

    def solve_multi(self, models, cfg):
        arr = (hh_model * len(models))(*models)
        res = (hh_result * len(models))()
        self.check(self.lib.hh_mgpu_solve_multi(self.handle, arr, len(models), C.byref(cfg), res))
        return list(res)

    def solve_shards(self, model, cfgs, terminals=None) -> hh_result:
        arr = (hh_config * len(cfgs))(*cfgs)
        tp = None
        if terminals is not None:
            tp = (_vp * len(cfgs))(*[(t if isinstance(t, int) or t is None else t.ctypes.data) for t in terminals])
        res = hh_result()
        self.check(self.lib.hh_mgpu_solve_shards(self.handle, C.byref(model), arr, C.byref(res), tp))
        return res

    def close(self):
        if getattr(self, "handle", None):
            for c in self._ctxs:
                c.close()
            self.lib.hh_mgpu_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


_contexts: dict[int, Context] = {}
_mgpus: dict[tuple, MultiGpu] = {}


def get_multi_gpu(devices, flags: int = HH_MGPU_AUTO) -> MultiGpu:
    key = (tuple(int(d) for d in devices), int(flags))
    mg = _mgpus.get(key)
    if mg is None:
        mg = _mgpus[key] = MultiGpu(key[0], flags)
    return mg


def get_context(device: int = 0) -> Context:
    ctx = _contexts.get(device)
    if ctx is None:
        ctx = _contexts[device] = Context(device)
    return ctx


def seed_array(values, n: int):
    """P-long seed vector -> ctypes double array (or NULL when all zero)."""
    if values is None or not any(values):
        return None
    arr = (C.c_double * n)(*[float(v) for v in values])
    return arr


# ---- plain-number builders of the C structs (bench, tools, tests drive the C-ABI directly) ----------

def make_model(S0=100.0, V0=0.04, kappa=2.0, theta=0.04, sigma=0.3, rho=-0.7, r=0.03, T=1.0,
               strike=100.0, cp=1.0, discount=None, seeds=None, n_partials=0):
    """hh_model from plain numbers; defaults = benchmark problem H252.
    seeds: dict name -> list of n_partials dual seeds (names: S0, V0, kappa, theta, sigma, r_drift,
    discount, strike)."""
    import math
    m = hh_model()
    m.S0, m.V0, m.kappa, m.theta, m.sigma, m.rho = S0, V0, kappa, theta, sigma, rho
    m.r_drift, m.T, m.strike, m.cp = r, T, strike, cp
    m.discount = math.exp(-r * T) if discount is None else discount
    keep = []
    for name, vals in (seeds or {}).items():
        arr = (C.c_double * n_partials)(*vals)
        keep.append(arr)
        setattr(m, "d" + name, C.cast(arr, C.POINTER(C.c_double)))
    m._keep = keep
    return m


def make_jump(lam=0.0, mu_j=0.0, sigma_j=0.0):
    """hh_jump from plain numbers (`lambda` is a Python keyword: the field is `lambda_`)."""
    j = hh_jump()
    j.lambda_, j.mu_j, j.sigma_j = lam, mu_j, sigma_j
    return j


def make_vg(theta=0.0, nu=1.0):
    """hh_vg from plain numbers"""
    g = hh_vg()
    g.theta, g.nu = theta, nu
    return g


def make_path_source(kind, jump=None, qe=None, localvol=None, vg=None):
    """hh_path_source of `kind` over the structs given (each kept alive by the descriptor)"""
    src = hh_path_source()
    src.kind = kind
    src._keep = (jump, qe, localvol, vg)
    for name, v in zip(("jump", "qe", "localvol", "vg"), src._keep):
        if v is not None:
            setattr(src, name, C.pointer(v))
    return src


def make_assets(spots, sigmas, weights, corr, index_kind=HH_INDEX_WEIGHTED_SUM):
    """hh_assets from plain numbers; corr is the d × d correlation matrix (nested sequences or an array)"""
    a = hh_assets()
    d = len(spots)
    if not 1 <= d <= HH_MAX_ASSETS or len(sigmas) != d or len(weights) != d or len(corr) != d:
        raise ValueError(f"1 .. {HH_MAX_ASSETS} assets, with as many sigmas, weights and correlation rows")
    a.n_assets, a.index_kind = d, int(index_kind)
    for i in range(d):
        a.spots[i], a.sigmas[i], a.weights[i] = float(spots[i]), float(sigmas[i]), float(weights[i])
        if len(corr[i]) != d:
            raise ValueError("the correlation matrix must be square")
        for j in range(d):
            a.corr[i * HH_MAX_ASSETS + j] = float(corr[i][j])
    return a


def make_localvol(times, vols, x_lo, h):
    """hh_localvol from arrays (kept alive on the returned struct): times [n_times], vols [n_times][n_x]"""
    import numpy as np
    times = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
    vols = np.ascontiguousarray(vols, dtype=np.float64)
    if vols.ndim != 2 or vols.shape[0] != times.size:
        raise ValueError("vols must be [n_times][n_x]")
    lv = hh_localvol()
    lv.times = times.ctypes.data_as(_dp)
    lv.vols = vols.ctypes.data_as(_dp)
    lv.x_lo, lv.h, lv.n_times, lv.n_x = float(x_lo), float(h), times.size, vols.shape[1]
    lv._keep = [times, vols]
    return lv


def make_qe(psi_c=0.0, martingale=False):
    """hh_qe from plain numbers (psi_c = 0: the library's default 1.5)"""
    q = hh_qe()
    q.psi_c, q.martingale, q.reserved = psi_c, int(bool(martingale)), 0
    return q


def make_config(dynamics, strategy, n_paths, n_steps=1, antithetic=0, em_split=1, noise_mode=0,
                seeds=None, replay=None, replay_layout=0, n_partials=0, path_offset=0,
                compat_sqrt_alpha=0):
    """hh_config from plain numbers; `seeds` / `replay` are HOST numpy arrays (kept alive on the
    returned struct) — set the pointer fields and the *_on_device flags yourself for device memory."""
    import numpy as np
    c = hh_config()
    c.dynamics, c.strategy, c.antithetic, c.em_split = dynamics, strategy, antithetic, em_split
    c.compat_sqrt_alpha = compat_sqrt_alpha
    c.noise_mode, c.replay_layout = noise_mode, replay_layout
    c.n_steps, c.n_partials, c.n_paths, c.path_offset = n_steps, n_partials, n_paths, path_offset
    keep = []
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        keep.append(seeds)
        c.seeds = seeds.ctypes.data
        c.seeds_len = seeds.size
    if replay is not None:
        replay = np.ascontiguousarray(replay, dtype=np.float64)
        keep.append(replay)
        c.replay = replay.ctypes.data
        c.replay_len = replay.size
    c._keep = keep
    return c
