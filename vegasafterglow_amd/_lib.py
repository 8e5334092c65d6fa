"""ctypes binding of the C-ABI in include/vegasafterglow_amd.h.

The shared library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  There is no
fallback of any kind: a missing library or a machine without a HIP device raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VAG_LIB_PATH") or os.path.join(_HERE, "libvegasafterglow_amd.so")  # override: kernel experiments

JET_TOPHAT, JET_GAUSSIAN, JET_POWERLAW, JET_TWO_COMPONENT, JET_MAGNETIZED_TOPHAT = 0, 1, 2, 3, 4
JET_STEP_POWERLAW, JET_POWERLAW_WING = 5, 6
MEDIUM_ISM, MEDIUM_WIND = 0, 1

VAG_OK, VAG_E_INVALID, VAG_E_NO_DEVICE, VAG_E_HIP, VAG_E_UNSUPPORTED, VAG_E_CAPACITY, VAG_E_NUMERIC, VAG_E_INTERNAL = 0, -1, -2, -3, -4, -5, -6, -7
FLAG_SSC, FLAG_KN, FLAG_RVS, FLAG_RVS_SSC, FLAG_RVS_KN, FLAG_SPREADING, FLAG_MAGNETAR = 1, 2, 4, 8, 16, 32, 64  # VAG_FLAG_* of include/vegasafterglow_amd.h
FLAG_NON_AXISYMMETRIC = 128

# VAG_P_* slots of the fit transformer (include/vegasafterglow_amd.h)
PARAM_SLOTS = {
    "theta_c": 0, "E_iso": 1, "Gamma0": 2, "k_e": 3, "k_g": 4, "theta_w": 5, "E_iso_w": 6, "Gamma0_w": 7,
    "tau": 8, "duration": 8, "n_ism": 9, "A_star": 10, "n0": 11, "lumi_dist": 12, "z": 13, "theta_v": 14,
    "theta_obs": 14, "eps_e": 15, "eps_B": 16, "p": 17, "xi_e": 18,
    "eps_e_r": 24, "eps_B_r": 25, "p_r": 26, "xi_e_r": 27,  # VAG_P_RVS_*: rvs_rad of Fitter(rvs_shock=True)
    "sigma0": 28, "k_m": 29, "L0": 30, "t0": 31, "q": 32,
}


class ModelParams(C.Structure):
    _fields_ = [
        ("jet_type", C.c_int32), ("medium_type", C.c_int32),
        ("theta_c", C.c_double), ("E_iso", C.c_double), ("Gamma0", C.c_double),
        ("k_e", C.c_double), ("k_g", C.c_double), ("theta_w", C.c_double),
        ("E_iso_w", C.c_double), ("Gamma0_w", C.c_double), ("duration", C.c_double),
        ("n_ism", C.c_double), ("A_star", C.c_double), ("n0", C.c_double),
        ("lumi_dist", C.c_double), ("z", C.c_double), ("theta_obs", C.c_double),
        ("eps_e", C.c_double), ("eps_B", C.c_double), ("p", C.c_double), ("xi_e", C.c_double),
        ("phi_resol", C.c_double), ("theta_resol", C.c_double), ("t_resol", C.c_double), ("rtol", C.c_double),
        ("radiative_fireball", C.c_int32), ("flags", C.c_int32),
        ("rvs_eps_e", C.c_double), ("rvs_eps_B", C.c_double), ("rvs_p", C.c_double), ("rvs_xi_e", C.c_double),
        ("sigma0", C.c_double), ("k_m", C.c_double),
        ("mag_L0", C.c_double), ("mag_t0", C.c_double), ("mag_q", C.c_double),
    ]


class BandObs(C.Structure):
    _fields_ = [("nu_min", C.c_double), ("nu_max", C.c_double), ("num_points", C.c_int32), ("n", C.c_int32),
                ("t", C.POINTER(C.c_double)), ("ln_flux", C.POINTER(C.c_double)), ("ln_err", C.POINTER(C.c_double)),
                ("weight", C.POINTER(C.c_double))]


# VAG_MATH_*: the device routines vag_debug_device_math evaluates (include/vegasafterglow_amd.h)
MATH = {name: i for i, name in enumerate([
    "exp2_fast", "exp2_ode", "exp2_sat", "exp2_or_zero", "log2_fast", "log2_tab", "log2_tab_nb",
    "rcp_fast", "rcp_ode", "rcp1", "sqrt_fast", "sqrt_ode", "sqrt1", "sp_fast", "sp_fast_global", "sp_fast_sel",
    "syn_cell", "ic_cell", "wave_prefix_sum", "wave_sum", "sky_wave_sum", "lds_add", "log_ndtr"])}
# VAG_MATH_* appended after VAG_MATH_LOG_NDTR.  They have a mapping of their own: MATH is pinned to end with log_ndtr
# (tests/test_limits_host.py), and the ids of both mappings are the enum's, one numbering.
MATH_MORE = {name: len(MATH) + i for i, name in enumerate([
    "poisson_deviance", "log_slope", "elec_cell", "fwd_state",
    "rel_gamma", "shock_jump", "sound_speed", "rvs_state", "cross_lattice", "rvs_extrap", "pair_init",
    "kn_lut", "kn_corr", "ic_table", "ic_bin_integral", "ic_suffix_scan", "ic_column_den",
    "ic_y", "ic_step", "ic_fixed_point", "ic_gamma_a",
    "exp2_fast_chain", "sp_fast_relu", "sp_fast_relu_vmagic"])}
# [n_in, n_out] per point of the routines of MATH_MORE that tests/_rsref.py restates (vag_debug_math.h)
MATH_RS_SHAPES = {"rel_gamma": (2, 2), "shock_jump": (2, 3), "sound_speed": (1, 2), "rvs_state": (14, 6), "cross_lattice": (7, 4),
                  "rvs_extrap": (65, 48), "pair_init": (10, 11)}
# the same for the inverse-Compton routines that tests/_icref.py restates
MATH_IC_SHAPES = {"kn_lut": (1, 2), "kn_corr": (2, 4), "ic_table": (21, 2), "ic_bin_integral": (9, 1), "ic_suffix_scan": (4, 4),
                  "ic_column_den": (9, 1), "ic_y": (10, 18), "ic_step": (8, 5), "ic_fixed_point": (9, 6), "ic_gamma_a": (11, 4)}

P_A_V = 1000  # VAG_P_A_V
# VAG_P_SKY_*: the sky placement of the centroid and visibility groups (vag_loglike_sky_batch / _vis_batch), not Model fields either
SKY_SLOTS = {"pa": 1001, "east0": 1002, "north0": 1003}
# VAG_P_POL_*: the field behind the shocks as the polarization groups see it (vag_loglike_pol_batch), not Model fields either
POL_SLOTS = {"pol_b": 1004, "pol_pi_max": 1005, "pol_b_rvs": 1006, "pol_pi_max_rvs": 1007}
# VAG_P_NOISE_SYS0 + g: the fractional systematic of noise group g (vag_loglike_noise_batch), the parameter "sys_<label>" of a Fitter
P_NOISE_SYS0, NOISE_MAX_GROUPS = 1008, 8
NOISE_PREFIX = "sys_"
# VAG_P_N_H: the absorbing column of the count-spectrum groups (vag_loglike_fold_batch), the parameter "N_H" of a Fitter
P_N_H = 1016
# VAG_P_TMPL_AMP0 + c: the amplitude of additive template c (vag_loglike_tmpl_batch), the parameter "amp_<name>" of a Fitter
P_TMPL_AMP0, TMPL_MAX = 1017, 8
TMPL_PREFIX = "amp_"
# VAG_P_ROBUST_FRAC0 / _SCALE0 / _SHIFT0 + g: the outlier fraction, extra scatter and mean offset of robust noise group g
# (vag_loglike_robust_batch), the parameters "out_frac_<label>", "out_scale_<label>", "out_shift_<label>" of a Fitter
P_ROBUST_FRAC0, P_ROBUST_SCALE0, P_ROBUST_SHIFT0 = 1025, 1033, 1041
ROBUST_PREFIXES = {"out_frac_": P_ROBUST_FRAC0, "out_scale_": P_ROBUST_SCALE0, "out_shift_": P_ROBUST_SHIFT0}


class CentroidObs(C.Structure):  # vag_centroid_obs
    _fields_ = [("nu", C.c_double), ("n", C.c_int32), ("pad", C.c_int32)] + \
               [(n, C.POINTER(C.c_double)) for n in ("t", "east", "north", "err_east", "err_north", "weight")]


class SkyFitSpec(C.Structure):  # vag_sky_fit_spec
    _fields_ = [("n_groups", C.c_int32), ("pad", C.c_int32), ("groups", C.POINTER(CentroidObs)),
                ("pa_fixed", C.c_double), ("east0_fixed", C.c_double), ("north0_fixed", C.c_double)]


VIS_COMPLEX, VIS_AMPLITUDE = 0, 1  # VAG_VIS_*
VIS_KINDS = {"complex": VIS_COMPLEX, "amplitude": VIS_AMPLITUDE}


class VisibilityObs(C.Structure):  # vag_visibility_obs
    _fields_ = [("nu", C.c_double), ("n_epochs", C.c_int32), ("n_vis", C.c_int32), ("n_az", C.c_int32), ("kind", C.c_int32),
                ("t", C.POINTER(C.c_double)), ("first", C.POINTER(C.c_int32))] + \
               [(n, C.POINTER(C.c_double)) for n in ("u", "v", "re", "im", "err", "weight")]


class PolSpec(C.Structure):  # vag_pol_spec: index 0 forward, 1 reverse shock; pi_max < 0: the default from p
    _fields_ = [("b", C.c_double * 2), ("pi_max", C.c_double * 2)]


class VisFitSpec(C.Structure):  # vag_vis_fit_spec
    _fields_ = [("n_groups", C.c_int32), ("pad", C.c_int32), ("groups", C.POINTER(VisibilityObs))]


POL_QU, POL_DEGREE = 0, 1  # VAG_POL_*
POL_KINDS = {"qu": POL_QU, "degree": POL_DEGREE}


class PolarizationObs(C.Structure):  # vag_polarization_obs
    _fields_ = [("nu", C.c_double), ("n", C.c_int32), ("n_az", C.c_int32), ("kind", C.c_int32), ("pad", C.c_int32)] + \
               [(n, C.POINTER(C.c_double)) for n in ("t", "q", "u", "err_q", "err_u", "weight")]


class PolFitSpec(C.Structure):  # vag_pol_fit_spec
    _fields_ = [("n_groups", C.c_int32), ("pad", C.c_int32), ("groups", C.POINTER(PolarizationObs)),
                ("b_fixed", C.c_double * 2), ("pi_max_fixed", C.c_double * 2)]


OBS_DETECTION, OBS_UPPER_LIMIT = 0, 1  # VAG_OBS_*


class LimitRows(C.Structure):  # vag_limit_rows
    _fields_ = [("kind", C.POINTER(C.c_int32)), ("limit", C.POINTER(C.c_double)), ("sigma", C.POINTER(C.c_double))]


class LimitFitSpec(C.Structure):  # vag_limit_fit_spec
    _fields_ = [("point", LimitRows), ("n_bands", C.c_int32), ("pad", C.c_int32), ("bands", C.POINTER(LimitRows)),
                ("n_pol_groups", C.c_int32), ("pad2", C.c_int32), ("pol_kind", C.POINTER(C.POINTER(C.c_int32)))]


class NoiseFitSpec(C.Structure):  # vag_noise_fit_spec
    _fields_ = [("n_groups", C.c_int32), ("n_bands", C.c_int32), ("point_group", C.POINTER(C.c_int32)),
                ("band_group", C.POINTER(C.c_int32)), ("sys_fixed", C.c_double * 8), ("calib", C.c_double * 8)]


class CountsObs(C.Structure):  # vag_counts_obs
    _fields_ = [("nu_min", C.c_double), ("nu_max", C.c_double), ("num_points", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("n_samples", C.c_int32), ("t_sample", C.POINTER(C.c_double)), ("sample_idx", C.POINTER(C.c_int32))] + \
               [(n, C.POINTER(C.c_double)) for n in ("counts", "background", "scale", "weight")]


class CountsFitSpec(C.Structure):  # vag_counts_fit_spec
    _fields_ = [("n_groups", C.c_int32), ("pad", C.c_int32), ("groups", C.POINTER(CountsObs))]


INDEX_MAX_NODES = 8  # VAG_INDEX_MAX_NODES


class IndexObs(C.Structure):  # vag_index_obs
    _fields_ = [("n", C.c_int32), ("k", C.c_int32), ("nu", C.POINTER(C.c_double)), ("coef", C.POINTER(C.c_double)),
                ("ext_slope", C.c_double)] + [(n, C.POINTER(C.c_double)) for n in ("t", "value", "err", "weight")]


class IndexFitSpec(C.Structure):  # vag_index_fit_spec
    _fields_ = [("n_groups", C.c_int32), ("pad", C.c_int32), ("groups", C.POINTER(IndexObs))]


FOLD_MAX_BINS, FOLD_MAX_CHANNELS = 64, 256  # VAG_FOLD_MAX_BINS, VAG_FOLD_MAX_CHANNELS


class FoldObs(C.Structure):  # vag_fold_obs
    _fields_ = [(n, C.c_int32) for n in ("J", "C", "n", "m", "n_samples", "pad")] + \
               [(n, C.POINTER(C.c_double)) for n in ("nu", "A", "sigma", "t_sample")] + [("sample_idx", C.POINTER(C.c_int32))] + \
               [(n, C.POINTER(C.c_double)) for n in ("exposure_over_m", "counts", "background", "weight")]


class FoldFitSpec(C.Structure):  # vag_fold_fit_spec
    _fields_ = [("n_groups", C.c_int32), ("pad", C.c_int32), ("groups", C.POINTER(FoldObs)), ("n_h_fixed", C.c_double)]


class TemplateFitSpec(C.Structure):  # vag_template_fit_spec
    _fields_ = [("n_templates", C.c_int32), ("n_bands", C.c_int32), ("point", C.POINTER(C.c_double)),
                ("bands", C.POINTER(C.POINTER(C.c_double))), ("amp_fixed", C.c_double * 8), ("extinguished", C.c_int32 * 8)]


COV_MAX_ROWS, COV_MAX_GROUPS = 256, 8  # VAG_COV_MAX_ROWS, VAG_COV_MAX_GROUPS


class CovObs(C.Structure):  # vag_cov_obs
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32)] + \
               [(n, C.POINTER(C.c_double)) for n in ("t", "nu", "ln_flux", "ext", "whitener")] + [("weight", C.c_double)]


class CovFitSpec(C.Structure):  # vag_cov_fit_spec
    _fields_ = [("n_groups", C.c_int32), ("pad", C.c_int32), ("groups", C.POINTER(CovObs))]


class RobustFitSpec(C.Structure):  # vag_robust_fit_spec
    _fields_ = [("n_groups", C.c_int32), ("mask", C.c_uint32), ("frac_fixed", C.c_double * 8), ("scale_fixed", C.c_double * 8),
                ("shift_fixed", C.c_double * 8)]


class FitSpec(C.Structure):
    _fields_ = [
        ("base", ModelParams), ("ndim", C.c_int32), ("slot", C.c_int32 * 16), ("is_log", C.c_int32 * 16),
        ("n_data", C.c_int32), ("pad", C.c_int32),
        ("t", C.POINTER(C.c_double)), ("nu", C.POINTER(C.c_double)), ("ln_flux", C.POINTER(C.c_double)),
        ("ln_err", C.POINTER(C.c_double)), ("weight", C.POINTER(C.c_double)),
        ("ext_kernel", C.POINTER(C.c_double)), ("a_v_fixed", C.c_double), ("n_bands", C.c_int32), ("pad2", C.c_int32),
        ("bands", C.POINTER(BandObs)),
        # ABI v7: bounds mask + priors on the device
        ("use_priors", C.c_int32), ("pad3", C.c_int32), ("lower", C.c_double * 16), ("upper", C.c_double * 16),
        ("prior_kind", C.c_int32 * 16), ("prior_a", C.c_double * 16), ("prior_b", C.c_double * 16),
    ]


class LoglikeRequest(C.Structure):  # vag_loglike_request: the spec blocks of the widest likelihood entry, None = absent
    _fields_ = [("spec", C.POINTER(FitSpec)), ("sky", C.POINTER(SkyFitSpec)), ("vis", C.POINTER(VisFitSpec)), ("pol", C.POINTER(PolFitSpec)),
                ("lim", C.POINTER(LimitFitSpec)), ("noise", C.POINTER(NoiseFitSpec)), ("counts", C.POINTER(CountsFitSpec)),
                ("index", C.POINTER(IndexFitSpec)), ("fold", C.POINTER(FoldFitSpec)), ("tmpl", C.POINTER(TemplateFitSpec)),
                ("cov", C.POINTER(CovFitSpec)), ("robust", C.POINTER(RobustFitSpec))]


class StretchSpec(C.Structure):  # vag_stretch_spec
    _fields_ = [("seed", C.c_uint64), ("a", C.c_double), ("n_walkers", C.c_int32), ("ndim", C.c_int32), ("thin", C.c_int32)]


STRETCH_ENTRIES = ("vag_stretch_propose_dev", "vag_stretch_accept_dev", "vag_stretch_run_dev")


def _entry(lib, name, needs):
    """An entry point added after ABI 13 and detected by symbol (VAG_LIB_PATH may name an older build); `needs`: what needs it."""
    if not hasattr(lib, name):
        raise RuntimeError(f"the loaded library has no {name}: {needs} a newer build")
    return getattr(lib, name)


def stretch_entry(lib, name):
    """One of the device sampler's entry points."""
    return _entry(lib, name, "the device sampler (sampling.StretchMove, run_stretch_move_device, fit(sampler='device')) needs")


class MoveSpec(C.Structure):  # vag_move_spec
    _fields_ = [("seed", C.c_uint64), ("a", C.c_double), ("gamma0", C.c_double), ("sigma", C.c_double), ("gamma_snooker", C.c_double),
                ("weights", C.c_double * 3), ("n_walkers", C.c_int32), ("ndim", C.c_int32), ("thin", C.c_int32)]


MOVE_STRETCH, MOVE_DE, MOVE_SNOOKER = 0, 1, 2  # VAG_MOVE_*
MOVE_ENTRIES = ("vag_move_propose_dev", "vag_move_accept_dev", "vag_move_run_dev")


def move_entry(lib, name):
    """One of the move-mix entry points."""
    return _entry(lib, name, "the DE and snooker moves (sampling.EnsembleMoves, run_moves_device, fit(sampler='device', moves=...)) need")


class TemperedSpec(C.Structure):  # vag_tempered_spec; betas points into a host array the caller keeps
    _fields_ = [("seed", C.c_uint64), ("a", C.c_double), ("n_temps", C.c_int32), ("n_walkers", C.c_int32), ("ndim", C.c_int32),
                ("thin", C.c_int32), ("betas", C.POINTER(C.c_double))]


TEMPER_MAX = 64  # VAG_TEMPER_MAX
TEMPERED_ENTRIES = ("vag_loglike_split_dev", "vag_tempered_propose_dev", "vag_tempered_accept_dev", "vag_tempered_swap_dev",
                    "vag_tempered_run_dev")


def tempered_entry(lib, name):
    """One of the parallel-tempering entry points."""
    return _entry(lib, name, "parallel tempering (sampling.TemperedMove, run_tempered_device, Fitter.log_like_and_prior_batch, "
                  "fit(sampler='tempered')) needs")


class NestedSpec(C.Structure):  # vag_nested_spec
    _fields_ = [("seed", C.c_uint64), ("n_live", C.c_int32), ("ndim", C.c_int32), ("walk", C.c_int32), ("pad", C.c_int32),
                ("gamma0", C.c_double), ("sigma", C.c_double)]


NESTED_MAX_LIVE = 16384  # VAG_NESTED_MAX_LIVE
NESTED_ENTRIES = ("vag_nested_rank_dev", "vag_nested_retire_dev", "vag_nested_propose_dev", "vag_nested_accept_dev", "vag_nested_run_dev")


def nested_entry(lib, name):
    """One of the nested-sampling entry points."""
    return _entry(lib, name, "nested sampling (sampling.NestedMove, run_nested_device, fit(sampler='nested')) needs")


class ChainSpec(C.Structure):  # vag_chain_spec
    _fields_ = [("nwalkers", C.c_int32), ("ndim", C.c_int32), ("n_rows", C.c_int64), ("row_stride", C.c_int64), ("max_lag", C.c_int32),
                ("c", C.c_double)]


CHAIN_SCRATCH_MAX = 1 << 30  # VAG_CHAIN_SCRATCH_MAX


def chain_entry(lib, name="vag_chain_autocorr_dev"):
    """The chain-autocorrelation entry point."""
    return _entry(lib, name, "the device autocorrelation estimate (sampling.chain_autocorr_device, converge= of the device run drivers, "
                  "the tau of fit(sampler='device')) needs")


class QuantileSpec(C.Structure):  # vag_quantile_spec
    _fields_ = [("nq", C.c_int32), ("pad", C.c_int32), ("q", C.c_double * 16)]


PREDICT_MAX_DRAWS, PREDICT_MAX_Q, PREDICT_MAX_VALUES = 4096, 16, 1 << 27  # VAG_PREDICT_MAX_DRAWS, _Q, _VALUES
PREDICT_ENTRIES = ("vag_column_quantiles_dev", "vag_predict_bands_dev")


def predict_tile_columns(n_draws):
    """vag::predict_tile_columns of csrc/vag_predict.h: adjacent columns per workgroup of the quantile kernel at ``n_draws`` draws."""
    size = 1
    while size < n_draws:
        size <<= 1
    return max(1, min(16, (128 * 1024) // (8 * size)))


def predict_entry(lib, name):
    """One of the two posterior-predictive entry points."""
    return _entry(lib, name, "posterior-predictive bands (sampling.column_quantiles_device, Fitter.predict) need")


PRIOR_UNIFORM, PRIOR_GAUSSIAN, PRIOR_LOG_UNIFORM, PRIOR_NONE, PRIOR_UNIFORM_RANGE = 0, 1, 2, 3, 4


class DetailsShape(C.Structure):
    _fields_ = [("n_phi", C.c_int32), ("n_theta", C.c_int32), ("n_t", C.c_int32), ("n_reps", C.c_int32),
                ("symmetry", C.c_int32), ("phi_mirrored", C.c_int32)]


class DetailsOut(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_double)) for n in
                ("phi", "theta", "t_src", "Gamma", "r", "t_comv", "B", "N_p", "Gamma_th")]


class StageTimes(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("grid_ms", "dynamics_ms", "cells_ms", "flux_ms", "reduce_ms", "total_ms")]


class Profile(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("dynamics", "EAT_grid", "syn_electrons", "syn_photons", "cooling", "sync_flux", "ic_photons",
                                          "ssc_flux", "total")]


class Plan(C.Structure):
    _fields_ = [("n_models_ok", C.c_int32), ("n_rows", C.c_int32), ("n_cells", C.c_int64), ("total_pairs", C.c_int64),
                ("eat_cells", C.c_int64), ("spec_evals", C.c_int64), ("interps", C.c_int64),
                ("flux_blocks", C.c_int32), ("pairs_per_block", C.c_int32),
                ("n_models_invalid", C.c_int32), ("n_models_capacity", C.c_int32),
                ("n_rows_failed", C.c_int32), ("n_rows_gave_up", C.c_int32),
                ("n_walkers_rejected", C.c_int32), ("n_walkers_ssc_failed", C.c_int32),
                ("ic_terms", C.c_int64), ("ic_nodes", C.c_int64), ("n_models_ssc_rebuilt", C.c_int32), ("n_ssc_all_cell_fallbacks", C.c_int32),
                ("ic_pool_bytes", C.c_int64), ("ode_rhs", C.c_int64), ("n_ssc_slow_cells", C.c_int64),
                ("ode_lane_attempts", C.c_int64), ("ode_lane_slots", C.c_int64)]


class Limits(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("max_theta", "max_phi", "max_time", "max_nu")]


EXPORTS = [
    "vag_params_default", "vag_params_validate", "vag_last_error", "vag_version", "vag_abi_version", "vag_reload_env_hooks",
    "vag_device_count", "vag_device_bytes_in_use", "vag_ctx_create", "vag_ctx_destroy", "vag_ctx_set_stream", "vag_ctx_get_stream", "vag_ctx_synchronize",
    "vag_get_limits", "vag_flux_density_grid_batch", "vag_flux_density_grid_components_batch", "vag_flux_components_batch",
    "vag_flux_density_grid_components4_batch", "vag_flux_components4_batch", "vag_flux_density_batch", "vag_flux_batch",
    "vag_flux_density_components4_batch", "vag_flux_density_grid_batch_dev", "vag_flux_density_batch_dev", "vag_loglike_batch", "vag_loglike_batch_dev",
    "vag_last_model_costs_dev", "vag_loglike_shard_dev", "vag_loglike_shard_finish_dev", "vag_loglike_shard_begin_dev", "vag_loglike_shard_end_dev", "vag_loglike_shard_state_dev", "vag_ctx_profile", "vag_last_profile", "vag_details", "vag_details_rvs", "vag_details_radiation", "vag_details_regime", "vag_details_eat", "vag_profile_eval", "vag_last_stage_times", "vag_last_plan", "vag_ctx_count_work",
    "vag_ctx_coalesce", "vag_ctx_coalesce_stats", "vag_flux_density_grid_coalesced", "vag_flux_density_coalesced", "vag_flux_coalesced",
    "vag_sky_image_batch", "vag_sky_moments_batch", "vag_sky_centroid_batch", "vag_loglike_sky_batch", "vag_loglike_sky_batch_dev",
    "vag_sky_visibility_batch", "vag_debug_device_math", "vag_loglike_vis_batch", "vag_loglike_vis_batch_dev",
    "vag_sky_polarization_batch", "vag_sky_stokes_image_batch", "vag_loglike_pol_batch", "vag_loglike_pol_batch_dev",
    "vag_loglike_lim_batch", "vag_loglike_lim_batch_dev", "vag_loglike_noise_batch", "vag_loglike_noise_batch_dev",
    "vag_loglike_counts_batch", "vag_loglike_counts_batch_dev", "vag_loglike_index_batch", "vag_loglike_index_batch_dev",
    "vag_loglike_fold_batch", "vag_loglike_fold_batch_dev", "vag_loglike_tmpl_batch", "vag_loglike_tmpl_batch_dev",
    "vag_loglike_cov_batch", "vag_loglike_cov_batch_dev", "vag_loglike_robust_batch", "vag_loglike_robust_batch_dev", "vag_stretch_propose_dev", "vag_stretch_accept_dev", "vag_stretch_run_dev",
    "vag_loglike_split_dev", "vag_tempered_propose_dev", "vag_tempered_accept_dev", "vag_tempered_swap_dev", "vag_tempered_run_dev",
    "vag_move_propose_dev", "vag_move_accept_dev", "vag_move_run_dev", "vag_chain_autocorr_dev",
    "vag_nested_rank_dev", "vag_nested_retire_dev", "vag_nested_propose_dev", "vag_nested_accept_dev", "vag_nested_run_dev",
    "vag_column_quantiles_dev", "vag_predict_bands_dev",
]

_lib = None
_dp = C.POINTER(C.c_double)
_pp = C.POINTER(ModelParams)


def load():
    """Load the HIP engine; raises ImportError (no silent CPU path) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so); the engine links the system one (/opt/rocm/lib).
    # Both carry the same SONAME, so whichever is mapped first serves both -- and torch does not initialise on the system
    # runtime ("No HIP GPUs are available").  Streams and device pointers are shared with torch (vag_ctx_set_stream, the *_dev
    # entry points), so the process must run ONE runtime: torch's, mapped before the engine.
    try:
        import torch  # noqa: F401
    except ImportError:  # a torch-free process uses the system runtime
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the gfx950 engine first (python -c 'import __graft_entry__ as g; g.build()')")
    lib = C.CDLL(LIB_PATH)
    v = C.c_void_p
    lib.vag_last_error.restype = C.c_char_p
    lib.vag_version.restype = C.c_char_p
    lib.vag_reload_env_hooks.restype = None
    lib.vag_params_default.argtypes = [_pp]
    lib.vag_params_default.restype = None
    lib.vag_params_validate.argtypes = [_pp]
    lib.vag_device_bytes_in_use.restype = C.c_longlong
    lib.vag_ctx_create.argtypes = [C.c_int, C.POINTER(v)]
    lib.vag_ctx_destroy.argtypes = [v]
    lib.vag_ctx_destroy.restype = None
    lib.vag_ctx_set_stream.argtypes = [v, v]
    lib.vag_ctx_get_stream.argtypes = [v, C.POINTER(v)]
    lib.vag_ctx_synchronize.argtypes = [v]
    lib.vag_get_limits.argtypes = [C.POINTER(Limits)]
    lib.vag_get_limits.restype = None
    lib.vag_flux_density_grid_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp]
    lib.vag_flux_density_grid_components_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp, _dp]
    lib.vag_flux_density_grid_components4_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, _dp, C.c_int, C.POINTER(_dp)]
    lib.vag_sky_image_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_double, C.c_int, C.c_int, _dp, _dp]
    lib.vag_sky_moments_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp]
    lib.vag_sky_centroid_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp]
    lib.vag_sky_visibility_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp, _dp, C.c_int, C.c_double, C.c_int, _dp]
    lib.vag_sky_polarization_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, _dp, C.c_int, C.POINTER(PolSpec), C.c_double, C.c_int, _dp]
    lib.vag_sky_stokes_image_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, _dp, C.c_int, C.POINTER(PolSpec), C.c_double, C.c_int,
                                               C.c_int, _dp, _dp]
    lib.vag_debug_device_math.argtypes = [v, C.c_int, _dp, C.c_int, _dp]
    lib.vag_loglike_sky_batch.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), _dp, C.c_int, C.c_int, _dp]
    lib.vag_loglike_sky_batch_dev.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), v, C.c_int, C.c_int, v]
    lib.vag_loglike_vis_batch.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), _dp, C.c_int, C.c_int, _dp]
    lib.vag_loglike_vis_batch_dev.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), v, C.c_int, C.c_int, v]
    lib.vag_loglike_pol_batch.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), C.POINTER(PolFitSpec), _dp,
                                          C.c_int, C.c_int, _dp]
    lib.vag_loglike_pol_batch_dev.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), C.POINTER(PolFitSpec), v,
                                              C.c_int, C.c_int, v]
    lib.vag_loglike_lim_batch.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), C.POINTER(PolFitSpec),
                                          C.POINTER(LimitFitSpec), _dp, C.c_int, C.c_int, _dp]
    lib.vag_loglike_lim_batch_dev.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), C.POINTER(PolFitSpec),
                                              C.POINTER(LimitFitSpec), v, C.c_int, C.c_int, v]
    lib.vag_loglike_noise_batch.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), C.POINTER(PolFitSpec),
                                            C.POINTER(LimitFitSpec), C.POINTER(NoiseFitSpec), _dp, C.c_int, C.c_int, _dp]
    lib.vag_loglike_noise_batch_dev.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), C.POINTER(PolFitSpec),
                                                C.POINTER(LimitFitSpec), C.POINTER(NoiseFitSpec), v, C.c_int, C.c_int, v]
    lib.vag_loglike_counts_batch.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), C.POINTER(PolFitSpec),
                                             C.POINTER(LimitFitSpec), C.POINTER(NoiseFitSpec), C.POINTER(CountsFitSpec), _dp, C.c_int,
                                             C.c_int, _dp]
    lib.vag_loglike_counts_batch_dev.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec),
                                                 C.POINTER(PolFitSpec), C.POINTER(LimitFitSpec), C.POINTER(NoiseFitSpec),
                                                 C.POINTER(CountsFitSpec), v, C.c_int, C.c_int, v]
    lib.vag_loglike_index_batch.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), C.POINTER(PolFitSpec),
                                            C.POINTER(LimitFitSpec), C.POINTER(NoiseFitSpec), C.POINTER(CountsFitSpec),
                                            C.POINTER(IndexFitSpec), _dp, C.c_int, C.c_int, _dp]
    lib.vag_loglike_index_batch_dev.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec),
                                                C.POINTER(PolFitSpec), C.POINTER(LimitFitSpec), C.POINTER(NoiseFitSpec),
                                                C.POINTER(CountsFitSpec), C.POINTER(IndexFitSpec), v, C.c_int, C.c_int, v]
    if hasattr(lib, "vag_loglike_fold_batch"):  # (detected by symbol: VAG_LIB_PATH may name an older build of ABI 13)
        lib.vag_loglike_fold_batch.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), C.POINTER(PolFitSpec),
                                               C.POINTER(LimitFitSpec), C.POINTER(NoiseFitSpec), C.POINTER(CountsFitSpec),
                                               C.POINTER(IndexFitSpec), C.POINTER(FoldFitSpec), _dp, C.c_int, C.c_int, _dp]
        lib.vag_loglike_fold_batch_dev.argtypes = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec),
                                                   C.POINTER(PolFitSpec), C.POINTER(LimitFitSpec), C.POINTER(NoiseFitSpec),
                                                   C.POINTER(CountsFitSpec), C.POINTER(IndexFitSpec), C.POINTER(FoldFitSpec), v, C.c_int,
                                                   C.c_int, v]
    if hasattr(lib, "vag_loglike_tmpl_batch"):  # (detected by symbol, like the fold entry)
        wide = [v, C.POINTER(FitSpec), C.POINTER(SkyFitSpec), C.POINTER(VisFitSpec), C.POINTER(PolFitSpec), C.POINTER(LimitFitSpec),
                C.POINTER(NoiseFitSpec), C.POINTER(CountsFitSpec), C.POINTER(IndexFitSpec), C.POINTER(FoldFitSpec),
                C.POINTER(TemplateFitSpec)]
        lib.vag_loglike_tmpl_batch.argtypes = wide + [_dp, C.c_int, C.c_int, _dp]
        lib.vag_loglike_tmpl_batch_dev.argtypes = wide + [v, C.c_int, C.c_int, v]
        if hasattr(lib, "vag_loglike_cov_batch"):  # (detected by symbol too: the template entry with the correlated groups behind it)
            lib.vag_loglike_cov_batch.argtypes = wide + [C.POINTER(CovFitSpec), _dp, C.c_int, C.c_int, _dp]
            lib.vag_loglike_cov_batch_dev.argtypes = wide + [C.POINTER(CovFitSpec), v, C.c_int, C.c_int, v]
    if hasattr(lib, "vag_loglike_robust_batch"):  # (detected by symbol: the request form, with the outlier groups)
        lib.vag_loglike_robust_batch.argtypes = [v, C.POINTER(LoglikeRequest), _dp, C.c_int, C.c_int, _dp]
        lib.vag_loglike_robust_batch_dev.argtypes = [v, C.POINTER(LoglikeRequest), v, C.c_int, C.c_int, v]
    if hasattr(lib, "vag_stretch_run_dev"):  # (detected by symbol: the device sampler)
        sp = C.POINTER(StretchSpec)
        lib.vag_stretch_propose_dev.argtypes = [v, sp, C.c_uint64, C.c_int, v, v]
        lib.vag_stretch_accept_dev.argtypes = [v, sp, C.c_uint64, C.c_int, v, v, v, v, v]
        lib.vag_stretch_run_dev.argtypes = [v, C.POINTER(LoglikeRequest), sp, C.c_uint64, C.c_int, v, v, v, v, v]
    if hasattr(lib, "vag_move_run_dev"):  # (detected by symbol: the move mix of the device sampler)
        mp = C.POINTER(MoveSpec)
        lib.vag_move_propose_dev.argtypes = [v, mp, C.c_uint64, C.c_int, v, v, v]
        lib.vag_move_accept_dev.argtypes = [v, mp, C.c_uint64, C.c_int, v, v, v, v, v, v]
        lib.vag_move_run_dev.argtypes = [v, C.POINTER(LoglikeRequest), mp, C.c_uint64, C.c_int, v, v, v, v, v]
    if hasattr(lib, "vag_tempered_run_dev"):  # (detected by symbol: parallel tempering)
        tp = C.POINTER(TemperedSpec)
        lib.vag_loglike_split_dev.argtypes = [v, C.POINTER(LoglikeRequest), v, C.c_int, C.c_int, v, v]
        lib.vag_tempered_propose_dev.argtypes = [v, tp, C.c_uint64, C.c_int, v, v]
        lib.vag_tempered_accept_dev.argtypes = [v, tp, C.c_uint64, C.c_int, v, v, v, v, v, v, v]
        lib.vag_tempered_swap_dev.argtypes = [v, tp, C.c_uint64, v, v, v, v]
        lib.vag_tempered_run_dev.argtypes = [v, C.POINTER(LoglikeRequest), tp, C.c_uint64, C.c_int, v, v, v, v, v, v, v, v]
    if hasattr(lib, "vag_nested_run_dev"):  # (detected by symbol: nested sampling)
        ns = C.POINTER(NestedSpec)
        lib.vag_nested_rank_dev.argtypes = [v, ns, v, v, v]
        lib.vag_nested_retire_dev.argtypes = [v, ns, C.c_uint64, v, v, v, v, v, v, v]
        lib.vag_nested_propose_dev.argtypes = [v, ns, C.c_uint64, C.c_int, v, v, v]
        lib.vag_nested_accept_dev.argtypes = [v, ns, C.c_uint64, C.c_int, v, v, v, v, v, v, v, v, v]
        lib.vag_nested_run_dev.argtypes = [v, C.POINTER(LoglikeRequest), ns, C.c_uint64, C.c_int, v, v, v, v, v, v, v]
    if hasattr(lib, "vag_chain_autocorr_dev"):  # (detected by symbol: chain autocorrelation)
        lib.vag_chain_autocorr_dev.argtypes = [v, C.POINTER(ChainSpec), v, v, v, v]
    if hasattr(lib, "vag_predict_bands_dev"):  # (detected by symbol: posterior-predictive bands)
        lib.vag_column_quantiles_dev.argtypes = [v, C.POINTER(QuantileSpec), v, C.c_int, C.c_int, v, v, v, v]
        lib.vag_predict_bands_dev.argtypes = [v, C.POINTER(FitSpec), v, C.c_int, C.c_int, v, C.c_int, v, C.c_int, v, C.POINTER(QuantileSpec),
                                              v, v, v, v]
    lib.vag_flux_density_components4_batch.argtypes = [v, _pp, C.c_int, _dp, _dp, C.c_int, C.POINTER(_dp)]
    lib.vag_flux_components4_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(_dp)]
    lib.vag_flux_density_batch.argtypes = [v, _pp, C.c_int, _dp, _dp, C.c_int, _dp]
    lib.vag_flux_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, C.c_double, C.c_double, C.c_int, _dp]
    lib.vag_ctx_coalesce.argtypes = [v, C.c_int, C.c_int]
    lib.vag_ctx_coalesce_stats.argtypes = [v, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.vag_flux_density_grid_coalesced.argtypes = [v, _pp, _dp, C.c_int, _dp, C.c_int, _dp, C.POINTER(_dp)]
    lib.vag_flux_density_coalesced.argtypes = [v, _pp, _dp, _dp, C.c_int, _dp, C.POINTER(_dp)]
    lib.vag_flux_coalesced.argtypes = [v, _pp, _dp, C.c_int, C.c_double, C.c_double, C.c_int, _dp, C.POINTER(_dp)]
    lib.vag_flux_components_batch.argtypes = [v, _pp, C.c_int, _dp, C.c_int, C.c_double, C.c_double, C.c_int, _dp, _dp]
    lib.vag_flux_density_grid_batch_dev.argtypes = [v, v, C.c_int, v, C.c_int, v, C.c_int, v]
    lib.vag_flux_density_batch_dev.argtypes = [v, v, C.c_int, v, v, C.c_int, v]
    lib.vag_loglike_batch.argtypes = [v, C.POINTER(FitSpec), _dp, C.c_int, C.c_int, _dp]
    lib.vag_loglike_batch_dev.argtypes = [v, C.POINTER(FitSpec), v, C.c_int, C.c_int, v]
    lib.vag_last_model_costs_dev.argtypes = [v, C.c_int, v]
    lib.vag_loglike_shard_dev.argtypes = [v, C.POINTER(FitSpec), v, C.c_int, C.c_int, C.c_int, C.c_int, v]
    lib.vag_loglike_shard_finish_dev.argtypes = [v, v, C.c_int, C.c_int, v]
    lib.vag_loglike_shard_begin_dev.argtypes = [v, C.POINTER(FitSpec), v, C.c_int, C.c_int, C.c_int, C.c_int, v, C.POINTER(C.c_uint64)]
    lib.vag_loglike_shard_end_dev.argtypes = [v, C.c_uint64, v, C.c_int, C.c_int, v]
    lib.vag_loglike_shard_state_dev.argtypes = [v, C.c_int, C.c_int, v, v]
    lib.vag_ctx_profile.argtypes = [v, C.c_int]
    lib.vag_last_profile.argtypes = [v, C.POINTER(Profile)]
    lib.vag_details.argtypes = [v, _pp, C.c_double, C.c_double, C.POINTER(DetailsShape), C.POINTER(DetailsOut)]
    lib.vag_details_rvs.argtypes = [v, _pp, C.c_double, C.c_double, C.POINTER(DetailsShape), C.POINTER(DetailsOut)]
    lib.vag_details_radiation.argtypes = [v, _pp, C.c_double, C.c_double, C.c_int, C.POINTER(_dp)]
    lib.vag_details_regime.argtypes = [v, _pp, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int32)]
    lib.vag_details_eat.argtypes = [v, _pp, C.c_double, C.c_double, C.POINTER(C.c_int), _dp, _dp]
    lib.vag_profile_eval.argtypes = [v, _pp, C.c_int, _dp, C.c_int, _dp]
    lib.vag_last_stage_times.argtypes = [v, C.POINTER(StageTimes)]
    lib.vag_last_plan.argtypes = [v, C.POINTER(Plan)]
    lib.vag_ctx_count_work.argtypes = [v, C.c_int]
    _lib = lib
    return lib


def torch_stream_handle(stream):
    """The void* vag_ctx_set_stream takes for a torch.cuda.Stream: its HIP handle, or VAG_STREAM_LEGACY_DEFAULT for torch's default
    stream (handle 0 = the legacy default stream; a plain 0 would select the context's own stream and the engine would race
    with torch's kernels)."""
    return C.c_void_p(stream.cuda_stream or 1)


def last_error():
    return load().vag_last_error().decode()


def check(rc):
    """Map C-ABI error codes onto the reference's exception types (pybind/error_handling.h:12-27)."""
    if rc == VAG_OK:
        return
    msg = last_error()
    if rc == VAG_E_INVALID:
        raise ValueError(msg)
    if rc == VAG_E_NO_DEVICE:
        raise RuntimeError("vegasafterglow_amd needs a HIP device (no CPU path): " + msg)
    if rc == VAG_E_CAPACITY:
        raise ValueError("engine capacity exceeded: " + msg)
    if rc == VAG_E_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == VAG_E_NUMERIC:
        raise RuntimeError("ODE integration failed: " + msg)  # odeint's step_adjustment_error surfaces as RuntimeError
    if rc == VAG_E_INTERNAL:
        raise RuntimeError("vegasafterglow_amd internal error (please report): " + msg)
    raise RuntimeError(f"vegasafterglow_amd error {rc}: {msg}")


class _Hooks:
    """The engine's developer / test switches are VAG_* environment variables which the library reads ONCE (inside its first call) --
    never on a call path, where getenv would race with another thread's setenv.  A process that flips one later does it through this
    mapping: the variable is set (or removed) in os.environ and the library is told to read its environment again.  Not for use while
    another thread is inside the engine."""

    @staticmethod
    def _reload():
        if os.path.exists(LIB_PATH):
            load().vag_reload_env_hooks()

    def __setitem__(self, name, value):
        os.environ[name] = value
        self._reload()

    def __delitem__(self, name):
        del os.environ[name]
        self._reload()

    def pop(self, name, *default):
        value = os.environ.pop(name, *default)
        self._reload()
        return value

    def get(self, name, default=None):
        return os.environ.get(name, default)

    def __contains__(self, name):
        return name in os.environ


hooks = _Hooks()
