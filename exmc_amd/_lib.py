"""ctypes binding of libexmc_hip.so (include/exmc_hip.h). No CPU fallback: if the library or a
HIP device is missing, calls raise ExmcHipError."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EXMC_HIP_LIB") or os.path.join(HERE, "lib", "libexmc_hip.so")

MAX_D = 256
OK, ERR_BADARG, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED = range(5)

EXPORTS = [
    "exmc_hip_last_error", "exmc_hip_device_count", "exmc_hip_model_create",
    "exmc_hip_model_destroy", "exmc_hip_model_dim", "exmc_hip_model_default_lanes", "exmc_hip_model_default_warmup_lanes",
    "exmc_hip_model_default_dense_lanes",
    "exmc_hip_model_stream", "exmc_hip_logp_grad_host", "exmc_hip_multi_step",
    "exmc_hip_multi_step_host", "exmc_hip_transitions_host", "exmc_hip_warmup",
    "exmc_hip_sample_chains", "exmc_hip_sample_chains_host", "exmc_hip_sample_host",
    "exmc_hip_chains_init", "exmc_hip_chains_advance", "exmc_hip_build_full_tree_host",
    "exmc_hip_ess", "exmc_hip_last_kernel_ms",
    "exmc_hip_traj_create", "exmc_hip_traj_destroy", "exmc_hip_traj_get_endpoint_host",
    "exmc_hip_traj_build_and_merge_host", "exmc_hip_traj_is_terminated_host",
    "exmc_hip_traj_get_result_host", "exmc_hip_build_subtree_host",
    "exmc_hip_stream_begin", "exmc_hip_stream_next_host", "exmc_hip_stream_start", "exmc_hip_stream_finish", "exmc_hip_rhat", "exmc_hip_ess_bulk",
    "exmc_hip_model_set_flat_order", "exmc_hip_warmup_from", "exmc_hip_sample_warm_host",
    "exmc_hip_warmup_dense", "exmc_hip_model_set_dense_mass", "exmc_hip_model_clear_dense_mass",
    "exmc_hip_sample_dense_host",
    "exmc_hip_sample_independent", "exmc_hip_sample_independent_host",
    "exmc_hip_leapfrog_chain_normal_host",
]

# include/exmc_hip_compare.h: model comparison (WAIC / LOO) over a device trace
COMPARE_EXPORTS = [
    "exmc_hip_model_n_data", "exmc_hip_pointwise_loglik", "exmc_hip_ic_stats",
    "exmc_hip_ic_stats_host", "exmc_hip_ic_stats_from_ll",
]

# include/exmc_hip_psis.h (the end of exmc_hip_compare.h): PSIS-LOO with the Pareto k diagnostic
PSIS_EXPORTS = ["exmc_hip_psis_stats", "exmc_hip_psis_stats_host", "exmc_hip_psis_stats_from_ll"]

# include/exmc_hip_pointwise.h (the end of exmc_hip_compare.h): the per-datum terms of a block of datums
POINTWISE_EXPORTS = ["exmc_hip_pointwise_loglik_range"]

# include/exmc_hip_pathfinder.h: Exmc.Pathfinder, one L-BFGS path per lane group
PATHFINDER_EXPORTS = ["exmc_hip_pathfinder", "exmc_hip_pathfinder_host"]
PF_MAX_HISTORY = 6

# include/exmc_hip_advi.h: Exmc.ADVI, one mean-field fit per lane group
ADVI_EXPORTS = ["exmc_hip_advi", "exmc_hip_advi_host"]

# include/exmc_hip_smc.h: Exmc.SMC, one particle per lane group
SMC_EXPORTS = ["exmc_hip_smc_init", "exmc_hip_smc_mutate", "exmc_hip_smc_reweight", "exmc_hip_smc", "exmc_hip_smc_host"]
SMC_DEFAULT_MAX_STAGES = 1000

# include/exmc_hip_smc_bridge.h: bridged SMC, the start divided out of the weights, with a log evidence
SMC_BRIDGE_EXPORTS = ["exmc_hip_smc_bridge_init", "exmc_hip_smc_bridge_mutate", "exmc_hip_smc_bridge_reweight",
                      "exmc_hip_smc_bridge", "exmc_hip_smc_bridge_host"]

# include/exmc_hip_fit_psis.h: the Pareto-smoothed importance ratios of the fits' draws and their resampling
FIT_PSIS_EXPORTS = ["exmc_hip_fit_log_ratio", "exmc_hip_ratio_psis_from_lr", "exmc_hip_ratio_gather",
                    "exmc_hip_fit_psis", "exmc_hip_fit_psis_host"]
FIT_SIGMA, FIT_LOG_SIGMA = 0, 1
FIT_PSIS_ROWS = ("khat", "log_mean_ratio", "ess", "n_zero", "tail")

# include/exmc_hip_predictive.h: Exmc.Predictive.posterior_predictive, one chain's generator per lane
PREDICTIVE_EXPORTS = ["exmc_hip_posterior_predictive", "exmc_hip_posterior_predictive_host"]

# include/exmc_hip_prior.h: Exmc.Predictive.prior_samples, the prior walk and the datums' replicates per lane
PRIOR_EXPORTS = ["exmc_hip_prior_samples", "exmc_hip_prior_samples_host"]

# include/exmc_hip_ppc.h: posterior predictive checks, the replicates reduced where they are drawn
PPC_EXPORTS = ["exmc_hip_ppc", "exmc_hip_ppc_host"]
PPC_BLOCK = 64

# include/exmc_hip_loo_pit.h: PSIS-LOO-PIT, the replicates weighted with the smoothed LOO weights
LOO_PIT_EXPORTS = ["exmc_hip_loo_pit", "exmc_hip_loo_pit_host", "exmc_hip_loo_pit_from_ll"]
LOO_PIT_ROWS = ("p_lt", "p_eq", "pit", "k")

# include/exmc_hip_convergence.h: rank-normalised R-hat and bulk / tail / mean ESS across chains
CONVERGENCE_EXPORTS = ["exmc_hip_convergence", "exmc_hip_convergence_host"]
CONVERGENCE_ROWS = ("rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")


class ExmcHipError(RuntimeError):
    pass


class Opts(C.Structure):
    _fields_ = [("num_warmup", C.c_int), ("num_samples", C.c_int), ("max_tree_depth", C.c_int),
                ("target_accept", C.c_double), ("seed", C.c_uint64), ("lanes_per_chain", C.c_int)]


class Tuning(C.Structure):
    _fields_ = [("epsilon", C.c_double), ("inv_mass", C.c_double * MAX_D),
                ("warmup_divergences", C.c_int)]


class PfOpts(C.Structure):
    _fields_ = [("num_draws", C.c_int), ("max_iters", C.c_int), ("history_size", C.c_int),
                ("seed", C.c_uint64), ("lanes_per_chain", C.c_int)]


class SmcOpts(C.Structure):
    _fields_ = [("num_particles", C.c_int), ("threshold_ratio", C.c_double), ("num_mh_steps", C.c_int),
                ("seed", C.c_uint64), ("max_stages", C.c_int), ("lanes_per_chain", C.c_int)]


class SmcState(C.Structure):
    """exmc_hip_smc_state: device pointers"""
    _fields_ = [(k, C.c_void_p) for k in ("beta", "run_rng", "active", "scale", "accept", "betas", "ess_history",
                                          "acceptance_rates", "num_stages", "status", "active_count")]


class AdviOpts(C.Structure):
    _fields_ = [("num_draws", C.c_int), ("max_iters", C.c_int), ("num_mc_samples", C.c_int),
                ("window_size", C.c_int), ("learning_rate", C.c_double), ("convergence_tol", C.c_double),
                ("seed", C.c_uint64), ("lanes_per_chain", C.c_int)]


class PredictiveOpts(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("chain_lo", C.c_int), ("resume", C.c_int)]


class Trace(C.Structure):
    _fields_ = [("draws", C.c_void_p), ("logp", C.c_void_p), ("tree_depth", C.c_void_p),
                ("n_steps", C.c_void_p), ("divergent", C.c_void_p), ("accept_prob", C.c_void_p),
                ("energy", C.c_void_p)]


_libs = {}


def load():
    """Load libexmc_hip.so. torch (if used in the same process) must be imported first so both
    share one HIP runtime; exmc_amd/__init__ takes care of the order."""
    return bind(LIB_PATH)


def bind(path):
    """Load a library with the include/exmc_hip.h ABI: libexmc_hip.so itself or a plug-in build
    made for one generated model (exmc_amd/codegen.py)."""
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ExmcHipError(
            "%s is not built: run `python -m exmc_amd.build` (or codegen.build_plugin for a "
            "generated model); there is no CPU fallback" % path)
    L = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    vp = C.c_void_p
    L.exmc_hip_last_error.restype = C.c_char_p
    L.exmc_hip_device_count.restype = C.c_int
    L.exmc_hip_model_create.argtypes = [C.c_int, C.c_int, dp, C.c_int, C.c_int, C.POINTER(vp)]
    L.exmc_hip_model_destroy.argtypes = [vp]
    L.exmc_hip_model_destroy.restype = None
    L.exmc_hip_model_dim.argtypes = [vp]
    L.exmc_hip_model_set_flat_order.argtypes = [vp, C.POINTER(C.c_int32), C.c_int]
    L.exmc_hip_model_default_lanes.argtypes = [vp]
    L.exmc_hip_model_default_warmup_lanes.argtypes = [vp]
    L.exmc_hip_model_default_dense_lanes.argtypes = [vp]
    L.exmc_hip_model_stream.argtypes = [vp]
    L.exmc_hip_model_stream.restype = vp
    L.exmc_hip_logp_grad_host.argtypes = [vp, dp, C.c_int, C.c_int, dp, dp]
    L.exmc_hip_multi_step.argtypes = [vp, vp, vp, vp, C.c_double, dp, C.c_int, C.c_int, C.c_int,
                                      vp, vp, vp, vp]
    L.exmc_hip_multi_step_host.argtypes = [vp, dp, dp, dp, C.c_double, dp, C.c_int, C.c_int,
                                           C.c_int, dp, dp, dp, dp]
    L.exmc_hip_transitions_host.argtypes = [vp, dp, dp, dp, C.POINTER(C.c_uint64), C.c_int,
                                            C.c_int, C.c_double, dp, C.c_int, C.c_int, Trace]
    L.exmc_hip_warmup.argtypes = [vp, dp, Opts, C.POINTER(Tuning)]
    L.exmc_hip_sample_chains.argtypes = [vp, C.POINTER(Tuning), dp, C.c_int, C.c_int, C.c_int,
                                         Opts, Trace, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    L.exmc_hip_sample_chains_host.argtypes = L.exmc_hip_sample_chains.argtypes
    L.exmc_hip_chains_init.argtypes = [vp, C.POINTER(Tuning), dp, C.c_int, C.c_int, C.c_int, Opts]
    L.exmc_hip_chains_advance.argtypes = [vp, C.c_int, C.c_int, Trace, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int32)]
    L.exmc_hip_sample_host.argtypes = [vp, dp, Opts, Trace, C.POINTER(Tuning),
                                       C.POINTER(C.c_int32)]
    L.exmc_hip_warmup_dense.argtypes = [vp, dp, Opts, C.POINTER(Tuning), dp, dp]
    L.exmc_hip_model_set_dense_mass.argtypes = [vp, dp, dp, C.c_int]
    L.exmc_hip_sample_dense_host.argtypes = [vp, dp, Opts, Trace, C.POINTER(Tuning), dp, dp, C.POINTER(C.c_int32)]
    L.exmc_hip_model_clear_dense_mass.argtypes = [vp]
    L.exmc_hip_warmup_from.argtypes = [vp, dp, Opts, C.POINTER(Tuning), C.POINTER(Tuning)]
    L.exmc_hip_sample_warm_host.argtypes = [vp, dp, Opts, C.POINTER(Tuning), Trace, C.POINTER(Tuning),
                                            C.POINTER(C.c_int32)]
    ip = C.POINTER(C.c_int32)
    L.exmc_hip_build_full_tree_host.argtypes = [
        C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, C.c_int, dp, dp, dp, dp,
        C.c_int, dp, dp, C.c_int, C.POINTER(C.c_uint64), dp, dp, dp, ip, ip, dp, ip]
    L.exmc_hip_stream_begin.argtypes = [vp, dp, Opts, C.POINTER(Tuning)]
    L.exmc_hip_stream_next_host.argtypes = [vp, C.c_int, Trace, ip]
    L.exmc_hip_stream_start.argtypes = [vp, C.c_int, C.POINTER(Trace), C.POINTER(ip)]
    L.exmc_hip_stream_finish.argtypes = [vp, ip]
    up = C.POINTER(C.c_uint64)
    L.exmc_hip_traj_create.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, C.POINTER(vp)]
    L.exmc_hip_traj_destroy.argtypes = [vp]
    L.exmc_hip_traj_destroy.restype = None
    L.exmc_hip_traj_get_endpoint_host.argtypes = [vp, ip, dp, dp, dp]
    L.exmc_hip_traj_build_and_merge_host.argtypes = [vp, dp, dp, dp, dp, C.c_int, dp, dp, ip, ip, up]
    L.exmc_hip_traj_is_terminated_host.argtypes = [vp, ip]
    L.exmc_hip_traj_get_result_host.argtypes = [vp, dp, dp, dp, ip, ip, dp, ip]
    L.exmc_hip_build_subtree_host.argtypes = [
        C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, C.c_int, dp, dp, ip, ip, up,
        dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, ip, ip, dp, ip, ip, dp]
    L.exmc_hip_leapfrog_chain_normal_host.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp, dp, C.c_int, C.c_double,
                                                      C.c_double, C.c_double, dp, dp, dp, dp]
    L.exmc_hip_sample_independent.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, Opts, Trace, dp,
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    L.exmc_hip_sample_independent_host.argtypes = L.exmc_hip_sample_independent.argtypes
    L.exmc_hip_ess.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.exmc_hip_rhat.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.exmc_hip_ess_bulk.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.exmc_hip_last_kernel_ms.argtypes = [vp]
    L.exmc_hip_last_kernel_ms.restype = C.c_double
    L.exmc_hip_model_n_data.argtypes = [vp]
    L.exmc_hip_pointwise_loglik.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.exmc_hip_pointwise_loglik_range.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.exmc_hip_ic_stats.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.exmc_hip_ic_stats_host.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, dp]
    L.exmc_hip_ic_stats_from_ll.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]
    L.exmc_hip_psis_stats.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, vp]
    L.exmc_hip_psis_stats_host.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, C.c_size_t, dp]
    L.exmc_hip_psis_stats_from_ll.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]
    L.exmc_hip_pathfinder.argtypes = [vp, PfOpts, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.exmc_hip_pathfinder_host.argtypes = [vp, PfOpts, C.c_int, C.c_int, dp, dp, dp, dp, ip, ip, ip]
    L.exmc_hip_advi.argtypes = [vp, AdviOpts, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.exmc_hip_advi_host.argtypes = [vp, AdviOpts, C.c_int, C.c_int, dp, dp, dp, dp, ip, ip]
    L.exmc_hip_smc_init.argtypes = [vp, SmcOpts, C.c_int, C.c_int, vp, vp, vp, SmcState]
    L.exmc_hip_smc_mutate.argtypes = [vp, SmcOpts, C.c_int, vp, vp, vp, SmcState]
    L.exmc_hip_smc_reweight.argtypes = [C.c_int, SmcOpts, C.c_int, C.c_int, C.c_int, vp, vp, SmcState]
    L.exmc_hip_smc.argtypes = [vp, SmcOpts, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.exmc_hip_smc_host.argtypes = [vp, SmcOpts, C.c_int, C.c_int, dp, dp, dp, dp, dp, ip, ip]
    L.exmc_hip_smc_bridge_init.argtypes = [vp, SmcOpts, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, SmcState, vp, vp]
    L.exmc_hip_smc_bridge_mutate.argtypes = [vp, SmcOpts, C.c_int, vp, vp, vp, vp, vp, vp, SmcState]
    L.exmc_hip_smc_bridge_reweight.argtypes = [C.c_int, SmcOpts, C.c_int, C.c_int, C.c_int, vp, vp, vp, SmcState, vp, vp]
    L.exmc_hip_smc_bridge.argtypes = [vp, SmcOpts, C.c_int, C.c_int, vp, vp] + [vp] * 10
    L.exmc_hip_smc_bridge_host.argtypes = [vp, SmcOpts, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, ip, ip, dp, dp]
    L.exmc_hip_fit_log_ratio.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.exmc_hip_ratio_psis_from_lr.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, vp, vp, vp]
    L.exmc_hip_ratio_gather.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.exmc_hip_fit_psis.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_uint64, vp, vp, vp, vp, vp, vp]
    L.exmc_hip_fit_psis_host.argtypes = [vp, dp, dp, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_uint64, dp, dp, ip, dp, dp, dp]
    L.exmc_hip_posterior_predictive.argtypes = [vp, PredictiveOpts, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.exmc_hip_posterior_predictive_host.argtypes = [vp, PredictiveOpts, dp, C.c_int, C.c_int, C.c_int, up, dp]
    L.exmc_hip_prior_samples.argtypes = [vp, PredictiveOpts, C.c_int, C.c_int, vp, vp, vp, vp]
    L.exmc_hip_prior_samples_host.argtypes = [vp, PredictiveOpts, C.c_int, C.c_int, up, dp, dp, dp]
    L.exmc_hip_ppc.argtypes = [vp, PredictiveOpts, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, dp, dp, dp]
    L.exmc_hip_ppc_host.argtypes = [vp, PredictiveOpts, dp, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp]
    L.exmc_hip_loo_pit.argtypes = [vp, PredictiveOpts, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, vp]
    L.exmc_hip_loo_pit_host.argtypes = [vp, PredictiveOpts, dp, C.c_int, C.c_int, C.c_int, C.c_size_t, dp]
    L.exmc_hip_loo_pit_from_ll.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.exmc_hip_convergence.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, vp]
    L.exmc_hip_convergence_host.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, C.c_size_t, dp]
    _libs[path] = L
    return L


def check(rc, L=None):
    if rc != OK:
        msg = (L or load()).exmc_hip_last_error()
        raise ExmcHipError("libexmc_hip error %d: %s" % (rc, msg.decode() if msg else ""))
