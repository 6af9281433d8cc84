/* exmc_hip_compare.h — model comparison entry points of libexmc_hip.so: Exmc.ModelComparison
 * (lib/exmc/model_comparison.ex) over a device trace. Plain C; included by nothing in exmc_hip.h.
 *
 * The unit is the DATUM of a built-in kind (one y_i, one return r_t), whatever way the reference
 * writes the model's likelihood; DESIGN.md "Model comparison" states the contract:
 *   ll_i(theta) per kind (exmc_detmath.h functions, the kind's own transforms), datum order the
 *   handle's (radon: its county-sorted observations);
 *   draws: a device trace [S][d][C] as the sampling kernels write it, pooled to n = S C samples;
 *   stats [4][N]: rows lppd_i = log_mean_exp(ll_i), p_waic_i = variance(ll_i) (divisor n - 1),
 *   elpd_loo_i = -log_mean_exp(-ll_i) (plain importance-sampling LOO, loo_i_basic), p_loo_i =
 *   lppd_i - elpd_loo_i; accumulated over fixed chunks of samples in a fixed order and merged
 *   left to right, so the bits depend on (S, C) and the trace only.
 * EXMC_MODEL_STD_NORMAL (no data) and generated models (EXMC_MODEL_CUSTOM) built without per-datum
 * terms answer EXMC_ERR_UNSUPPORTED: form their ll on the host and use exmc_hip_ic_stats_from_ll. A
 * model generated WITH them (exmc_hip_pointwise.h) answers exmc_hip_model_n_data and the two matrix
 * calls; its reductions are exmc_hip_pointwise_loglik_range and libexmc_hip.so's *_from_ll.
 * Errors: EXMC_ERR_BADARG for a null pointer, d != the model's dimension, n_draws < 1,
 * n_chains < 1 or fewer than 2 samples in all (the variance needs n >= 2).
 *
 * Handle state (exmc_hip.h "Handle state"). The calls read no handle state: their outputs depend on
 * their arguments and the model's data only. They run on the handle's stream, allocate their
 * scratch (chunk partials, a staging copy) for the call alone and free it before they return, when
 * the results are written; exmc_hip_last_kernel_ms times the kernels, not those allocations. Like the diagnostics (ess, ess_bulk, rhat)
 * they leave the flat order, an installed dense mass and resident chains in place: after any of
 * them exmc_hip_chains_advance and the stream continuations go on as if it had not been called.
 */
#ifndef EXMC_HIP_COMPARE_H
#define EXMC_HIP_COMPARE_H

#include "exmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* N, the number of datums of the model, or < 0 when the kind has no per-datum terms */
int exmc_hip_model_n_data(const exmc_hip_model* m);

/* pointwise_log_likelihood/2 (model_comparison.ex:19-50) per datum: ll_dev [S][N][C] */
int exmc_hip_pointwise_loglik(exmc_hip_model* m, const double* draws_dev, int n_draws, int d,
                              int n_chains, double* ll_dev);

/* the four per-datum statistics in one pass over the trace, the matrix never formed:
 * stats_dev [4][N] (lppd, p_waic, elpd_loo, p_loo) */
int exmc_hip_ic_stats(exmc_hip_model* m, const double* draws_dev, int n_draws, int d,
                      int n_chains, double* stats_dev);

/* the same from a host trace in the reference's layout [C][S][d] into host stats [4][N] */
int exmc_hip_ic_stats_host(exmc_hip_model* m, const double* draws_host, int n_draws, int d,
                           int n_chains, double* stats_host);

/* model-free: the statistics of a device matrix ll_dev [S][N][C] on `device`; stats_dev [4][N].
 * Runs on the null stream of that device and returns when the results are written. A generated
 * model's plug-in carries no comparison kernels and answers EXMC_ERR_UNSUPPORTED: call libexmc_hip.so. */
int exmc_hip_ic_stats_from_ll(int device, const double* ll_dev, int n_draws, int n_data,
                              int n_chains, double* stats_dev);

#ifdef __cplusplus
}
#endif

/* PSIS-LOO with the Pareto k diagnostic: the exmc_hip_psis_* entry points, part of this interface */
#include "exmc_hip_psis.h"
/* the per-datum terms of a block of datums: what generated models take part through */
#include "exmc_hip_pointwise.h"

#endif
