/* exmc_hip_ppc.h -- posterior predictive checks of a built-in model kind on the device: where every
 * observation falls among its replicates, the replicates' mean and spread per datum, and four test
 * statistics of every replicated data set against the observed one (the Bayesian p-values), without the
 * replicate matrix. Plain C. DESIGN.md "Posterior predictive checks" states the contract; ppc_kernel
 * (exmc_amd/csrc/exmc_ppc.hpp) is the kernel; tests/ppc_statement.py restates the arithmetic.
 *
 * Replicates. Exactly those of exmc_hip_posterior_predictive (exmc_hip_predictive.h) at the same handle,
 * trace, seed and chain_lo: chain c's generator is seeded seed + 7919 (chain_lo + c) and walks the draws
 * ascending and within a draw the datums ascending in the handle's order; the samplers, the gamma cap
 * and the parameters per kind are the same. No generator state goes in or comes out: opts.resume != 0 is
 * EXMC_ERR_BADARG. y_i is the observed value of datum i in the handle's order, n = S C, every product
 * and sum rounded separately (-ffp-contract=off).
 *
 * Per datum, reduced over chains and draws. Chains form blocks of 64: block b holds chains 64 b ..
 * 64 b + 63 of the call, whatever chain_lo is, B = ceil(C / 64). For datum i and block b, from E = 0,
 * E2 = 0, n_lt = 0, n_eq = 0:
 *   for s = 0 .. S - 1, for c ascending over the block's chains that exist:
 *     e = yrep - y_i;  E = E + e;  E2 = E2 + e * e;  n_lt += (yrep < y_i);  n_eq += (yrep == y_i)
 * one running sum per (b, i), strictly left to right. A NaN replicate is in neither count and makes the
 * two sums NaN.
 *   datum_sums   [B][N][2] double:  E, E2
 *   datum_counts [B][N][2] int64:   n_lt, n_eq
 * Finished on the host (here in the _host form, in numpy in exmc_amd/predictive.py, the same
 * expressions), the blocks summed left to right, b ascending, from 0:
 *   mean_i = y_i + E / n;  var_i = (E2 - (E * E) / n) / (n - 1);  p_lt_i = n_lt / n;  p_eq_i = n_eq / n
 *
 * Per replicated data set (s, c), i ascending. m0 = (sum_i y_i, left to right from 0) / N is the
 * observed mean. From A = 0, Bq = 0, mn = +inf, mx = -inf, for each replicate v:
 *   e = v - m0;  A = A + e;  Bq = Bq + e * e;  mn = (v < mn) ? v : mn;  mx = (v > mx) ? v : mx
 *   T_mean = m0 + A / N;  T_var = (Bq - (A * A) / N) / (N - 1);  T_min = mn;  T_max = mx
 * t_obs[4] are the same expressions over y, formed on the host before the launch.
 *   chain_counts [4][C] int32: per statistic k (mean, var, min, max) and chain, the draws with
 *                              T_k >= t_obs[k]; a NaN compares false
 *   tstat        [S][4][C] double, optional
 * The Bayesian p-value of statistic k is (sum_c chain_counts[k][c]) / n, an integer sum.
 *
 * Sharding. Every output word depends on the chains of one block alone (or of one chain), and every
 * word has one writer: a batch cut into shards at multiples of 64 chains, chain_lo set to each shard's
 * first chain, gives the whole call's blocks, chain_counts and tstat columns, bit for bit.
 *
 * EXMC_MODEL_STD_NORMAL (no data) and generated models (EXMC_MODEL_CUSTOM) answer EXMC_ERR_UNSUPPORTED.
 * Errors: EXMC_ERR_BADARG for a null trace or a null required output, d != the model's dimension,
 * n_draws < 1, n_chains < 1, chain_lo < 0, resume != 0, or a handle with a stream run in flight.
 *
 * Handle state (exmc_hip.h "Handle state"): the call reads none and changes none. It runs on the
 * handle's stream and returns when the results are written; exmc_hip_last_kernel_ms times the kernel. */
#ifndef EXMC_HIP_PPC_H
#define EXMC_HIP_PPC_H

#include <stdint.h>

#include "exmc_hip_predictive.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EXMC_PPC_BLOCK 64   /* chains per block of the per-datum sums */
#define EXMC_PPC_NSTAT 4    /* mean, var, min, max */

/* draws_dev [S][d][C] -> datum_sums_dev [B][N][2], datum_counts_dev [B][N][2], chain_counts_dev [4][C]
 * and, where it is given, tstat_dev [S][4][C], all on the device and written whole (nothing is read
 * from them); t_obs [4] and m0 on the host. y_obs [N] on the host is optional: the observed values in
 * the handle's order, which the finishing expressions take. N = exmc_hip_model_n_data. */
int exmc_hip_ppc(exmc_hip_model* m, exmc_hip_predictive_opts opts, const double* draws_dev, int n_draws, int d,
                 int n_chains, double* datum_sums_dev, int64_t* datum_counts_dev, int32_t* chain_counts_dev,
                 double* tstat_dev, double* t_obs, double* m0, double* y_obs);

/* the same in the reference's layouts, finished: host draws [C][S][d] in; datum [N][4] (mean, var, p_lt,
 * p_eq), t_obs [4], p_value [4] out; tstat [C][S][4] optional */
int exmc_hip_ppc_host(exmc_hip_model* m, exmc_hip_predictive_opts opts, const double* draws, int n_draws, int d,
                      int n_chains, double* datum, double* t_obs, double* p_value, double* tstat);

#ifdef __cplusplus
}
#endif

#endif
