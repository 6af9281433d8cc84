/* exmc_hip_convergence.h -- convergence diagnostics ACROSS chains on the device: rank-normalised and
 * folded split R-hat, bulk and tail ESS, the ESS of the mean and its Monte Carlo standard error, after
 * Vehtari, Gelman, Simpson, Carpenter and Buerkner, "Rank-normalization, folding, and localization"
 * (2021). Model-free: the call reads a trace [S][d][C] and no model (d is the trace's, not the
 * handle's), so a plug-in library of a generated model has it too. The reference has none of this;
 * DESIGN.md "Convergence diagnostics across chains" says why it is here. tests/convergence_statement.py
 * restates the contract in numpy; the device equals it byte for byte.
 *
 * Numeric contract. -ffp-contract=off: products and sums round separately. log is exmc_log
 * (exmc_detmath.h); sqrt and / are IEEE. Per dimension of the trace:
 *
 *   Split.  n = S div 2, M = 2 C. Split chain k = 2 c + half holds x[half n + i], i = 0 .. n-1 (the
 *     split of exmc_hip_rhat; with odd S the last draw is unused). N = M n pooled values. A dimension
 *     with a NaN among its N used values has all six outputs NaN; that is decided before any sorting.
 *   Scores.  r = the average 1-based rank among the N pooled values, ties by == (-0.0 and 0.0 tie);
 *     z = probit((r - 0.375) / (N + 0.25)) with the probit of exmc_hip_ess_bulk, the reference's
 *     rational approximation (4.5e-4 absolute: the stated deviation from the paper's exact inverse).
 *     Ranks are integers (or halves), so how they are found is free.
 *   Quantiles.  Of the pooled values sorted ascending, Diagnostics.quantile (diagnostics.ex:170-180):
 *     h = (N - 1) p, lo_val + frac (hi_val - lo_val); med at 0.5, q05 at 0.05, q95 at 0.95.
 *   Derived series, M chains of n each:  z;  zf = the scores of fabs(x - med), ranked over the pool
 *     again;  i05 = (x <= q05) ? 1.0 : 0.0, i95 likewise with q95;  x itself.
 *   R-hat of a series y (no further splitting).  mean_k = (sum_i y_i, left to right) / n,
 *     var_k = (sum_i (y_i - mean_k)^2, left to right) / (n - 1); then over k = 0 .. M-1, left to right,
 *     gm = (sum mean_k) / M, b = sum (mean_k - gm)^2, w = sum var_k, b = (double)n / (M - 1) * b,
 *     w = w / M, var_hat = (double)(n - 1) / n * w + b / n, R-hat = sqrt(var_hat / w) -- the
 *     expressions of exmc_hip_rhat with len = n and m = M.  rhat_bulk is that of z, rhat_tail of zf.
 *   ESS of a series y.  c_i = y_i - mean_k;  acov_k(t) = (sum_{i=0}^{n-t-1} c_i c_{i+t}, left to
 *     right) / n;  A(t) = (sum_k acov_k(t), k ascending) / M;  W = (sum_k acov_k(0) * n / (n - 1)) / M;
 *     gm = (sum_k mean_k) / M;  Bn = (sum_k (mean_k - gm)^2) / (M - 1);  var_plus = W * (n - 1) / n + Bn.
 *     If !(var_plus > 0) the ESS is NaN. Otherwise rho(0) = 1, rho(t) = 1 - (W - A(t)) / var_plus;
 *     tau = -1, prev = +inf; for j = 0, 1, ... while 2 j + 1 <= n - 1:  P = rho(2j) + rho(2j+1); stop
 *     at the first !(P > 0);  P = (P < prev) ? P : prev;  tau = tau + 2 * P;  prev = P.  Then
 *     tau = max(tau, exmc_log(10.0) / exmc_log((double)N)) (the ESS is at most N log10 N) and
 *     ESS = N / tau.  This is Geyer's initial positive and initial monotone sequence; Stan's extra
 *     treatment of the last odd term is not taken.
 *   Outputs.  ess_bulk = ESS(z);  ess_tail = NaN if ESS(i05) or ESS(i95) is NaN, else the smaller;
 *     ess_mean = ESS(x);  mcse_mean = sqrt(var_plus(x) / ess_mean).
 *
 * Only lags in front of a series' cut are ever used: the device computes them sixteen at a time and
 * stops per dimension and series; the values that are used are the same bits.
 *
 * Scratch. The call walks the dimensions in blocks whose working set (about 40 N bytes a dimension)
 * fits scratch_bytes (0: EXMC_CONVERGENCE_DEFAULT_SCRATCH; never fewer than one dimension a block).
 * The result does not depend on the blocking. The scratch is allocated for the call and freed before
 * it returns.
 *
 * Errors: EXMC_ERR_BADARG for a null pointer, n_draws < 8, n_chains < 1, d < 1, N above 2^31 - 1, or a
 * handle with a stream run in flight.
 *
 * Handle state (exmc_hip.h "Handle state"): the call reads none and changes none. It runs on the
 * handle's stream and returns when the results are written; exmc_hip_last_kernel_ms covers its
 * launches. */
#ifndef EXMC_HIP_CONVERGENCE_H
#define EXMC_HIP_CONVERGENCE_H

#include <stddef.h>

#include "exmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EXMC_CONVERGENCE_NOUT 6   /* rhat_bulk, rhat_tail, ess_bulk, ess_tail, ess_mean, mcse_mean */
#define EXMC_CONVERGENCE_DEFAULT_SCRATCH (4ull << 30)   /* 4 GiB */

/* draws_dev [S][d][C] -> out_dev [6][d], both on the device */
int exmc_hip_convergence(exmc_hip_model* m, const double* draws_dev, int n_draws, int d, int n_chains,
                         size_t scratch_bytes, double* out_dev);

/* the same from a host trace in the reference's layout [C][S][d] into host out [6][d] */
int exmc_hip_convergence_host(exmc_hip_model* m, const double* draws_host, int n_draws, int d,
                              int n_chains, size_t scratch_bytes, double* out_host);

#ifdef __cplusplus
}
#endif

#endif
