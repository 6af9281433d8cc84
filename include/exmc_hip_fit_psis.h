/* exmc_hip_fit_psis.h -- importance diagnostics of the variational fits (exmc_hip_pathfinder,
 * exmc_hip_advi): the Pareto-smoothed importance ratios p(x) / q(x) of a fit's own draws, their
 * Pareto k as the answer to "is this approximation usable" (Yao, Vehtari, Simpson, Gelman 2018), and
 * importance resampling of the draws, per fit or pooled over all fits (multi-path Pathfinder, Zhang,
 * Carpenter, Gelman, Vehtari 2022). Plain C. DESIGN.md "Importance diagnostics of the fits" states the
 * contract; tests/fit_psis_statement.py restates the estimator from the papers and
 * tests/host/fit_psis_host_checker.c the device's orders, which the device equals byte for byte.
 *
 * Numeric contract. -ffp-contract=off: products and sums round separately. exp, log, log1p and expm1
 * are those of exmc_detmath.h; sqrt and / are IEEE.
 *
 *   Log ratio.  Fit c is the diagonal normal (mu, sigma) over the d unconstrained dimensions in kernel
 *     order, its draws the column c of draws [S][d][C]. Per draw: logp = the model's log-density as the
 *     sampler evaluates it in the lane layout of the launch; z_r = (x_r - mu_r) / sigma_r;
 *     t_r = 0.5 * (z_r * z_r) + ls_r; logq = -(sum_r t_r) - c with the lane layout's sum over the
 *     dimensions from 0.0 (DESIGN.md section 2 "Reductions", the sum Pathfinder's dot products take) and
 *     c = 0.5 d log(2 pi) from libm on the host; lr = logp - logq. With EXMC_FIT_SIGMA the scale array
 *     is sigma and ls = log(sigma); with EXMC_FIT_LOG_SIGMA it is log_sigma, ls the array and
 *     sigma = exp(log_sigma), as exmc_hip_advi forms it for its draws.
 *     lr = -inf where logp is NaN or -inf, or where the draw or its fit's mu or scale array holds a
 *     non-finite value: such a draw has weight zero. logp = +inf otherwise gives lr = NaN.
 *   Groups.  The samples smoothed together: per fit (pooled = 0) the S draws of a fit, k = s, G = n_fits
 *     groups; pooled (pooled = 1) all n = S n_fits samples, k = s n_fits + c, G = 1. Each draw's ratio
 *     is taken under its own fit's approximation.
 *   PSIS.  Per group as exmc_hip_compare.h "PSIS-LOO" with x_k = lr_k - max lr: M = ceil(min(n / 5,
 *     3 sqrt n)), the cutoff the (M + 1)-th largest x (log DBL_MIN where n <= M) and at least
 *     log DBL_MIN, the tail {x > cutoff} of T samples sorted by (x, k), T > 4 for a fit, the
 *     Zhang-Stephens fit with PSIS' prior, the smoothed tail, then min(x, 0.0). Three differences:
 *     a ratio of -inf is admitted (it counts in n, never enters the tail and contributes exp(-inf) = 0);
 *     a group with a NaN or +inf ratio has every output NaN; so has a group without a finite ratio.
 *   Weights.  L1 = lse(x) and L2 = lse(2 x): online log-sum-exps in sample order over chunks of
 *     ic_chunk(n) samples, the chunk states merged left to right. out [5][G]: khat;
 *     log_mean_ratio = (max lr + L1) - log((double)n); ess = exp(2 L1 - L2); n_zero = the number of
 *     -inf ratios; T. lw_k = x_k - L1, the normalised smoothed log weights, in the layout of lr.
 *   Resampling.  Systematic, R draws from the n weights of a group g (smc.ex:180-195): w_k = exp(lw_k);
 *     the cumulative sum in blocks of 4096 consecutive samples, r_k the running sum inside the block
 *     left to right from 0.0, base_b the sum of the earlier blocks' totals left to right from 0.0,
 *     cum_k = base_b + r_k; u = the first uniform of the generator seeded with seed + 7919 g;
 *     pos_j = (u + (double)j) / (double)R; idx_j = the first k with cum_k >= pos_j, n - 1 if there is
 *     none. A group whose outputs are NaN has idx = -1 and NaN draws.
 *
 * Errors: EXMC_ERR_BADARG for a null required pointer, n_draws < 1, n_fits < 1, n_resample < 0, a
 * scale_kind that is neither, d other than the model's dimension, a pooled n above 2^31 - 1, or a handle
 * with a stream run in flight. A plug-in library of a generated model carries exmc_hip_fit_log_ratio
 * and answers EXMC_ERR_UNSUPPORTED to the others: libexmc_hip.so's model-free calls serve its ratios.
 *
 * Handle state (exmc_hip.h "Handle state"): the calls that take a handle read the model and nothing
 * else; the flat order, an installed dense mass and resident chains stay in place. Scratch is
 * allocated for the call and freed before it returns. They run on the handle's stream and return when
 * the results are written; exmc_hip_last_kernel_ms covers their launches. The model-free calls run on
 * the null stream of `device`, like exmc_hip_psis_stats_from_ll. */
#ifndef EXMC_HIP_FIT_PSIS_H
#define EXMC_HIP_FIT_PSIS_H

#include <stdint.h>

#include "exmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EXMC_FIT_SIGMA 0
#define EXMC_FIT_LOG_SIGMA 1
#define EXMC_FIT_PSIS_NOUT 5   /* khat, log_mean_ratio, ess, n_zero, T */

/* draws_dev [S][d][C], mu_dev and scale_dev [d][C] -> lr_dev [S][C] and, unless NULL, logp_dev [S][C];
 * C = n_fits, S = n_draws; lanes_per_chain 0: the model kind's default layout */
int exmc_hip_fit_log_ratio(exmc_hip_model* m, const double* draws_dev, const double* mu_dev,
                           const double* scale_dev, int scale_kind, int n_draws, int d, int n_fits,
                           int lanes_per_chain, double* lr_dev, double* logp_dev);

/* lr_dev [S][C] -> out_dev [5][G]; unless NULL, lw_dev [S][C]; with n_resample = R > 0, idx_dev [R][G]
 * (the sample index k inside the group) */
int exmc_hip_ratio_psis_from_lr(int device, const double* lr_dev, int n_draws, int n_fits, int pooled,
                                int n_resample, uint64_t seed, double* out_dev, double* lw_dev,
                                int32_t* idx_dev);

/* draws_dev [S][d][C], idx_dev [R][G] -> out_dev [R][d][G]: the draws the indices name, NaN where an
 * index is negative or not below n */
int exmc_hip_ratio_gather(int device, const double* draws_dev, const int32_t* idx_dev, int n_draws, int d,
                          int n_fits, int pooled, int n_resample, double* out_dev);

/* the whole chain on the handle's stream: the log ratios, the smoothing and, with n_resample > 0, the
 * resampling and the gather. lw_dev, lr_dev and logp_dev [S][C], idx_dev [R][G] and resampled_dev
 * [R][d][G] may each be NULL */
int exmc_hip_fit_psis(exmc_hip_model* m, const double* draws_dev, const double* mu_dev,
                      const double* scale_dev, int scale_kind, int n_draws, int d, int n_fits,
                      int lanes_per_chain, int pooled, int n_resample, uint64_t seed, double* out_dev,
                      double* lw_dev, int32_t* idx_dev, double* resampled_dev, double* lr_dev,
                      double* logp_dev);

/* the same from and into host arrays in the reference's layouts: draws [C][S][d], mu and scale [C][d];
 * out [5][G]; lw, lr and logp [C][S]; per fit idx [C][R] and resampled [C][R][d]; pooled idx [R] (the
 * pooled index k = s C + c) and resampled [R][d]. Every output but out may be NULL */
int exmc_hip_fit_psis_host(exmc_hip_model* m, const double* draws, const double* mu, const double* scale,
                           int scale_kind, int n_draws, int d, int n_fits, int lanes_per_chain, int pooled,
                           int n_resample, uint64_t seed, double* out, double* lw, int32_t* idx,
                           double* resampled, double* lr, double* logp);

#ifdef __cplusplus
}
#endif

#endif
