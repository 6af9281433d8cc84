/* exmc_hip_advi.h -- Exmc.ADVI (lib/exmc/advi.ex) on the device: one mean-field fit per lane group,
 * all fits of a call in one launch. Plain C.
 *
 * Fit c of a call is ADVI.fit(ir, seed: seed + 7919 (chain_lo + c)): mu = 0, log_sigma = -1, then up to
 * max_iters iterations of stochastic gradient ascent on the ELBO -- num_mc_samples samples
 * z = mu + exp(log_sigma) eps per iteration with eps from the fit's running generator in the flat order,
 * elbo = logp(z) + sum(log_sigma) + 0.5 d (1 + log 2 pi) (-1.0e10 where logp is not finite),
 * mu += lr g, log_sigma += lr ((g sigma) eps + 1) -- the reference's convergence test on the two halves
 * of the last window_size ELBOs, and num_draws draws mu + exp(log_sigma) normal_s from the generator as
 * the loop left it. DESIGN.md "ADVI" states the semantics and the summation contract; the results are
 * bit-identical to the checker's statement of advi.ex in the lane layout of the launch.
 *
 * Stated deviations from the reference:
 *  - max_iters >= 1, num_draws >= 1, num_mc_samples >= 1 and window_size >= 2, otherwise
 *    EXMC_ERR_BADARG (Elixir's 1..0 counts down and a half window of 0 divides by zero: what the
 *    reference does below these bounds is an accident). window_size has no upper bound but int's; a
 *    window longer than max_iters never fills, so such a fit never converges, as in the reference;
 *  - mu, log_sigma and the draws are in the unconstrained kernel space, in kernel order (the Python
 *    and Elixir callers constrain the draws as they constrain a sampler's trace);
 *  - elbo_history has max_iters entries per fit; those at and after num_iters are NaN;
 *  - where sum(log_sigma) is not finite the reference raises; here the value flows on, a finite logp
 *    then gives a non-finite ELBO, and a window that holds one never passes the test. */
#ifndef EXMC_HIP_ADVI_H
#define EXMC_HIP_ADVI_H

#include <stdint.h>

#include "exmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int num_draws, max_iters, num_mc_samples, window_size;   /* the reference's defaults: 1000, 10000, 1, 100 */
  double learning_rate, convergence_tol;                   /* 0.01, 1e-4 */
  uint64_t seed;
  int lanes_per_chain;                                     /* 0: the model kind's default layout */
} exmc_hip_advi_opts;

/* n_fits fits with the seeds of fits chain_lo .. chain_lo + n_fits - 1 (a caller shards a batch by
 * chain_lo, as with exmc_hip_sample_independent). Device outputs, any of which may be NULL:
 * draws [S][d][C], mu and log_sigma [d][C], elbo_history [max_iters][C], num_iters [C], converged [C]
 * (0 or 1); C = n_fits, S = num_draws.
 *
 * Handle state: the call reads the flat order and nothing else; the flat order, an installed dense
 * mass and resident chains stay in place. The ELBO window is read back from elbo_history; where that
 * is NULL, max_iters * n_fits doubles of scratch are allocated for the call and freed before it
 * returns. A handle with a stream run in flight is refused (EXMC_ERR_BADARG). The kernel time is
 * exmc_hip_last_kernel_ms. */
int exmc_hip_advi(exmc_hip_model* m, exmc_hip_advi_opts o, int n_fits, int chain_lo,
                  double* draws_dev, double* mu_dev, double* log_sigma_dev, double* elbo_history_dev,
                  int32_t* num_iters_dev, int32_t* converged_dev);

/* the same into host arrays in the reference's layout: draws [C][S][d], mu and log_sigma [C][d],
 * elbo_history [C][max_iters], the rest [C]; any may be NULL */
int exmc_hip_advi_host(exmc_hip_model* m, exmc_hip_advi_opts o, int n_fits, int chain_lo,
                       double* draws, double* mu, double* log_sigma, double* elbo_history,
                       int32_t* num_iters, int32_t* converged);

#ifdef __cplusplus
}
#endif

#endif
