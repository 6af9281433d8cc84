/* exmc_hip_pathfinder.h -- Exmc.Pathfinder (lib/exmc/pathfinder.ex) on the device: one L-BFGS path
 * per lane group, all paths of a call in one launch. Plain C.
 *
 * Path c of a call is Pathfinder.fit(ir, seed: seed + 7919 (chain_lo + c)): the start
 * q0[r] = 0.1 normal_s in the flat order, max_iters steps q + 0.01 direction of the two-loop L-BFGS
 * recursion over at most history_size pairs, a diagonal normal (mu = q, sigma = 1 / sqrt(|g| + 1e-6))
 * at every path point, the first point of the largest ELBO, and num_draws draws mu + sigma normal_s
 * from the generator as it was seeded (so the first d variates are q0 / 0.1, as in the reference).
 * DESIGN.md "Pathfinder" states the semantics and the summation contract; the results are
 * bit-identical to the checker's statement of pathfinder.ex in the lane layout of the launch.
 *
 * Stated deviations from the reference:
 *  - max_iters >= 1, num_draws >= 1 and 1 <= history_size <= EXMC_PF_MAX_HISTORY, otherwise
 *    EXMC_ERR_BADARG (the bound is a compile-time one; 6 is the reference's default);
 *  - a path point whose ELBO is not finite is never selected (the reference raises for the fit);
 *  - a path with no finite ELBO reports status 1, best_index -1, and NaN elbo, mu, sigma and draws;
 *  - mu, sigma and the draws are in the unconstrained kernel space, in kernel order (the Python and
 *    Elixir callers constrain the draws as they constrain a sampler's trace). */
#ifndef EXMC_HIP_PATHFINDER_H
#define EXMC_HIP_PATHFINDER_H

#include <stdint.h>

#include "exmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EXMC_PF_MAX_HISTORY 6

typedef struct {
  int num_draws, max_iters, history_size;   /* the reference's defaults: 1000, 100, 6 */
  uint64_t seed;
  int lanes_per_chain;                      /* 0: the model kind's default layout */
} exmc_hip_pf_opts;

/* n_paths paths with the seeds of paths chain_lo .. chain_lo + n_paths - 1 (a caller shards a batch
 * by chain_lo, as with exmc_hip_sample_independent). Device outputs, any of which may be NULL:
 * draws [S][d][C], mu and sigma [d][C], elbo [C], num_iters [C] (the path length, 1 + accepted steps),
 * best_index [C] (the path point taken), status [C]; C = n_paths, S = num_draws.
 *
 * Handle state: the call reads the flat order and nothing else; the flat order, an installed dense
 * mass and resident chains stay in place. Its scratch is allocated for the call and freed before it
 * returns. A handle with a stream run in flight is refused (EXMC_ERR_BADARG). The kernel time is
 * exmc_hip_last_kernel_ms. */
int exmc_hip_pathfinder(exmc_hip_model* m, exmc_hip_pf_opts o, int n_paths, int chain_lo,
                        double* draws_dev, double* mu_dev, double* sigma_dev, double* elbo_dev,
                        int32_t* num_iters_dev, int32_t* best_index_dev, int32_t* status_dev);

/* the same into host arrays in the reference's layout: draws [C][S][d], mu and sigma [C][d], the
 * rest [C]; any may be NULL */
int exmc_hip_pathfinder_host(exmc_hip_model* m, exmc_hip_pf_opts o, int n_paths, int chain_lo,
                             double* draws, double* mu, double* sigma, double* elbo,
                             int32_t* num_iters, int32_t* best_index, int32_t* status);

#ifdef __cplusplus
}
#endif

#endif
