/* exmc_hip_smc.h -- Exmc.SMC (lib/exmc/smc.ex) on the device: tempered sequential Monte Carlo with one
 * particle per lane group, a batch of independent runs in one call. Plain C.
 *
 * Run r of a call is SMC.sample(ir, num_particles: N, threshold_ratio:, num_mh_steps:, seed:
 * seed + 7919 (run_lo + r)): N particles 0.5 normal_s in the flat order, then stages until beta reaches
 * 1.0 -- the next beta by the reference's bisection on the ESS of the incremental weights, systematic
 * resampling when the stage's ESS is below threshold_ratio N, a per-dimension random-walk scale from
 * the particles, num_mh_steps Metropolis proposals per particle at the new beta. DESIGN.md "SMC" states
 * the semantics and the summation contract (particle_sum); the results are bit-identical to the
 * checker's statement of smc.ex in the lane layout of the launch.
 *
 * Stated deviations from the reference:
 *  - the generators: the reference threads one generator through a run. Here seed_r = seed + 7919
 *    (run_lo + r); the run generator rng_seed(seed_r) serves only the one uniform of each resampling;
 *    slot j has the particle generator rng_seed(seed_r ^ ((uint64_t)(j + 1) << 32)), which stays with
 *    the slot through a resampling and is kept in device memory between stages; the generators of a
 *    finished run do not advance;
 *  - at u = 0 in the acceptance test (probability 2^-53) the reference raises; here the proposal is
 *    accepted;
 *  - max_stages (0: 1000) bounds the loop, since the bisection can return beta itself: status is 0
 *    when the run finished at beta = 1.0 and 1 when the bound ended it, the outputs then being the
 *    state after the last stage. betas, ess_history and acceptance_rates have max_stages entries per
 *    run, NaN at and after num_stages;
 *  - num_particles >= 1, num_mh_steps >= 1, threshold_ratio finite, max_stages >= 0, otherwise
 *    EXMC_ERR_BADARG;
 *  - the particles are in the unconstrained kernel space, in kernel order.
 * The algorithm is the reference's as it is: it tempers the whole log density, not the likelihood
 * alone, and starts from N(0, 0.25) without a correction for that start. */
#ifndef EXMC_HIP_SMC_H
#define EXMC_HIP_SMC_H

#include <stdint.h>

#include "exmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int num_particles;        /* the reference's defaults: 500, 0.5, 5, 0 */
  double threshold_ratio;
  int num_mh_steps;
  uint64_t seed;
  int max_stages;           /* 0: 1000 */
  int lanes_per_chain;      /* 0: the model kind's default layout */
} exmc_hip_smc_opts;

#define EXMC_SMC_DEFAULT_MAX_STAGES 1000

/* The state of the runs of a call between its steps: device arrays the caller owns, none NULL.
 * R = n_runs, C = R * num_particles, d the model's dimension. */
typedef struct {
  double* beta;               /* [R] */
  uint64_t* run_rng;          /* [2][R]: the run generators */
  int32_t* active;            /* [R]: 1 while the run goes on */
  double* scale;              /* [d][R] */
  int32_t* accept;            /* [C]: acceptances of the last mutation */
  double* betas;              /* [max_stages][R] */
  double* ess_history;        /* [max_stages][R] */
  double* acceptance_rates;   /* [max_stages][R] */
  int32_t* num_stages;        /* [R] */
  int32_t* status;            /* [R] */
  int32_t* active_count;      /* [1]: the runs that go on, written by every reweight */
} exmc_hip_smc_state;

/* The steps, on device arrays the caller owns: q [d][C], logp [C], rng_words [2][C] (the particle
 * generators). A run is
 *     init; for stage = 0, 1, ...: reweight(stage); stop when *active_count == 0; mutate
 * with the last reweight (at most the one at stage == max_stages) closing the histories.
 *
 * exmc_hip_smc_init and exmc_hip_smc_mutate launch the model's kernels on the handle's stream, between
 * its events (exmc_hip_last_kernel_ms), and wait; a plug-in library carries them. init fills q, logp,
 * the generators and the whole state. mutate does the stage's num_mh_steps proposals of every particle
 * of an active run in place. */
int exmc_hip_smc_init(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, double* q_dev,
                      double* logp_dev, uint64_t* rng_words_dev, exmc_hip_smc_state st);
int exmc_hip_smc_mutate(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, double* q_dev, double* logp_dev,
                        uint64_t* rng_words_dev, exmc_hip_smc_state st);

/* The model-free front of stage `stage`, on the null stream: the acceptance rates of the stage before,
 * which runs go on and their count; for those the bisection, the weights and the ESS, the resampling
 * (q and logp gathered through scratch of the call), the scale and the history entries. A plug-in
 * library answers EXMC_ERR_UNSUPPORTED: use libexmc_hip.so's. */
int exmc_hip_smc_reweight(int device, exmc_hip_smc_opts o, int n_runs, int d, int stage, double* q_dev,
                          double* logp_dev, exmc_hip_smc_state st);

/* The whole of n_runs runs with the seeds of runs run_lo .. run_lo + n_runs - 1, for the built model
 * kinds (a plug-in answers EXMC_ERR_UNSUPPORTED: its caller loops over the steps). Device outputs, any
 * of which may be NULL: particles [d][C], logp [C], betas, ess_history and acceptance_rates
 * [max_stages][R], num_stages and status [R].
 *
 * The stage loop is on the host: it reads one int32 per stage and ends when no run goes on. Handle
 * state: the call reads the flat order and nothing else; the flat order, an installed dense mass and
 * resident chains stay in place. Scratch lives for the call. A handle with a stream run in flight is
 * refused (EXMC_ERR_BADARG). exmc_hip_last_kernel_ms is the sum over the call's kernels. */
int exmc_hip_smc(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, double* particles_dev,
                 double* logp_dev, double* betas_dev, double* ess_history_dev, double* acceptance_rates_dev,
                 int32_t* num_stages_dev, int32_t* status_dev);

/* the same into host arrays in the reference's layout: particles [R][N][d], logp [R][N], the
 * histories [R][max_stages], num_stages and status [R]; any may be NULL */
int exmc_hip_smc_host(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, double* particles,
                      double* logp, double* betas, double* ess_history, double* acceptance_rates,
                      int32_t* num_stages, int32_t* status);

#ifdef __cplusplus
}
#endif

#endif
