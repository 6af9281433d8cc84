/* exmc_hip_smc_bridge.h -- bridged SMC: the tempered sampler of exmc_hip_smc.h with its start divided out
 * of the weights, and an estimate of the log evidence. Plain C. DESIGN.md "Bridged SMC" is the contract.
 *
 * The temper runs along the geometric bridge from a normalised diagonal normal q0 = N(mu, diag sigma^2),
 * the base, to the model's density: log pi_beta = beta logp + (1 - beta) log q0. Beside q and logp every
 * particle carries lb = log q0(q), the logq of exmc_hip_fit_psis.h in its EXMC_FIT_SIGMA form. What differs
 * from exmc_hip_smc.h:
 *  - the base: mu [d] and sigma [d] in kernel order, one pair per call shared by its runs; a NULL mu is
 *    0.0 and a NULL sigma 0.5 (the start of exmc_hip_smc.h). Both finite with sigma > 0, otherwise
 *    EXMC_ERR_BADARG (init and the whole-run forms read them back and check; mutate trusts what init took);
 *  - the start is q = mu + sigma * v per flat entry, the generators and seeds those of exmc_hip_smc.h;
 *  - the weights are of lr = logp - lb. A stage first evaluates the ESS at 1.0 - beta and goes to beta =
 *    1.0 when it is at or above the threshold; otherwise the bisection of exmc_hip_smc.h runs on lr;
 *  - log_evidence [R] is the sum over the stages of inc = mx + log(sw / N), mx and sw the maximum and the
 *    sum of the stage's unnormalised weights; log_evidence_steps [max_stages][R] holds inc per stage, NaN
 *    at and after num_stages. It estimates log of the integral of exp(logp), log p(y) as far as the
 *    model's densities carry their constants (the built kinds do);
 *  - every stage of an active run resamples, with one uniform of the run generator; lb is gathered with
 *    q and logp;
 *  - a proposal is judged on the bridge: log_alpha = (beta logp' + (1 - beta) lb') - (beta logp + (1 -
 *    beta) lb); a NaN log_alpha (beta = 1.0 with lb' = -inf) rejects.
 * max_stages, status, the three histories, the options and their checks, the handle-state rules and a
 * plug-in library's answers are those of exmc_hip_smc.h, whose structs these functions take. */
#ifndef EXMC_HIP_SMC_BRIDGE_H
#define EXMC_HIP_SMC_BRIDGE_H

#include <stdint.h>

#include "exmc_hip_smc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The steps, on device arrays the caller owns: those of exmc_hip_smc_init / _mutate / _reweight, and
 * logb [C], log_evidence [R], log_evidence_steps [max_stages][R], none NULL; mu_dev and sigma_dev [d] or
 * NULL. The order of a run is that of exmc_hip_smc.h. init fills logb and sets log_evidence to 0.0 and
 * log_evidence_steps to NaN; reweight adds the stage's inc; mutate carries lb with the particle. A
 * plug-in library carries init and mutate and answers EXMC_ERR_UNSUPPORTED to reweight. */
int exmc_hip_smc_bridge_init(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, const double* mu_dev,
                             const double* sigma_dev, double* q_dev, double* logp_dev, double* logb_dev,
                             uint64_t* rng_words_dev, exmc_hip_smc_state st, double* log_evidence_dev,
                             double* log_evidence_steps_dev);
int exmc_hip_smc_bridge_mutate(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, const double* mu_dev,
                               const double* sigma_dev, double* q_dev, double* logp_dev, double* logb_dev,
                               uint64_t* rng_words_dev, exmc_hip_smc_state st);
int exmc_hip_smc_bridge_reweight(int device, exmc_hip_smc_opts o, int n_runs, int d, int stage, double* q_dev,
                                 double* logp_dev, double* logb_dev, exmc_hip_smc_state st, double* log_evidence_dev,
                                 double* log_evidence_steps_dev);

/* The whole of n_runs runs for the built model kinds (a plug-in answers EXMC_ERR_UNSUPPORTED): the device
 * outputs of exmc_hip_smc and logb [C], log_evidence [R], log_evidence_steps [max_stages][R]; any may be
 * NULL. mu_dev and sigma_dev are device arrays [d] or NULL. */
int exmc_hip_smc_bridge(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, const double* mu_dev,
                        const double* sigma_dev, double* particles_dev, double* logp_dev, double* logb_dev,
                        double* betas_dev, double* ess_history_dev, double* acceptance_rates_dev,
                        int32_t* num_stages_dev, int32_t* status_dev, double* log_evidence_dev,
                        double* log_evidence_steps_dev);

/* the same from and into host arrays: mu and sigma [d] or NULL; the layout of exmc_hip_smc_host, logb
 * [R][N], log_evidence [R], log_evidence_steps [R][max_stages]; any output may be NULL */
int exmc_hip_smc_bridge_host(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, const double* mu,
                             const double* sigma, double* particles, double* logp, double* logb, double* betas,
                             double* ess_history, double* acceptance_rates, int32_t* num_stages, int32_t* status,
                             double* log_evidence, double* log_evidence_steps);

#ifdef __cplusplus
}
#endif

#endif
