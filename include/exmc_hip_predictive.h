/* exmc_hip_predictive.h -- Exmc.Predictive.posterior_predictive (lib/exmc/predictive.ex) on the device:
 * replicates of every datum of a built-in model kind, drawn from a device trace. Plain C.
 *
 * The unit is the datum of a built-in kind, as in exmc_hip_compare.h (one y_i, one return r_t, whatever
 * way the reference writes the likelihood node), in the handle's datum order (radon: county-sorted).
 * Chain c of a call is posterior_predictive(ir, trace_c, seed: seed + 7919 (chain_lo + c)): one
 * generator seed_s(:exsss, .) per chain walks the draws s = 0 .. S - 1 and within a draw the datums
 * i = 0 .. N - 1 (predictive.ex:44-63, 98-108), each datum's replicate the sample/2 of its family at the
 * parameters the kind's likelihood has at draw s:
 *   Normal     loc + scale * normal_s                                      (normal.ex:33-39)
 *   Bernoulli  u = uniform_s; 1.0 if u < p, else 0.0; p unclipped, NaN p gives 0.0   (bernoulli.ex:36-41)
 *   StudentT   z = normal_s; chi2 = sample_gamma(df / 2.0, 0.5); loc + (scale * z) / sqrt(chi2 / df)
 *                                                                          (student_t.ex:38-46)
 *   sample_gamma  Marsaglia-Tsang with the alpha < 1 boost                 (gamma.ex:43-72)
 * DESIGN.md "Posterior predictive" states the parameters per kind and the arithmetic; the results are
 * bit-identical to the checker's statement of these texts (tests/predictive_statement.py).
 *
 * Stated deviations from the reference:
 *  - the reference is handed one trace and has one generator: here every chain has its own, seeded as
 *    exmc_hip_sample_independent and exmc_hip_advi seed theirs;
 *  - the reference walks the obs nodes of the IR in map order: here the datums in the handle's order;
 *  - :math.pow(u, 1.0 / alpha) of the boost is exmc_exp((1.0 / alpha) * exmc_log(u)), and :math.log is
 *    exmc_log (exmc_detmath.h; libm's pow is not in the numeric contract); sqrt and / are IEEE;
 *  - a gamma variate whose Marsaglia loop rejects EXMC_PREDICTIVE_GAMMA_CAP times in a row is NaN, and
 *    the generator goes on from where the rejections left it (a boosted variate still draws its
 *    uniform). The reference would loop on; no input may make a launch run without end.
 * EXMC_MODEL_STD_NORMAL (no data) and generated models (EXMC_MODEL_CUSTOM) answer EXMC_ERR_UNSUPPORTED.
 * Errors: EXMC_ERR_BADARG for a null trace or output, d != the model's dimension, n_draws < 1,
 * n_chains < 1, chain_lo < 0, resume without a state, or a handle with a stream run in flight.
 *
 * Handle state (exmc_hip.h "Handle state"): the call reads none and changes none. It runs on the
 * handle's stream and returns when the results are written; the flat order, an installed dense mass
 * and resident chains stay in place. exmc_hip_last_kernel_ms times the kernel. */
#ifndef EXMC_HIP_PREDICTIVE_H
#define EXMC_HIP_PREDICTIVE_H

#include <stdint.h>

#include "exmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EXMC_PREDICTIVE_GAMMA_CAP 64

typedef struct {
  uint64_t seed;
  int chain_lo;   /* chain c draws with the seed of chain chain_lo + c (a caller shards a batch by it) */
  int resume;     /* 0: seed the generators; 1: take them from rng_state, as an earlier call left them */
} exmc_hip_predictive_opts;

/* draws_dev [S][d][C] (a device trace as the sampling kernels write it) -> yrep_dev [S][N][C], N =
 * exmc_hip_model_n_data (exmc_hip_compare.h). rng_state_dev [2][C] of uint64_t is optional: where it is
 * given the call leaves every chain's generator in it, and with opts.resume it starts from it, so
 * that draws 0 .. S - 1 of one call equal draws 0 .. S1 - 1 and S1 .. S - 1 of two, bit for bit. */
int exmc_hip_posterior_predictive(exmc_hip_model* m, exmc_hip_predictive_opts opts, const double* draws_dev,
                                  int n_draws, int d, int n_chains, uint64_t* rng_state_dev, double* yrep_dev);

/* the same in the reference's layouts: host draws [C][S][d] in, host yrep [C][S][N] out; rng_state
 * [2][C] on the host, optional */
int exmc_hip_posterior_predictive_host(exmc_hip_model* m, exmc_hip_predictive_opts opts, const double* draws,
                                       int n_draws, int d, int n_chains, uint64_t* rng_state, double* yrep);

#ifdef __cplusplus
}
#endif

#endif
