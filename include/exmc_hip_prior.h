/* exmc_hip_prior.h -- Exmc.Predictive.prior_samples (lib/exmc/predictive.ex:19-33) on the device: draws of
 * every free variable of a built-in model kind from its prior, and prior predictive replicates of every
 * datum. Plain C.
 *
 * Chain c of a call is prior_samples(ir, S, seed: seed + 7919 (chain_lo + c)): one generator
 * seed_s(:exsss, .) per chain walks the draws s = 0 .. S - 1 (predictive.ex:27-30). Within a draw the
 * free variables come in the order of the reference's topo_sort / kahn_sort (:140-196) over the IR the
 * kind stands for after Rewrite.apply: always the smallest ready id by string comparison, the string
 * order being the handle's flat order (exmc_hip_model_set_flat_order; the string sort of the kind's names
 * by default, radon's caller passes it). For simple, eight_schools, logistic and radon that is the flat
 * order itself; for sv it is nu, sigma, s_1, ..., s_100; for sv_ncp the rewritten s_2 .. s_100 have no
 * parents and come in string order before sigma, and s_1 comes last. Then the datums follow in the
 * handle's order, exactly as exmc_hip_posterior_predictive walks them (exmc_hip_predictive.h).
 *
 * Every variable is the sample/2 of its family, Nx.to_number of the parameters first:
 *   Normal       mu + sigma * normal_s                          (normal.ex:33-39)
 *   HalfCauchy   scale * exmc_tan_halfpi(uniform_s)              (half_cauchy.ex:34-40)
 *   Exponential  (-exmc_log(uniform_s)) / lambda                 (exponential.ex:26-31)
 * The literals are those of the kind's log-density (where the reference writes an f32 tensor, the f32
 * value: sv's nu ~ Exponential((double)0.1f)); a parameter that refers to a parent takes the parent's
 * sampled, constrained value (resolve_params, :115-120). DESIGN.md "Prior predictive" has the table.
 *
 * Stated deviations from the reference:
 *  - the reference has one generator: here every chain has its own, seeded as
 *    exmc_hip_posterior_predictive seeds them;
 *  - the datums come after the free variables, in the handle's order (the reference walks an observed
 *    rv node in id order with the rest);
 *  - the tangent is exmc_tan_halfpi (exmc_detmath.h), the tangent of the exact (pi/2) u and not of the
 *    rounded product :math.pi() * u * 0.5, and :math.log is exmc_log;
 *  - uniform_s = 0.0 gives +inf from Exponential and 0.0 from HalfCauchy, where Erlang's :math.log(0.0)
 *    would raise (and the position of such a variable is exmc_log of that value);
 *  - for sv_ncp the children of a non-centred variable see the reconstructed walk, not the raw N(0, 1)
 *    value that predictive.ex, which ignores ncp_info, would hand them;
 *  - the reference kinds' Custom likelihoods have no sample_fn, so the datum replicates are defined
 *    here: pp_sample(src.params(datum, row, consts)) at the unconstrained row q of the draw, the very
 *    bits exmc_hip_posterior_predictive has at that row.
 *
 * Outputs. x_dev and q_dev are [S][d][C], in exactly the layout and row order that
 * exmc_hip_posterior_predictive reads from this handle (kernel order): x holds the constrained values,
 * q the unconstrained position (exmc_log for a :log variable), so q is a valid trace for
 * posterior_predictive, ppc and the pointwise terms. For sv_ncp the trace rows of s_2 .. s_100 hold the
 * raw z_t, and q holds them; x holds the walk s_t = s_{t-1} + sigma z_t as the kernels reconstruct it
 * from q (sigma = exp(clamp200(q_sigma))).
 * yrep_dev is [S][N][C], N = exmc_hip_model_n_data, or NULL: then no datum is drawn and the generator
 * does not advance for the datums, so the variables of draw s + 1 differ from a call with yrep.
 * rng_state_dev [2][C] is optional, as in exmc_hip_predictive.h: out always, in with opts.resume.
 *
 * EXMC_MODEL_STD_NORMAL and generated models (EXMC_MODEL_CUSTOM) answer EXMC_ERR_UNSUPPORTED.
 * Errors: EXMC_ERR_BADARG for a null x or q, n_draws < 1, n_chains < 1, chain_lo < 0, resume without
 * a state, or a handle with a stream run in flight.
 *
 * Handle state (exmc_hip.h "Handle state"): the call reads the flat order and changes nothing. It runs
 * on the handle's stream and returns when the results are written; the flat order, an installed dense
 * mass and resident chains stay in place. exmc_hip_last_kernel_ms times the kernel. */
#ifndef EXMC_HIP_PRIOR_H
#define EXMC_HIP_PRIOR_H

#include <stdint.h>

#include "exmc_hip_predictive.h"

#ifdef __cplusplus
extern "C" {
#endif

int exmc_hip_prior_samples(exmc_hip_model* m, exmc_hip_predictive_opts opts, int n_draws, int n_chains,
                           uint64_t* rng_state_dev, double* x_dev, double* q_dev, double* yrep_dev);

/* the same in the reference's layouts: host x [C][S][d], q [C][S][d] and yrep [C][S][N] (or NULL) out;
 * rng_state [2][C] on the host, optional */
int exmc_hip_prior_samples_host(exmc_hip_model* m, exmc_hip_predictive_opts opts, int n_draws, int n_chains,
                                uint64_t* rng_state, double* x, double* q, double* yrep);

#ifdef __cplusplus
}
#endif

#endif
