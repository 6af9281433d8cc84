/* exmc_hip_loo_pit.h -- PSIS-LOO-PIT of a built-in model kind on the device: the probability integral
 * transform of every observation under its leave-one-out predictive distribution, the replicates of
 * exmc_hip_posterior_predictive re-weighted with the Pareto-smoothed importance weights of PSIS-LOO
 * (Vehtari, Gelman, Gabry 2017; Gabry et al. 2019, "Visualization in Bayesian workflow"; ArviZ loo_pit).
 * Plain C. DESIGN.md "LOO-PIT" states the contract; the kernels are exmc_amd/csrc/exmc_loo_pit.hpp;
 * tests/loo_pit_statement.py restates the estimator, tests/host/loo_pit_host_checker.c the arithmetic.
 *
 * Samples. The pooled samples of the call are k = s C + c, n = S C, over the chains of the call. Per
 * datum i, in the handle's order:
 *   ll_{k,i}  the bits of exmc_hip_pointwise_loglik (exmc_hip_compare.h);
 *   lw_{k,i}  the smoothed log weight of PSIS-LOO (exmc_hip_psis.h, DESIGN.md "PSIS-LOO", r_eff = 1):
 *             x = -ll - max_k(-ll); for a sample of a smoothed datum's tail (x > cutoff) the entry of the
 *             sorted, smoothed tail found by (x, k); then fmin(x, 0.0). M, the cutoff with its
 *             log DBL_MIN floor, the T > 4 rule and the Zhang-Stephens fit are those of PSIS-LOO;
 *   v_{k,i}   the replicate of exmc_hip_posterior_predictive (exmc_hip_predictive.h) at the same handle,
 *             trace, seed and chain_lo; y_i is the observed value of datum i.
 *
 * Accumulation. Chains form blocks of 64: block b holds chains 64 b .. 64 b + 63 of the call,
 * B = ceil(C / 64). Per datum and block the state is (m, sA, sL, sQ), from (-inf, 0, 0, 0): one running
 * maximum m of lw and three sums of exp(lw - m), over all samples (sA), over those with v < y (sL) and
 * over those with v == y (sQ), so that a sample costs one exponential; every weight is at most 1 and
 * nothing overflows. For s = 0 .. S - 1, for c ascending over the block's chains that exist, the push of
 * x = lw with fL = (v < y), fQ = (v == y) as 0.0 or 1.0 (a NaN replicate is in neither set and counts in
 * sA):
 *   x NaN:      m = sA = sL = sQ = x
 *   x == -inf:  nothing changes
 *   x > m:      r = exp(m - x);  sA = sA * r + 1;  sL = sL * r + fL;  sQ = sQ * r + fQ;  m = x
 *               (from m = -inf, r = 0)
 *   x == m:     sA = sA + 1;  sL = sL + fL;  sQ = sQ + fQ
 *   otherwise:  e = exp(x - m);  sA = sA + e;  sL = sL + e where fL;  sQ = sQ + e where fQ
 * exp is exmc_exp of exmc_detmath.h; every product and sum is rounded separately (-ffp-contract=off).
 *
 * Finish, on the device. The blocks are merged left to right, b ascending, (m, sA, sL, sQ) taking
 * (m2, a2, l2, q2):
 *   m or m2 NaN:  all four NaN
 *   m2 == -inf:   nothing changes
 *   m == -inf:    the state becomes (m2, a2, l2, q2)
 *   m == m2:      sA = sA + a2;  sL = sL + l2;  sQ = sQ + q2
 *   m > m2:       r = exp(m2 - m);  sA = sA + a2 * r;  sL = sL + l2 * r;  sQ = sQ + q2 * r
 *   otherwise:    r = exp(m - m2);  sA = sA * r + a2;  sL = sL * r + l2;  sQ = sQ * r + q2;  m = m2
 * out [4][N]:
 *   row 0  p_lt = sL / sA     the weighted share of replicates below the observation
 *   row 1  p_eq = sQ / sA     ... equal to it (discrete data)
 *   row 2  pit  = p_lt + 0.5 * p_eq
 *   row 3  k                  the datum's Pareto k (+inf where nothing was smoothed, NaN from a degenerate
 *                             fit); a PIT whose k is above min(1 - 1 / log10(n), 0.7) is not to be trusted
 * A datum with a NaN or infinite term has all four NaN. The bits depend on (S, C), the trace, seed and
 * chain_lo only; they do not depend on scratch_bytes.
 *
 * No sharding. The weights of a sample are normalised over ALL chains of the call (the tail, its fit
 * and the maximum are per datum over the pooled samples), so a call over a shard of the chains is another
 * estimator: unlike exmc_hip_ppc there is no sharding property, and chain_lo only seeds the generators.
 *
 * Memory. exmc_hip_loo_pit forms the pointwise matrix of a block of datums at a time, as many datums as
 * fit scratch_bytes (0: the default below) and one at the least, as exmc_hip_psis_stats does. BESIDE that
 * budget it keeps the sorted tails of all N datums for the second pass: keys, sample indices and smoothed
 * values [N][P] with P the power of two at or above M = ceil(min(n / 5, 3 sqrt n)), and six doubles per
 * datum -- 20 P bytes per datum (logistic, 1000 datums at 8192 x 1000: P = 16384, 164 MB) -- and the
 * block states [B][N][4]. All of it is allocated for the call and freed before it returns.
 *
 * EXMC_MODEL_STD_NORMAL (no data) and plug-in libraries of generated models answer
 * EXMC_ERR_UNSUPPORTED. Errors: EXMC_ERR_BADARG for a null trace or output, d != the model's dimension,
 * n_draws < 1, n_chains < 1, chain_lo < 0, resume != 0, n < 2, n > 2^31 - 1, or a handle with a stream run
 * in flight.
 *
 * Handle state (exmc_hip.h "Handle state"): exmc_hip_loo_pit reads none and changes none. It runs on the
 * handle's stream and returns when the results are written; exmc_hip_last_kernel_ms times its kernels. */
#ifndef EXMC_HIP_LOO_PIT_H
#define EXMC_HIP_LOO_PIT_H

#include <stddef.h>

#include "exmc_hip_predictive.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EXMC_LOO_PIT_BLOCK 64    /* chains per block of the per-datum states */
#define EXMC_LOO_PIT_ROWS 4      /* p_lt, p_eq, pit, k */
#define EXMC_LOO_PIT_DEFAULT_SCRATCH (8ull << 30)   /* that of exmc_hip_psis_stats */

/* draws_dev [S][d][C] -> out_dev [4][N] on the device, written whole. N = exmc_hip_model_n_data. */
int exmc_hip_loo_pit(exmc_hip_model* m, exmc_hip_predictive_opts opts, const double* draws_dev, int n_draws, int d,
                     int n_chains, size_t scratch_bytes, double* out_dev);

/* the same from a host trace in the reference's layout [C][S][d] into host out [4][N] */
int exmc_hip_loo_pit_host(exmc_hip_model* m, exmc_hip_predictive_opts opts, const double* draws_host, int n_draws,
                          int d, int n_chains, size_t scratch_bytes, double* out_host);

/* model-free: the same contract and the same bits from device matrices ll_dev [S][N][C] (the terms),
 * yrep_dev [S][N][C] (the replicates) and y_dev [N] (the observations) on `device`, into out_dev [4][N]
 * (null stream; returns when written). For models whose terms and replicates the caller made. The tails
 * of all N datums are kept as above. A plug-in library answers EXMC_ERR_UNSUPPORTED: libexmc_hip.so
 * serves this call. */
int exmc_hip_loo_pit_from_ll(int device, const double* ll_dev, const double* yrep_dev, const double* y_dev,
                             int n_draws, int n_data, int n_chains, double* out_dev);

#ifdef __cplusplus
}
#endif

#endif
