/* exmc_hip_psis.h -- the PSIS-LOO entry points of libexmc_hip.so, part of the model comparison
 * interface: include exmc_hip_compare.h, which ends by including this file. Plain C. */
#ifndef EXMC_HIP_PSIS_H
#define EXMC_HIP_PSIS_H

#include <stddef.h>

#include "exmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- PSIS-LOO: Pareto-smoothed importance-sampling LOO with the Pareto k diagnostic ----
 * DESIGN.md "PSIS-LOO" states the estimator (Vehtari, Simpson, Gelman, Yao, Gabry; the generalised-
 * Pareto fit of Zhang & Stephens), r_eff = 1. out [3][N]: rows elpd_loo_i, p_loo_i = lppd_i -
 * elpd_loo_i (lppd_i as exmc_hip_ic_stats forms it) and the Pareto k of the datum's importance
 * ratios (+inf where the tail has at most 4 samples and nothing is smoothed). A datum with a NaN or
 * infinite term has all three NaN. The bits depend on (S, C) and the terms only. At most
 * 2^31 - 1 pooled samples (EXMC_ERR_BADARG above). Errors and handle state are those of
 * exmc_hip_ic_stats above; kinds without datums and plug-in libraries answer EXMC_ERR_UNSUPPORTED.
 *
 * exmc_hip_psis_stats forms the pointwise matrix of a block of datums at a time in scratch memory
 * and walks the model's datums in such blocks: as many datums as fit scratch_bytes (0: the default
 * below), one at the least. The result per datum does not depend on the blocking. Scratch (that
 * matrix, the sorted tails, chunk states) is allocated for the call and freed before it returns. */
#define EXMC_PSIS_DEFAULT_SCRATCH (8ull << 30)   /* 8 GiB: profiles/psis/README.md */

int exmc_hip_psis_stats(exmc_hip_model* m, const double* draws_dev, int n_draws, int d,
                        int n_chains, size_t scratch_bytes, double* out_dev);

/* the same from a host trace in the reference's layout [C][S][d] into host out [3][N] */
int exmc_hip_psis_stats_host(exmc_hip_model* m, const double* draws_host, int n_draws, int d,
                             int n_chains, size_t scratch_bytes, double* out_host);

/* model-free: of a device matrix ll_dev [S][N][C] on `device` (null stream; returns when written) */
int exmc_hip_psis_stats_from_ll(int device, const double* ll_dev, int n_draws, int n_data,
                                int n_chains, double* out_dev);

#ifdef __cplusplus
}
#endif

#endif
