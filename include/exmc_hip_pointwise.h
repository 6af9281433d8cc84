/* exmc_hip_pointwise.h -- per-datum log-likelihoods of a block of datums, part of the model comparison
 * interface: include exmc_hip_compare.h, which ends by including this file. Plain C.
 *
 * The entry point that lets a GENERATED model take part in model comparison (DESIGN.md "Model
 * comparison", per-datum terms of generated models). A plug-in library carries no reduction kernels;
 * a model generated with per-datum terms (exmc_amd/codegen.py generate(pointwise=True)) carries one
 * kernel that evaluates its datum terms over a trace. The caller walks the datums in blocks: this call
 * on the plug-in's handle into a scratch matrix, then libexmc_hip.so's exmc_hip_ic_stats_from_ll /
 * exmc_hip_psis_stats_from_ll on that block (exmc_amd/model_comparison.py does so). */
#ifndef EXMC_HIP_POINTWISE_H
#define EXMC_HIP_POINTWISE_H

#include "exmc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ll_dev [S][nb][C]: the terms of the datums i0 .. i0 + nb - 1 (in the handle's datum order: radon's
 * county-sorted) at every sample of the device trace draws_dev [S][d][C]. The columns are those of
 * exmc_hip_pointwise_loglik, bit for bit. Runs on the handle's stream and returns when the matrix is
 * written; reads the model's data and nothing else of the handle (exmc_hip_compare.h, "Handle state").
 * Errors: those of exmc_hip_ic_stats, and EXMC_ERR_BADARG for a range outside [0, N) or nb < 1.
 * libexmc_hip.so serves the built-in kinds; a plug-in generated with per-datum terms its model; a
 * plug-in generated without them answers EXMC_ERR_UNSUPPORTED. */
int exmc_hip_pointwise_loglik_range(exmc_hip_model* m, const double* draws_dev, int n_draws, int d,
                                    int n_chains, int i0, int nb, double* ll_dev);

#ifdef __cplusplus
}
#endif

#endif
