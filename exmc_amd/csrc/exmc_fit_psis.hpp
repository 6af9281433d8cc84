// exmc_fit_psis.hpp — the log importance ratios log p(x) - log q(x) of the draws of a batch of
// variational fits (exmc_hip_pathfinder, exmc_hip_advi): fit c is the diagonal normal (mu, sigma) of
// lane group c, its S draws the column c of draws[S][D][C], exactly what the two fit calls write.
// DESIGN.md "Importance diagnostics of the fits" is the contract, include/exmc_hip_fit_psis.h the C ABI.
//
// Per draw of a fit, over the fit's dimensions r (slot k of lane l holds dimension l + k G):
//   logp   = M::logp_grad at the draw, the gradient discarded
//   z_r    = (x_r - mu_r) / sigma_r                        IEEE division
//   t_r    = 0.5 * (z_r * z_r) + ls_r
//   logq   = -(group_sum_slots(t, init0 = 0.0)) - c        c = 0.5 d log(2 pi), libm on the host
//   lr     = logp - logq
// With EXMC_FIT_SIGMA the scale array is sigma and ls = exmc_log(sigma) (Pathfinder reports sigma);
// with EXMC_FIT_LOG_SIGMA it is log_sigma, ls the array and sigma = exmc_exp(log_sigma), the call
// advi_kernel makes for its draws. Every product and sum rounds separately (-ffp-contract=off).
//
// lr = -inf (weight zero) where logp is NaN or -inf, or where the draw or the fit's mu or scale array
// holds a non-finite value; logp = +inf otherwise gives lr = NaN.
//
// One wavefront per workgroup, the launch shape of pathfinder_kernel; lane groups without a fit
// shadow the last fit in the co-operative kinds and store nothing.
#pragma once

#include "exmc_kernels.hpp"   // attach_scratch, the launch shape of init_chains_kernel

namespace exmc {

constexpr int kFitSigma = 0;      // EXMC_FIT_SIGMA
constexpr int kFitLogSigma = 1;   // EXMC_FIT_LOG_SIGMA

struct FitLogRatioParams {
  const double* draws;   // [S][D][C]
  const double* mu;      // [D][C]
  const double* scale;   // [D][C]: sigma or log_sigma
  int scale_kind;
  int n_draws, n_fits;
  double log_norm;       // 0.5 * d * log(2.0 * pi), libm on the host
  double* lr;            // [S][C]
  double* logp;          // [S][C] or null
};

template <class M, int G>
__global__ void __launch_bounds__(64) fit_log_ratio_kernel(FitLogRatioParams P, typename M::Consts mc) {
  constexpr int D = M::D, DPL = M::DPL;
  extern __shared__ double xlds[];
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int l = threadIdx.x & (G - 1);
  const int C = P.n_fits;
  const bool has_chain = (tid / G) < C;
  const int chain = has_chain ? (tid / G) : (C - 1);
  if (!M::kCoop && !has_chain) return;
  typename M::Lane ln;
  M::load(mc, l, ln);
  attach_scratch<M>(ln, xlds);

  bool valid[DPL];
  double mu[DPL], sig[DPL], ls[DPL], flag[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    const int i = l + k * G;
    valid[k] = i < D;
    const size_t o = (size_t)i * C + chain;
    mu[k] = valid[k] ? P.mu[o] : 0.0;
    const double sc = valid[k] ? P.scale[o] : (P.scale_kind == kFitLogSigma ? 0.0 : 1.0);
    sig[k] = (P.scale_kind == kFitLogSigma) ? exmc_exp(sc) : sc;
    ls[k] = (P.scale_kind == kFitLogSigma) ? sc : exmc_log(sc);
    flag[k] = (exmc_isfinite(mu[k]) && exmc_isfinite(sc)) ? 0.0 : 1.0;
  }
  auto dsum = [&](const double (&t)[DPL]) { return group_sum_slots<G, DPL, D>(t, valid, l, 0.0); };
  const bool fit_bad = dsum(flag) > 0.0;
  const double ninf = -__builtin_inf();

  for (int s = 0; s < P.n_draws; s++) {
    double x[DPL], g[DPL], t[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      x[k] = valid[k] ? P.draws[((size_t)s * D + (size_t)(l + k * G)) * C + chain] : 0.0;
      g[k] = 0.0;
      flag[k] = exmc_isfinite(x[k]) ? 0.0 : 1.0;
    }
    const double logp = M::logp_grad(mc, ln, l, x, g);
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      const double z = (x[k] - mu[k]) / sig[k];
      t[k] = 0.5 * (z * z) + ls[k];
    }
    const double logq = -dsum(t) - P.log_norm;
    const bool zero = fit_bad || (dsum(flag) > 0.0) || !(logp == logp) || logp == ninf;
    const double lr = zero ? ninf : (logp == __builtin_inf() ? exmc_from_bits(EXMC_NAN_BITS) : logp - logq);
    if (has_chain && l == 0) {
      P.lr[(size_t)s * C + chain] = lr;
      if (P.logp) P.logp[(size_t)s * C + chain] = logp;
    }
  }
}

}  // namespace exmc
