// exmc_advi.hpp — Exmc.ADVI (lib/exmc/advi.ex) with one mean-field fit per lane group: fit c is
// ADVI.fit(ir, seed: base + 7919 (chain_lo + c)). The start, the whole stochastic-gradient loop with its
// convergence test, and the draws happen in one launch.
//
// Restated semantics (DESIGN.md "ADVI"):
//   start      rng = seed_s(:exsss, seed), mu = 0.0, log_sigma = -1.0 in every dimension (advi.ex:29-32)
//   iteration  i = 1 .. max_iters (:62-99): sigma = exp(log_sigma); for each of num_mc_samples samples
//              d variates of normal_s from the RUNNING generator, variate r to flat entry r,
//              z = mu + sigma eps, (logp, g) = logp_grad(z), entropy = sum(log_sigma) + 0.5 d (1 + log 2 pi),
//              elbo_s = isfinite(logp) ? logp + entropy : -1.0e10 (:128), grad_mu_s = g,
//              grad_ls_s = (g sigma) eps + 1.0 (:132-136); elbo = (0 + elbo_1 + ...) / n, the gradients
//              summed in sample order from the first and divided by n * 1.0 (:141-153);
//              mu += lr grad_mu, log_sigma += lr grad_ls (:70-73)
//   test       once the history holds window_size values, h = window_size div 2, recent = the sum of the h
//              newest ELBOs, newest first, old = the sum of the next h; converged when
//              |recent/h - old/h| / (|old/h| + 1e-8) < tol (:77-86). A converged fit stops after this
//              iteration's update with num_iters = i; otherwise num_iters = max_iters
//   draws      from the generator AS THE LOOP LEFT IT: draw n, flat entry r = mu + exp(log_sigma) normal_s
//              (:158-173)
// Every product and sum rounds separately (-ffp-contract=off); every sum over the dimensions is
// group_sum_slots with init0 = 0.0, the summation contract of exmc_device.hpp. A non-finite gradient
// is not repaired: it flows into mu and log_sigma as in the reference.
//
// Stated deviations: max_iters >= 1, num_draws >= 1, num_mc_samples >= 1 and window_size >= 2 (the
// host refuses anything else: Elixir's 1..0 counts down and a half window of 0 divides by zero); the
// results are in the unconstrained kernel space in kernel order; history entries at and after
// num_iters are NaN; where sum(log_sigma) is not finite the reference raises (:126 adds a float to
// an atom) and here the value flows on -- a finite logp then gives a non-finite ELBO, which never
// passes the test.
//
// One wavefront per workgroup, the launch shape of init_chains_kernel. A converged fit is
// predicated off -- its generator does not advance, its lanes stay in the DPP stages -- and the
// wavefront leaves the loop when none of its fits is active (wave-uniform, no bit changes).
//
// The ELBO window lives in the history buffer [max_iters][C] in device memory (the caller's, or
// scratch of the call): every lane of a group stores the group's ELBO to the same word and reads back
// what it stored, so program order suffices. The two half sums are sequential, newest first; with
// G >= 2 even lanes form `recent` and odd lanes `old` with the same instructions, and one exchange
// gives both to every lane. No private-memory array has a run-time index; window_size is bounded by
// int only (a window longer than max_iters never fills).
#pragma once

#include "exmc_kernels.hpp"   // attach_scratch, the launch shape of init_chains_kernel

namespace exmc {

struct AdviParams {
  int n_chains;
  int chain_lo;
  uint64_t base_seed;
  int max_iters, num_draws, num_mc_samples, window_size;
  double learning_rate, convergence_tol;
  double entropy_const;   // 0.5 * d * (1.0 + log(2.0 * pi)), libm on the host (advi.ex:126)
  double* history;        // [max_iters][C], never null: the window is read from it
  int fill_history;       // the caller wants it: entries at and after num_iters are set to NaN
  double* draws;          // [S][D][C] or null
  double* mu;             // [D][C] or null
  double* log_sigma;      // [D][C] or null
  int32_t* num_iters;     // [C] or null
  int32_t* converged;     // [C] or null
  RngArgs rng;
  FlatOrder flat;
};

template <class M, int G>
__global__ void __launch_bounds__(64) advi_kernel(AdviParams P, typename M::Consts mc) {
  constexpr int D = M::D, DPL = M::DPL;
  extern __shared__ double xlds[];
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int l = threadIdx.x & (G - 1);
  const int C = P.n_chains;
  const bool has_chain = (tid / G) < C;
  const int chain = has_chain ? (tid / G) : (C - 1);
  if (!M::kCoop && !has_chain) return;
  typename M::Lane ln;
  M::load(mc, l, ln);
  attach_scratch<M>(ln, xlds);
  const ZigTables zt{P.rng.ki, P.rng.wi, P.rng.fi};
  const uint64_t seed = P.base_seed + 7919ULL * (uint64_t)(P.chain_lo + chain);

  bool valid[DPL];
  int rank[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    const int i = l + k * G;
    valid[k] = i < D;
    rank[k] = valid[k] ? (P.flat.rank ? P.flat.rank[i] : i) : D;
  }
  auto dsum = [&](const double (&t)[DPL]) { return group_sum_slots<G, DPL, D>(t, valid, l, 0.0); };

  // advi.ex:29-32
  Rng rng;
  rng_seed(rng, seed);
  double mu[DPL], ls[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    mu[k] = 0.0;
    ls[k] = -1.0;
  }

  const int n_mc = P.num_mc_samples, window = P.window_size, h = window / 2;
  const double lr = P.learning_rate, dn = (double)n_mc, dh = (double)h;
  double* const hist = P.history + chain;   // entry i of this fit: hist[(size_t)i * C]
  bool active = true, conv = false;
  int n_iters = P.max_iters;

  for (int it = 1; it <= P.max_iters; it++) {
    if (!__any(active)) break;   // every fit of the wavefront has converged
    double sigma[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) sigma[k] = exmc_exp(ls[k]);   // :63
    const double entropy = dsum(ls) + P.entropy_const;          // :126, the same for every sample

    double elbo_sum = 0.0, gm[DPL], gl[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) gm[k] = gl[k] = 0.0;
    for (int s = 0; s < n_mc; s++) {
      double eps[DPL], z[DPL], g[DPL];
#pragma unroll
      for (int k = 0; k < DPL; k++) eps[k] = g[k] = 0.0;
      if (active) {   // the generator of a converged fit stays where its halt left it
        for (int r = 0; r < D; r++) {
          const double v = rng_normal(rng, zt, P.rng.nor_r);
#pragma unroll
          for (int k = 0; k < DPL; k++)
            if (rank[k] == r) eps[k] = v;
        }
      }
#pragma unroll
      for (int k = 0; k < DPL; k++) z[k] = mu[k] + sigma[k] * eps[k];   // :122
      const double logp = M::logp_grad(mc, ln, l, z, g);
      const double elbo_s = exmc_isfinite(logp) ? (logp + entropy) : -1.0e10;   // :128
      elbo_sum = elbo_sum + elbo_s;                                             // :141
#pragma unroll
      for (int k = 0; k < DPL; k++) {
        const double gls = (g[k] * sigma[k]) * eps[k] + 1.0;   // :132-136
        gm[k] = (s == 0) ? g[k] : (gm[k] + g[k]);              // Enum.reduce: the first is the start
        gl[k] = (s == 0) ? gls : (gl[k] + gls);
      }
    }
    const double elbo = elbo_sum / dn;
#pragma unroll
    for (int k = 0; k < DPL; k++) {   // :70-73
      const double m1 = mu[k] + lr * (gm[k] / dn);
      const double l1 = ls[k] + lr * (gl[k] / dn);
      mu[k] = active ? m1 : mu[k];
      ls[k] = active ? l1 : ls[k];
    }

    // :75-86. Every lane of the group stores the same ELBO to the same word and reads its own store back.
    if (active) hist[(size_t)(it - 1) * C] = elbo;
    const bool full = active && it >= window;
    double a = 0.0, b = 0.0;
    if (full) {
      const size_t top = (size_t)(it - 1) - (size_t)((G >= 2) ? (l & 1) * h : 0);   // this lane's half, newest
      for (int j = 0; j < h; j++) a = a + hist[(top - (size_t)j) * C];
      if (G == 1)
        for (int j = 0; j < h; j++) b = b + hist[(top - (size_t)(h + j)) * C];
    }
    const double recent = group_bcast_c<G, 0>(a);
    const double old = (G >= 2) ? group_bcast_c<G, (G >= 2 ? 1 : 0)>(a) : b;
    const double mr = recent / dh, mo = old / dh;
    const bool now = full && (fabs(mr - mo) / (fabs(mo) + 1.0e-8) < P.convergence_tol);
    n_iters = now ? it : n_iters;
    conv = conv || now;
    active = active && !now;
  }

  if (!has_chain) return;
  if (l == 0) {
    if (P.num_iters) P.num_iters[chain] = n_iters;
    if (P.converged) P.converged[chain] = conv ? 1 : 0;
    if (P.fill_history) {
      const double nan = exmc_from_bits(EXMC_NAN_BITS);
      for (int i = n_iters; i < P.max_iters; i++) hist[(size_t)i * C] = nan;
    }
  }
  double sigma[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    sigma[k] = exmc_exp(ls[k]);   // :159
    if (valid[k]) {
      const size_t o = (size_t)(l + k * G) * C + chain;
      if (P.mu) P.mu[o] = mu[k];
      if (P.log_sigma) P.log_sigma[o] = ls[k];
    }
  }
  // draw_samples (:158-173), from the generator as the loop left it
  if (!P.draws) return;
  for (int n = 0; n < P.num_draws; n++) {
    double dr[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) dr[k] = 0.0;
    for (int r = 0; r < D; r++) {
      const double v = rng_normal(rng, zt, P.rng.nor_r);
#pragma unroll
      for (int k = 0; k < DPL; k++)
        if (rank[k] == r) dr[k] = mu[k] + sigma[k] * v;
    }
#pragma unroll
    for (int k = 0; k < DPL; k++)
      if (valid[k]) P.draws[((size_t)n * D + (size_t)(l + k * G)) * C + chain] = dr[k];
  }
}

}  // namespace exmc
