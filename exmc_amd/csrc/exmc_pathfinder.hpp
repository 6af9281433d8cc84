// exmc_pathfinder.hpp — Exmc.Pathfinder (lib/exmc/pathfinder.ex) with one L-BFGS path per lane
// group: path c is Pathfinder.fit(ir, seed: base + 7919 (chain_lo + c)). The start, the whole path,
// the ELBO of every path point, the running best approximation and the draws happen in one launch;
// no path is stored, since the ELBO of a point is formed when the point is visited.
//
// Restated semantics (DESIGN.md "Pathfinder"):
//   start      q0[r] = 0.1 normal_s, variate r to entry r of the flat vector (pathfinder.ex:59-63)
//   step i     direction = g without history, else the two-loop recursion (:117-154);
//              q_new = q + 0.01 direction; a non-finite logp halts the path, the failing point is
//              no path point (:85-86); s = q_new - q, y = g_new - g, the pair is pushed in front
//              of the history (at most history_size pairs) when dot(y, s) > 1e-10 (:88-99)
//   point      sigma = 1 / sqrt(|g| + 1e-6), elbo = logp + (0.5 d (1 + log 2 pi) + sum log sigma)
//              (:156-171); the best approximation is the FIRST point of the largest ELBO (:43)
//   draws      from the INITIAL generator again: draw n, flat entry r = mu + sigma normal_s (:173-190)
// Every product and sum rounds separately (-ffp-contract=off); every sum over the dimensions is
// group_sum_slots with init0 = 0.0, the summation contract of exmc_device.hpp. rho_j = 1 / dot(y_j, s_j)
// and dot(s_0, y_0) are kept from the push: the same products in the same sum order, the same bits.
//
// Stated deviations: a point whose ELBO is not finite is never selected (the reference raises for
// the whole fit); a path without a finite ELBO reports status 1 and NaN results; history_size is at
// most kPfHistory (the reference's default); a pair whose dot(y, s) is NaN is not pushed (the
// reference raises).
//
// One wavefront per workgroup, the launch shape of init_chains_kernel. The trip count is the
// launch's max_iters: a halted path is predicated off and its lanes keep taking part in the sums.
// The history lives in registers at compile-time indices and is shifted on a push.
#pragma once

#include "exmc_kernels.hpp"   // attach_scratch, the launch shape of init_chains_kernel

namespace exmc {

constexpr int kPfHistory = 6;

struct PathfinderParams {
  int n_chains;
  int chain_lo;
  uint64_t base_seed;
  int max_iters, history_size, num_draws;
  double entropy_const;   // 0.5 * d * (1.0 + log(2.0 * pi)), libm on the host (pathfinder.ex:165)
  double* draws;          // [S][D][C] or null
  double* mu;             // [D][C] or null
  double* sigma;          // [D][C] or null
  double* elbo;           // [C] or null
  int32_t* num_iters;     // [C] or null: the path length, 1 + accepted steps
  int32_t* best_index;    // [C] or null: the path point of the best approximation (-1: none)
  int32_t* status;        // [C] or null: 1 when no path point has a finite ELBO
  RngArgs rng;
  FlatOrder flat;
};

template <class M, int G>
__global__ void __launch_bounds__(64) pathfinder_kernel(PathfinderParams P, typename M::Consts mc) {
  constexpr int D = M::D, DPL = M::DPL, H = kPfHistory;
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
  const int hs = P.history_size;

  bool valid[DPL];
  int rank[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    const int i = l + k * G;
    valid[k] = i < D;
    rank[k] = valid[k] ? (P.flat.rank ? P.flat.rank[i] : i) : D;
  }
  auto dsum = [&](const double (&t)[DPL]) { return group_sum_slots<G, DPL, D>(t, valid, l, 0.0); };

  // pathfinder.ex:59-66: the start and its value and gradient
  double q[DPL], g[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) q[k] = g[k] = 0.0;
  {
    Rng rng;
    rng_seed(rng, seed);
    for (int r = 0; r < D; r++) {
      const double z = rng_normal(rng, zt, P.rng.nor_r);
#pragma unroll
      for (int k = 0; k < DPL; k++)
        if (rank[k] == r) q[k] = z * 0.1;
    }
  }
  const double logp0 = M::logp_grad(mc, ln, l, q, g);

  // the running best approximation (fit_approximations + Enum.max_by, :156-171 and :43)
  double best_elbo = 0.0, best_mu[DPL], best_sig[DPL];
  int best_idx = -1;
#pragma unroll
  for (int k = 0; k < DPL; k++) best_mu[k] = best_sig[k] = 0.0;
  auto visit = [&](bool on, double lp, const double (&qq)[DPL], const double (&gg)[DPL], int idx) {
    double sig[DPL], ls[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      sig[k] = 1.0 / __dsqrt_rn(fabs(gg[k]) + 1.0e-6);
      ls[k] = exmc_log(sig[k]);
    }
    const double elbo = lp + (P.entropy_const + dsum(ls));
    const bool take = on && exmc_isfinite(elbo) && (best_idx < 0 || elbo > best_elbo);
    best_elbo = take ? elbo : best_elbo;
    best_idx = take ? idx : best_idx;
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      best_mu[k] = take ? qq[k] : best_mu[k];
      best_sig[k] = take ? sig[k] : best_sig[k];
    }
  };
  visit(true, logp0, q, g, 0);

  // the history, newest pair first (s_list / y_list, :92-99)
  double hs_s[H][DPL], hs_y[H][DPL], rho[H];
#pragma unroll
  for (int j = 0; j < H; j++) {
    rho[j] = 0.0;
#pragma unroll
    for (int k = 0; k < DPL; k++) hs_s[j][k] = hs_y[j][k] = 0.0;
  }
  double ys0 = 0.0;   // dot(y_0, s_0) of the newest pair
  int n_hist = 0, path_len = 1;
  bool active = true;

  for (int it = 0; it < P.max_iters; it++) {
    // lbfgs_direction (:117-154)
    double dir[DPL], t[DPL], alpha[H];
#pragma unroll
    for (int k = 0; k < DPL; k++) dir[k] = g[k];
#pragma unroll
    for (int j = 0; j < H; j++) {   // newest to oldest
      alpha[j] = 0.0;
      if (j < hs) {
#pragma unroll
        for (int k = 0; k < DPL; k++) t[k] = hs_s[j][k] * dir[k];
        const double a = rho[j] * dsum(t);
        const bool use = j < n_hist;
        alpha[j] = a;
#pragma unroll
        for (int k = 0; k < DPL; k++) dir[k] = use ? (dir[k] - a * hs_y[j][k]) : dir[k];
      }
    }
#pragma unroll
    for (int k = 0; k < DPL; k++) t[k] = hs_y[0][k] * hs_y[0][k];
    const double yy = dsum(t);
    const double gamma = ys0 / ((yy > 1.0e-10) ? yy : 1.0e-10);
#pragma unroll
    for (int k = 0; k < DPL; k++) dir[k] = (n_hist > 0) ? (gamma * dir[k]) : dir[k];
#pragma unroll
    for (int j = H - 1; j >= 0; j--) {   // oldest to newest
      if (j < hs) {
#pragma unroll
        for (int k = 0; k < DPL; k++) t[k] = hs_y[j][k] * dir[k];
        const double beta = rho[j] * dsum(t);
        const bool use = j < n_hist;
        const double ab = alpha[j] - beta;
#pragma unroll
        for (int k = 0; k < DPL; k++) dir[k] = use ? (dir[k] + ab * hs_s[j][k]) : dir[k];
      }
    }

    // :80-83 (a halted path stays at its last point)
    double qn[DPL], gn[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      qn[k] = active ? (q[k] + 0.01 * dir[k]) : q[k];
      gn[k] = 0.0;
    }
    const double lpn = M::logp_grad(mc, ln, l, qn, gn);
    const bool ok = active && exmc_isfinite(lpn);
    active = ok;

    // :88-99
    double sv[DPL], yv[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      sv[k] = qn[k] - q[k];
      yv[k] = gn[k] - g[k];
      t[k] = yv[k] * sv[k];
    }
    const double ys = dsum(t);
    const bool push = ok && (ys > 1.0e-10);
#pragma unroll
    for (int j = H - 1; j >= 1; j--) {
      rho[j] = push ? rho[j - 1] : rho[j];
#pragma unroll
      for (int k = 0; k < DPL; k++) {
        hs_s[j][k] = push ? hs_s[j - 1][k] : hs_s[j][k];
        hs_y[j][k] = push ? hs_y[j - 1][k] : hs_y[j][k];
      }
    }
    rho[0] = push ? (1.0 / ys) : rho[0];
    ys0 = push ? ys : ys0;
    n_hist = push ? ((n_hist + 1 < hs) ? n_hist + 1 : hs) : n_hist;
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      hs_s[0][k] = push ? sv[k] : hs_s[0][k];
      hs_y[0][k] = push ? yv[k] : hs_y[0][k];
      q[k] = ok ? qn[k] : q[k];
      g[k] = ok ? gn[k] : g[k];
    }
    visit(ok, lpn, qn, gn, path_len);
    path_len = ok ? path_len + 1 : path_len;
  }

  if (!has_chain) return;
  const bool none = best_idx < 0;
  const double nan = exmc_from_bits(EXMC_NAN_BITS);
  if (l == 0) {
    if (P.elbo) P.elbo[chain] = none ? nan : best_elbo;
    if (P.num_iters) P.num_iters[chain] = path_len;
    if (P.best_index) P.best_index[chain] = best_idx;
    if (P.status) P.status[chain] = none ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    best_mu[k] = none ? nan : best_mu[k];
    best_sig[k] = none ? nan : best_sig[k];
    if (valid[k]) {
      const size_t o = (size_t)(l + k * G) * C + chain;
      if (P.mu) P.mu[o] = best_mu[k];
      if (P.sigma) P.sigma[o] = best_sig[k];
    }
  }
  // draw_from_normal (:173-190) from the seeded generator, not from the one the start left behind
  if (!P.draws) return;
  Rng rng;
  rng_seed(rng, seed);
  for (int n = 0; n < P.num_draws; n++) {
    double dr[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) dr[k] = 0.0;
    for (int r = 0; r < D; r++) {
      const double z = rng_normal(rng, zt, P.rng.nor_r);
#pragma unroll
      for (int k = 0; k < DPL; k++)
        if (rank[k] == r) dr[k] = best_mu[k] + best_sig[k] * z;
    }
#pragma unroll
    for (int k = 0; k < DPL; k++)
      if (valid[k]) P.draws[((size_t)n * D + (size_t)(l + k * G)) * C + chain] = dr[k];
  }
}

}  // namespace exmc
