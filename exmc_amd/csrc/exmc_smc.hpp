// exmc_smc.hpp — Exmc.SMC (lib/exmc/smc.ex), the tempered sequential Monte Carlo sampler, with one
// particle per lane group. Run r of a call has N particles; particle j of run r is "chain" c = r N + j
// of the launches, C = n_runs N. DESIGN.md "SMC" is the contract, include/exmc_hip_smc.h the C ABI,
// tests/smc_statement.py the statement.
//
// Restated semantics:
//   init       d variates of normal_s per particle, variate r to flat entry r, each times 0.5 (smc.ex:46-56);
//              lp = logp(q), -1.0e10 where it is not finite (:32-36)
//   stage      new_beta = min(find_next_beta, 1.0) (:103-104); find_next_beta is the bisection of :157-178:
//              mid = (lo + hi) / 2 from lo = beta, hi = 1.0; x_j = (mid - beta) lp_j, w_j = exp(x_j - max x),
//              nw = w / sum w, ess = 1.0 / sum nw^2; mid when |ess - threshold| < 1.0, else hi = mid (ess
//              below) or lo = mid; after the 51st evaluation (lo + hi) / 2. The stage's weights and ESS
//              (:107-117) the same way at delta_beta = new_beta - beta
//   resample   when ess < threshold (:119-124, :180-195): u the next uniform_s of the RUN generator,
//              pos_i = u / N + i / N, idx_i the first k with cum_k >= pos_i or N - 1; cum the cumulative sum
//              of nw in blocks of kRatioScan from 0.0 with the bases left to right (exmc_psis_ratio.hpp; for
//              N <= 4096 the reference's Enum.scan); q and lp gathered into second buffers
//   scale      per dimension after the resampling (:197-207): mean = sum / N, var = sum (v - mean)^2 /
//              max(N - 1, 1), scale = sqrt(max(var, 1.0e-10)) * 2.38 / sqrt(d), left to right
//   mutate     num_mh_steps times per particle (:209-247): d variates of normal_s in the flat order, each
//              times the scale of its dimension; lp' = logp(q + pert) with the -1.0e10 rule;
//              log_alpha = new_beta (lp' - lp); one uniform_s u; accepted when log(u) < log_alpha;
//              acceptance_rate = the count of acceptances / max(N num_mh_steps, 1) (:245)
// Every sum over the particles of a run is particle_sum: partial t of 256 adds the terms j = t (mod 256)
// in ascending j from 0.0; the partials are combined by the xor butterfly m = 1, 2, ..., 128, lane t
// taking part[t] + part[t ^ m] -- the shape of group_sum_slots. The maximum is exact in any order.
// Products and sums round separately (-ffp-contract=off).
//
// Stated deviations: the reference threads ONE generator through a run. Here seed_r = seed + 7919
// (run_lo + r); the run generator rng_seed(seed_r) serves only the uniform of each resampling; slot j has
// the particle generator rng_seed(seed_r ^ ((j + 1) << 32)), which stays with the slot through a
// resampling (copies diverge) and is kept in device memory between stages. At u = 0 (probability 2^-53)
// the reference raises; here the proposal is accepted. max_stages bounds the loop (status 1), since the
// bisection can return beta itself. A finished run is predicated off: its generators do not advance.
//
// smc_init_kernel and smc_mutate_kernel: one wavefront per workgroup, the launch shape of advi_kernel;
// lane groups past C shadow the last one in the co-operative kinds and store nothing. The model-free
// kernels (not in a plug-in): one workgroup of kSmcBlock lanes per run, or per (run, dimension).
// Vector stores only, one writer per output word, no floating-point atomics.
//
// The bridged mode (DESIGN.md "Bridged SMC", include/exmc_hip_smc_bridge.h, tests/smc_bridge_statement.py)
// tempers along log pi_beta = beta logp + (1 - beta) log q0 from a diagonal-normal base q0 and estimates the
// log evidence. Its kernels are siblings of the ones above over the same bodies (smc_init_body,
// smc_mutate_body, smc_weights_body with kBridge); what they add travels in SmcBridge.
#pragma once

#include "exmc_kernels.hpp"   // attach_scratch, the launch shape of init_chains_kernel
#ifndef EXMC_ONLY_CUSTOM
#include "exmc_psis_ratio.hpp"   // ratio_scan_kernel, ratio_bases, ratio_search
#endif

namespace exmc {

constexpr double kSmcNonFinite = -1.0e10;   // smc.ex:35, :223
constexpr int kSmcBlock = 256;              // lanes of a model-free workgroup: the partials of particle_sum
constexpr int kSmcLdsParticles = 4096;      // up to here a run's logps sit in LDS during the bisection
constexpr int kSmcBisect = 51;              // evaluations: iter = 0 .. 50 (:157)

// the state of the runs of a call, all in device memory (exmc_hip_smc_state)
struct SmcRuns {
  double* beta;               // [R]
  uint64_t* run_rng;          // [2][R]
  int32_t* active;            // [R]
  double* scale;              // [D][R]
  int32_t* accept;            // [C]
  double* betas;              // [max_stages][R]
  double* ess_history;        // [max_stages][R]
  double* acceptance_rates;   // [max_stages][R]
  int32_t* num_stages;        // [R]
  int32_t* status;            // [R]
  int32_t* active_count;      // [1]
};

struct SmcParams {
  int n_chains;      // C = n_runs * n_particles
  int n_particles, n_runs, run_lo;
  uint64_t base_seed;
  int num_mh_steps, max_stages;
  double* q;         // [D][C]
  double* logp;      // [C]
  uint64_t* words;   // [2][C]: the particle generators
  SmcRuns runs;
  RngArgs rng;
  FlatOrder flat;
};

// What the bridged mode adds to a call (DESIGN.md "Bridged SMC", include/exmc_hip_smc_bridge.h): the base
// q0 = N(mu, diag sigma^2) in kernel order, shared by the runs of the call, lb = log q0 of every particle and
// the evidence. The temper runs along log pi_beta = beta logp + (1 - beta) log q0.
struct SmcBridge {
  const double* mu;             // [D] or null: 0.0
  const double* sigma;          // [D] or null: 0.5
  double log_norm;              // 0.5 * d * log(2.0 * pi), libm on the host
  double* logb;                 // [C]
  double* log_evidence;         // [R]
  double* log_evidence_steps;   // [max_stages][R]
};

// log q0 in the EXMC_FIT_SIGMA form of exmc_fit_psis.hpp: z = (x - mu) / sigma, t = 0.5 * (z * z) + ls,
// -(group_sum_slots(t, 0.0)) - log_norm, ls = exmc_log(sigma)
template <int G, int DPL, int D>
__device__ __forceinline__ double smc_base_logq(const double (&x)[DPL], const double (&mu)[DPL],
                                                const double (&sg)[DPL], const double (&ls)[DPL],
                                                const bool (&valid)[DPL], int l, double log_norm) {
  double t[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    const double z = (x[k] - mu[k]) / sg[k];
    t[k] = 0.5 * (z * z) + ls[k];
  }
  return -group_sum_slots<G, DPL, D>(t, valid, l, 0.0) - log_norm;
}

__device__ __forceinline__ uint64_t smc_run_seed(const SmcParams& P, int run) {
  return P.base_seed + 7919ULL * (uint64_t)(P.run_lo + run);
}

// smc.ex:46-56 and :32-36; the first particle of a run also sets the run's state. kBridge: the start is the
// base, q = mu + sigma * v, and lb and the evidence are set beside lp and the histories.
template <class M, int G, bool kBridge>
__device__ __forceinline__ void smc_init_body(const SmcParams& P, const SmcBridge& B, const typename M::Consts& mc) {
  constexpr int D = M::D, DPL = M::DPL;
  extern __shared__ double xlds[];
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int l = threadIdx.x & (G - 1);
  const int C = P.n_chains, N = P.n_particles, R = P.n_runs;
  const bool has_chain = (tid / G) < C;
  const int chain = has_chain ? (tid / G) : (C - 1);
  if (!M::kCoop && !has_chain) return;
  typename M::Lane ln;
  M::load(mc, l, ln);
  attach_scratch<M>(ln, xlds);
  const ZigTables zt{P.rng.ki, P.rng.wi, P.rng.fi};
  const int run = chain / N, j = chain - run * N;
  const uint64_t seed_r = smc_run_seed(P, run);

  Rng rng;
  rng_seed(rng, seed_r ^ ((uint64_t)(j + 1) << 32));
  double q[DPL], g[DPL];
  bool valid[DPL];
  int rank[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    const int i = l + k * G;
    valid[k] = i < D;
    rank[k] = valid[k] ? (P.flat.rank ? P.flat.rank[i] : i) : D;
    q[k] = g[k] = 0.0;
  }
  double lb = 0.0;
  if constexpr (kBridge) {
    double mu[DPL], sg[DPL], ls[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      const int i = l + k * G;
      mu[k] = (valid[k] && B.mu) ? B.mu[i] : 0.0;
      sg[k] = valid[k] ? (B.sigma ? B.sigma[i] : 0.5) : 1.0;
      ls[k] = exmc_log(sg[k]);
    }
    for (int r = 0; r < D; r++) {
      const double v = rng_normal(rng, zt, P.rng.nor_r);
#pragma unroll
      for (int k = 0; k < DPL; k++)
        if (rank[k] == r) q[k] = mu[k] + sg[k] * v;
    }
    lb = smc_base_logq<G, DPL, D>(q, mu, sg, ls, valid, l, B.log_norm);
  } else {
    for (int r = 0; r < D; r++) {
      const double v = rng_normal(rng, zt, P.rng.nor_r) * 0.5;   // :50-51
#pragma unroll
      for (int k = 0; k < DPL; k++)
        if (rank[k] == r) q[k] = v;
    }
  }
  const double raw = M::logp_grad(mc, ln, l, q, g);
  const double lp = exmc_isfinite(raw) ? raw : kSmcNonFinite;   // :35
  if (!has_chain) return;
#pragma unroll
  for (int k = 0; k < DPL; k++)
    if (valid[k]) P.q[(size_t)(l + k * G) * C + chain] = q[k];
  if (l != 0) return;
  P.logp[chain] = lp;
  if constexpr (kBridge) B.logb[chain] = lb;
  P.words[chain] = rng.a;
  P.words[(size_t)C + chain] = rng.b;
  P.runs.accept[chain] = 0;
  if (j != 0) return;
  Rng rr;
  rng_seed(rr, seed_r);
  P.runs.run_rng[run] = rr.a;
  P.runs.run_rng[(size_t)R + run] = rr.b;
  P.runs.beta[run] = 0.0;   // :61
  P.runs.active[run] = 1;
  P.runs.num_stages[run] = 0;
  P.runs.status[run] = 1;
  if constexpr (kBridge) B.log_evidence[run] = 0.0;
  const double nan = exmc_from_bits(EXMC_NAN_BITS);
  for (int s = 0; s < P.max_stages; s++) {
    const size_t o = (size_t)s * R + run;
    P.runs.betas[o] = nan;
    P.runs.ess_history[o] = nan;
    P.runs.acceptance_rates[o] = nan;
    if constexpr (kBridge) B.log_evidence_steps[o] = nan;
  }
}

template <class M, int G>
__global__ void __launch_bounds__(64) smc_init_kernel(SmcParams P, typename M::Consts mc) {
  smc_init_body<M, G, false>(P, SmcBridge{}, mc);
}

template <class M, int G>
__global__ void __launch_bounds__(64) smc_bridge_init_kernel(SmcParams P, SmcBridge B, typename M::Consts mc) {
  smc_init_body<M, G, true>(P, B, mc);
}

// smc.ex:209-247 for one stage: the particle stays in registers across the num_mh_steps proposals. kBridge:
// lb stays there too, lb' is one group_sum_slots per proposal, and the proposal is judged on the bridge:
// log_alpha = (beta lp' + (1 - beta) lb') - (beta lp + (1 - beta) lb); a NaN log_alpha rejects.
template <class M, int G, bool kBridge>
__device__ __forceinline__ void smc_mutate_body(const SmcParams& P, const SmcBridge& B, const typename M::Consts& mc) {
  constexpr int D = M::D, DPL = M::DPL;
  extern __shared__ double xlds[];
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int l = threadIdx.x & (G - 1);
  const int C = P.n_chains, R = P.n_runs;
  const bool has_chain = (tid / G) < C;
  const int chain = has_chain ? (tid / G) : (C - 1);
  if (!M::kCoop && !has_chain) return;
  const int run = chain / P.n_particles;
  const bool active = P.runs.active[run] != 0;
  if (!__any(active)) return;   // every run of the wavefront has finished (wave-uniform)
  typename M::Lane ln;
  M::load(mc, l, ln);
  attach_scratch<M>(ln, xlds);
  const ZigTables zt{P.rng.ki, P.rng.wi, P.rng.fi};

  double q[DPL], sc[DPL];
  bool valid[DPL];
  int rank[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    const int i = l + k * G;
    valid[k] = i < D;
    rank[k] = valid[k] ? (P.flat.rank ? P.flat.rank[i] : i) : D;
    q[k] = valid[k] ? P.q[(size_t)i * C + chain] : 0.0;
    sc[k] = valid[k] ? P.runs.scale[(size_t)i * R + run] : 0.0;
  }
  double lp = P.logp[chain];
  Rng rng{P.words[chain], P.words[(size_t)C + chain]};
  const double beta = P.runs.beta[run];
  int accepted = 0;
  double lb = 0.0, omb = 0.0, mu[kBridge ? DPL : 1], sg[kBridge ? DPL : 1], ls[kBridge ? DPL : 1];
  if constexpr (kBridge) {
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      const int i = l + k * G;
      mu[k] = (valid[k] && B.mu) ? B.mu[i] : 0.0;
      sg[k] = valid[k] ? (B.sigma ? B.sigma[i] : 0.5) : 1.0;
      ls[k] = exmc_log(sg[k]);
    }
    lb = B.logb[chain];
    omb = 1.0 - beta;
  }

  for (int s = 0; s < P.num_mh_steps; s++) {
    double prop[DPL], g[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      prop[k] = q[k];
      g[k] = 0.0;
    }
    if (active) {   // the generator of a finished run stays where it is
      for (int r = 0; r < D; r++) {
        const double v = rng_normal(rng, zt, P.rng.nor_r);
#pragma unroll
        for (int k = 0; k < DPL; k++)
          if (rank[k] == r) prop[k] = q[k] + v * sc[k];   // :216-221
      }
    }
    const double raw = M::logp_grad(mc, ln, l, prop, g);
    const double lpp = exmc_isfinite(raw) ? raw : kSmcNonFinite;   // :223
    double log_alpha, lbp = 0.0;
    if constexpr (kBridge) {
      lbp = smc_base_logq<G, DPL, D>(prop, mu, sg, ls, valid, l, B.log_norm);
      const double tc = beta * lp + omb * lb, tp = beta * lpp + omb * lbp;
      log_alpha = tp - tc;
    } else {
      log_alpha = beta * (lpp - lp);                               // :227
    }
    bool take = false;
    if (active) {
      const double u = rng_uniform(rng);                           // :232
      take = (u == 0.0) || (exmc_log(u) < log_alpha);              // :234; u = 0: a stated deviation
      if constexpr (kBridge) take = take && (log_alpha == log_alpha);
    }
#pragma unroll
    for (int k = 0; k < DPL; k++) q[k] = take ? prop[k] : q[k];
    lp = take ? lpp : lp;
    if constexpr (kBridge) lb = take ? lbp : lb;
    accepted += take ? 1 : 0;
  }

  if (!has_chain || !active) return;
#pragma unroll
  for (int k = 0; k < DPL; k++)
    if (valid[k]) P.q[(size_t)(l + k * G) * C + chain] = q[k];
  if (l != 0) return;
  P.logp[chain] = lp;
  if constexpr (kBridge) B.logb[chain] = lb;
  P.words[chain] = rng.a;
  P.words[(size_t)C + chain] = rng.b;
  P.runs.accept[chain] = accepted;
}

template <class M, int G>
__global__ void __launch_bounds__(64) smc_mutate_kernel(SmcParams P, typename M::Consts mc) {
  smc_mutate_body<M, G, false>(P, SmcBridge{}, mc);
}

template <class M, int G>
__global__ void __launch_bounds__(64) smc_bridge_mutate_kernel(SmcParams P, SmcBridge B, typename M::Consts mc) {
  smc_mutate_body<M, G, true>(P, B, mc);
}

#ifndef EXMC_ONLY_CUSTOM   // a generated model's plug-in carries no model-free kernels

// ---- the reductions over the particles of a run: a workgroup of kSmcBlock lanes ------------------------
// `red` is kSmcBlock / 64 doubles of LDS; every lane returns the same value
template <class F>
__device__ __forceinline__ double particle_sum(int N, int tid, double* red, F&& term) {
  double v = 0.0;
  for (int j = tid; j < N; j += kSmcBlock) v = v + term(j);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m);
  const int w = tid >> 6;
  red[w] = v;
  __syncthreads();
  const double a = red[w] + red[w ^ 1];         // m = 64
  const double b = red[w ^ 2] + red[w ^ 3];     // the partner's value after m = 64
  __syncthreads();
  return a + b;                                 // m = 128
}

template <class F>
__device__ __forceinline__ double particle_max(int N, int tid, double* red, F&& term) {
  double v = -__builtin_inf();
  for (int j = tid; j < N; j += kSmcBlock) v = fmax(v, term(j));
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m));
  const int w = tid >> 6;
  red[w] = v;
  __syncthreads();
  const double r = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return r;
}

__device__ __forceinline__ int particle_count(const int32_t* v, int N, int tid, int* red) {
  int a = 0;
  for (int j = tid; j < N; j += kSmcBlock) a += v[j];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m);
  red[tid >> 6] = a;
  __syncthreads();
  const int r = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return r;
}

struct SmcStage {
  int n_particles, n_runs, stage, max_stages, num_mh_steps;
  double threshold;   // threshold_ratio * N (:59)
  int d;
  double sqrt_d;      // :math.sqrt(d) on the host (:205)
  SmcRuns runs;
};

// One workgroup: the acceptance rate of the stage before (:245), which runs go on, how many. A run goes
// on while beta < 1.0 (:78) and stage < max_stages.
__global__ __launch_bounds__(kSmcBlock) void smc_close_kernel(SmcStage S) {
  __shared__ int red[kSmcBlock / 64];
  const int tid = threadIdx.x, N = S.n_particles, R = S.n_runs;
  const long long den = (long long)N * S.num_mh_steps;
  int count = 0;
  for (int r = 0; r < R; r++) {
    const bool was = S.runs.active[r] != 0;
    const double beta = S.runs.beta[r];
    int total = 0;
    if (was && S.stage > 0) total = particle_count(S.runs.accept + (size_t)r * N, N, tid, red);
    else __syncthreads();   // the reads of active[r] before its store
    const bool now = was && beta < 1.0 && S.stage < S.max_stages;
    count += now ? 1 : 0;
    if (tid == 0 && was) {
      if (S.stage > 0)
        S.runs.acceptance_rates[(size_t)(S.stage - 1) * R + r] = (double)total / (double)(den > 1 ? den : 1);
      if (!(beta < 1.0)) S.runs.status[r] = 0;
      S.runs.active[r] = now ? 1 : 0;
    }
  }
  if (tid == 0) S.runs.active_count[0] = count;
}

// One workgroup per run: the bisection (:147-178), the stage's weights and ESS (:107-117). nw [R][N];
// resample [R] = 1 where ess < threshold (:120). kLds: the run's logps stay in LDS.
// kBridge (DESIGN.md "Bridged SMC" 3-5): the weights are of lr_j = lp_j - lb_j; the stage's first evaluation
// is at 1.0 - beta and ends the temper when its ESS is at or above the threshold, otherwise the bisection
// runs as it is; inc = mx + log(sw / N) is the stage's share of the log evidence; every stage resamples.
template <bool kLds, bool kBridge>
__device__ __forceinline__ void smc_weights_body(const SmcStage& S, const double* __restrict__ logp,
                                                 const SmcBridge& B, double* __restrict__ nw,
                                                 int32_t* __restrict__ resample) {
  extern __shared__ double lds_lp[];
  __shared__ double red[kSmcBlock / 64];
  const int tid = threadIdx.x, r = blockIdx.x, N = S.n_particles, R = S.n_runs;
  if (S.runs.active[r] == 0) {
    if (tid == 0) resample[r] = 0;
    return;
  }
  const double* lp = logp + (size_t)r * N;
  const double* lb = kBridge ? B.logb + (size_t)r * N : nullptr;
  if (kLds) {
    for (int j = tid; j < N; j += kSmcBlock) lds_lp[j] = kBridge ? lp[j] - lb[j] : lp[j];
    __syncthreads();
    lp = lds_lp;
  }
  auto at = [&](int j) { return (kBridge && !kLds) ? lp[j] - lb[j] : lp[j]; };
  const double beta = S.runs.beta[r], thr = S.threshold;
  double mx = 0.0, sw = 1.0;
  auto ess_at = [&](double delta) {
    mx = particle_max(N, tid, red, [&](int j) { return delta * at(j); });
    sw = particle_sum(N, tid, red, [&](int j) { return exmc_exp(delta * at(j) - mx); });
    const double s2 = particle_sum(N, tid, red, [&](int j) {
      const double w = exmc_exp(delta * at(j) - mx) / sw;
      return w * w;
    });
    return 1.0 / s2;
  };
  double lo = beta, hi = 1.0, next = 0.0;
  bool found = false;
  if constexpr (kBridge) {
    if (ess_at(1.0 - beta) >= thr) {   // block-uniform
      next = 1.0;
      found = true;
    }
  }
  for (int it = 0; it < kSmcBisect && !found; it++) {   // block-uniform: every lane holds the same sums
    const double mid = (lo + hi) / 2.0;
    const double ess = ess_at(mid - beta);
    if (fabs(ess - thr) < 1.0) {
      next = mid;
      found = true;
    } else if (ess < thr) {
      hi = mid;
    } else {
      lo = mid;
    }
  }
  if (!found) next = (lo + hi) / 2.0;    // :157
  const double new_beta = fmin(next, 1.0);   // :104
  const double ess = ess_at(new_beta - beta);
  const double delta = new_beta - beta;
  for (int j = tid; j < N; j += kSmcBlock) nw[(size_t)r * N + j] = exmc_exp(delta * at(j) - mx) / sw;
  if (tid == 0) {
    resample[r] = (kBridge || ess < thr) ? 1 : 0;
    S.runs.beta[r] = new_beta;
    S.runs.betas[(size_t)S.stage * R + r] = new_beta;
    S.runs.ess_history[(size_t)S.stage * R + r] = ess;
    S.runs.num_stages[r] = S.stage + 1;
    if constexpr (kBridge) {
      const double inc = mx + exmc_log(sw / (double)N);
      B.log_evidence_steps[(size_t)S.stage * R + r] = inc;
      B.log_evidence[r] = B.log_evidence[r] + inc;
    }
  }
}

template <bool kLds>
__global__ __launch_bounds__(kSmcBlock) void smc_weights_kernel(SmcStage S, const double* __restrict__ logp,
                                                               double* __restrict__ nw, int32_t* __restrict__ resample) {
  smc_weights_body<kLds, false>(S, logp, SmcBridge{}, nw, resample);
}

template <bool kLds>
__global__ __launch_bounds__(kSmcBlock) void smc_bridge_weights_kernel(SmcStage S, const double* __restrict__ logp,
                                                                      SmcBridge B, double* __restrict__ nw,
                                                                      int32_t* __restrict__ resample) {
  smc_weights_body<kLds, true>(S, logp, B, nw, resample);
}

// One workgroup per run (:180-195) over the cumulative sums of ratio_scan_kernel (linear, S = 1, Nb = R,
// C = N). base [R][n_blocks + 1] is scratch of the launch; idx [R][N], the identity where the run does
// not resample.
__global__ __launch_bounds__(kSmcBlock) void smc_resample_kernel(SmcStage S, const double* __restrict__ rcum,
                                                                const double* __restrict__ tot, double* __restrict__ base,
                                                                int n_blocks, const int32_t* __restrict__ resample,
                                                                int32_t* __restrict__ idx) {
  const int tid = threadIdx.x, r = blockIdx.x, N = S.n_particles, R = S.n_runs;
  int32_t* out = idx + (size_t)r * N;
  if (resample[r] == 0) {
    for (int j = tid; j < N; j += kSmcBlock) out[j] = j;
    return;
  }
  double* bs = base + (size_t)r * ((size_t)n_blocks + 1);
  if (tid == 0) ratio_bases(tot, bs, n_blocks, R, r);
  Rng rng{S.runs.run_rng[r], S.runs.run_rng[(size_t)R + r]};
  __syncthreads();   // the bases; every lane has read the generator
  const double u = rng_uniform(rng);   // :181
  if (tid == 0) {
    S.runs.run_rng[r] = rng.a;
    S.runs.run_rng[(size_t)R + r] = rng.b;
  }
  const double dn = (double)N, u_start = u / dn;   // :182
  for (int j = tid; j < N; j += kSmcBlock) {
    const double pos = u_start + (double)j / dn;   // :183
    out[j] = (int32_t)ratio_search(rcum, bs, pos, N, n_blocks, R, N, r);
  }
}

// rows 0 .. d - 1 of q [d][C] and, as row d, logp [C], gathered by idx inside every run (:192-193); in the
// bridged mode logb [C] travels as row d + 1 (null otherwise)
__global__ __launch_bounds__(256) void smc_gather_kernel(const double* __restrict__ q, const double* __restrict__ logp,
                                                        const double* __restrict__ logb,
                                                        const int32_t* __restrict__ idx, int d, int N, long long C,
                                                        double* __restrict__ q2, double* __restrict__ logp2,
                                                        double* __restrict__ logb2) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ((long long)d + (logb ? 2 : 1)) * C) return;
  const long long row = e / C, c = e - row * C;
  const long long src = (c / N) * N + idx[c];
  if (row < d) q2[e] = q[row * C + src];
  else if (row == d) logp2[c] = logp[src];
  else logb2[c] = logb[src];
}

// One workgroup per (run, dimension): estimate_scale (:197-207)
__global__ __launch_bounds__(kSmcBlock) void smc_scale_kernel(SmcStage S, const double* __restrict__ q, long long C) {
  __shared__ double red[kSmcBlock / 64];
  const int tid = threadIdx.x, r = blockIdx.x, i = blockIdx.y, N = S.n_particles, R = S.n_runs;
  if (S.runs.active[r] == 0) return;
  const double* v = q + (size_t)i * C + (size_t)r * N;
  const double mean = particle_sum(N, tid, red, [&](int j) { return v[j]; }) / (double)N;
  const double ss = particle_sum(N, tid, red, [&](int j) {
    const double t = v[j] - mean;
    return t * t;
  });
  const double var = ss / (double)(N - 1 > 1 ? N - 1 : 1);
  if (tid == 0) S.runs.scale[(size_t)i * R + r] = __dsqrt_rn(fmax(var, 1.0e-10)) * 2.38 / S.sqrt_d;
}

#endif

}  // namespace exmc
