// exmc_kernels.hpp — the other gfx950 kernels of the hot path (the NUTS transition kernel and
// the adaptation warmup are in exmc_nuts.hpp).
//
//   multi_step_kernel  B2 `multi_step_fn` contract, chain-batched (batched_leapfrog.ex:50-101).
//   init_chains_kernel seed :rand, init position, first logp/grad (sampler.ex:154-165,339-349).
//   find_eps_kernel    find_reasonable_epsilon_with_rng (sampler.ex:451-530).
//   logp_grad_kernel   vag_fn batched (compiler.ex:131-141).
// (The kernels that are no template on a model -- the diagnostics, the fused normal chain -- are
// in exmc_diag.hpp.)
//
// All are launched with one wavefront per workgroup (64 threads) and M::kExtraLdsDoubles * 8
// bytes of dynamic LDS. For wave-cooperative models (M::kCoop, the MFMA logistic) lane groups
// without a chain shadow the last chain instead of leaving, so that logp_grad sees a full wave.
#pragma once

#include "exmc_nuts.hpp"

namespace exmc {

constexpr int kAuxBlock = 64;

template <class M>
__host__ __device__ constexpr size_t aux_lds_bytes() { return (size_t)M::kExtraLdsDoubles * 8; }

template <class M>
__device__ __forceinline__ void attach_scratch(typename M::Lane& ln, double* sh) {
  if constexpr (M::kExtraLdsDoubles > 0) ln.sh = sh;
}

// ------------------------------------------------------------------------------------------
// B2: chain-batched multi_step (batched_leapfrog.ex:50-101). all_* rows are [step][dim][chain].
// ------------------------------------------------------------------------------------------
struct MultiStepParams {
  const double* q;  // [D][C]
  const double* p;
  const double* g;
  double eps;
  const double* inv_mass;  // dev [D]
  int n_steps;
  int n_chains;
  double* all_q;     // [n][D][C]
  double* all_p;
  double* all_g;
  double* all_logp;  // [n][C]
};

template <class M, int G>
__global__ void __launch_bounds__(kAuxBlock) multi_step_kernel(MultiStepParams P,
                                                               typename M::Consts mc) {
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
  double q[DPL], p[DPL], g[DPL], im[DPL];
  bool valid[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    const int i = l + k * G;
    valid[k] = i < D;
    const size_t o = (size_t)i * C + chain;
    q[k] = valid[k] ? P.q[o] : 0.0;
    p[k] = valid[k] ? P.p[o] : 0.0;
    g[k] = valid[k] ? P.g[o] : 0.0;
    im[k] = valid[k] ? P.inv_mass[i] : 1.0;
  }
  const double eps = P.eps;
  const double h = eps / 2.0;
  for (int s = 0; s < P.n_steps; s++) {
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      const double ph = p[k] + h * g[k];
      p[k] = ph;
      q[k] = q[k] + eps * (im[k] * ph);
    }
    const double logp = M::logp_grad(mc, ln, l, q, g);
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      p[k] = p[k] + h * g[k];
      if (valid[k] && has_chain) {
        const size_t o = ((size_t)s * D + (l + k * G)) * C + chain;
        P.all_q[o] = q[k];
        P.all_p[o] = p[k];
        P.all_g[o] = g[k];
      }
    }
    if (l == 0 && has_chain) P.all_logp[(size_t)s * C + chain] = logp;
  }
}

// vag_fn batched: q [D][C] -> logp [C], grad [D][C]
template <class M, int G>
__global__ void __launch_bounds__(kAuxBlock)
logp_grad_kernel(const double* qin, int C, double* logp, double* grad, typename M::Consts mc) {
  constexpr int D = M::D, DPL = M::DPL;
  extern __shared__ double xlds[];
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int l = threadIdx.x & (G - 1);
  const bool has_chain = (tid / G) < C;
  const int chain = has_chain ? (tid / G) : (C - 1);
  if (!M::kCoop && !has_chain) return;
  typename M::Lane ln;
  M::load(mc, l, ln);
  attach_scratch<M>(ln, xlds);
  double q[DPL], g[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    const int i = l + k * G;
    q[k] = (i < D) ? qin[(size_t)i * C + chain] : 0.0;
    g[k] = 0.0;
  }
  const double lp = M::logp_grad(mc, ln, l, q, g);
  if (!has_chain) return;
  if (l == 0) logp[chain] = lp;
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    const int i = l + k * G;
    if (i < D) grad[(size_t)i * C + chain] = g[k];
  }
}

// sampler.ex:154-165, 339-349, 1083-1093: seed, initial position, first logp/grad
struct InitParams {
  ChainState st;
  int n_chains;
  int chain_lo;
  uint64_t base_seed;
  const double* init_q;  // dev [D] or null
  const uint64_t* zig_ki;
  const double* zig_wi;
  const double* zig_fi;
  double nor_r;
  FlatOrder flat;
};

template <class M, int G>
__global__ void __launch_bounds__(kAuxBlock) init_chains_kernel(InitParams P,
                                                                typename M::Consts mc) {
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
  const ZigTables zt{P.zig_ki, P.zig_wi, P.zig_fi};
  Rng rng;
  rng_seed(rng, P.base_seed + 7919ULL * (uint64_t)(P.chain_lo + chain));
  double q[DPL], g[DPL];
#pragma unroll
  for (int k = 0; k < DPL; k++) q[k] = g[k] = 0.0;
  if (P.init_q) {
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      const int i = l + k * G;
      if (i < D) q[k] = P.init_q[i];
    }
  } else {
    // sampler.ex:339-349: variate r fills entry r of the reference's flat vector
    int rank[DPL];
#pragma unroll
    for (int k = 0; k < DPL; k++) {
      const int i = l + k * G;
      rank[k] = (i < D) ? (P.flat.rank ? P.flat.rank[i] : i) : D;
    }
    for (int r = 0; r < D; r++) {
      const double z = rng_normal(rng, zt, P.nor_r);
#pragma unroll
      for (int k = 0; k < DPL; k++)
        if (rank[k] == r) q[k] = z * 0.1;
    }
  }
  const double lp = M::logp_grad(mc, ln, l, q, g);
  if (!has_chain) return;
  if (l == 0) {
    P.st.logp[chain] = lp;
    P.st.rng[chain] = rng.a;
    P.st.rng[(size_t)C + chain] = rng.b;
  }
#pragma unroll
  for (int k = 0; k < DPL; k++) {
    const int i = l + k * G;
    if (i < D) {
      P.st.q[(size_t)i * C + chain] = q[k];
      P.st.g[(size_t)i * C + chain] = g[k];
    }
  }
}

// find_reasonable_epsilon_with_rng (sampler.ex:451-530) for chain 0 of the state buffers (the
// host-driven warmup path; the device warmup calls find_eps_dev directly). Launched with
// nuts_lds_bytes<M, 0>() of dynamic LDS.
struct FindEpsParams {
  ChainState st;
  int n_chains;
  const double* inv_mass;
  const double* sqrt_inv_mass;
  double log_half;  // libm log(0.5), computed on the host as :math.log(0.5)
  double* eps_out;
  const uint64_t* zig_ki;
  const double* zig_wi;
  const double* zig_fi;
  double nor_r;
  FlatOrder flat;
};

template <class M, int G>
__global__ void __launch_bounds__(kNutsBlock) find_eps_kernel(FindEpsParams P,
                                                              typename M::Consts mc) {
  constexpr int DPL = M::DPL;
  constexpr int NSLOT = nuts_nslot<M>();
  extern __shared__ double lds[];
  const ZigTables zt = stage_zig_tables<0, NSLOT>(lds, P.zig_ki, P.zig_wi, P.zig_fi);
  const bool writer = threadIdx.x < G;
  if (blockIdx.x != 0 || (!M::kCoop && !writer)) return;
  NutsLane<M, G> L;
  lane_setup<M, G, 0>(L, mc, lds, nullptr, P.inv_mass, P.sqrt_inv_mass, zt, P.nor_r, P.flat);
  ChainRegs<DPL> st;
  chain_load<M, G>(P.st, P.n_chains, 0, L.l, st);
  const double eps = find_eps_dev<M, G>(mc, L, st, P.log_half);
  if (writer && L.l == 0) {
    *P.eps_out = eps;
    P.st.rng[0] = st.rng.a;
    P.st.rng[(size_t)P.n_chains] = st.rng.b;
  }
}

}  // namespace exmc

#include "exmc_gen_pointwise.hpp"   // gen_pointwise_kernel of a plug-in generated with pointwise terms
#include "exmc_pathfinder.hpp"      // pathfinder_kernel: Exmc.Pathfinder, one L-BFGS path per lane group
#include "exmc_advi.hpp"            // advi_kernel: Exmc.ADVI, one mean-field fit per lane group
#include "exmc_fit_psis.hpp"        // fit_log_ratio_kernel: log p - log q of the fits' draws
#include "exmc_smc.hpp"             // smc_init_kernel, smc_mutate_kernel: Exmc.SMC, one particle per lane group
#ifndef EXMC_ONLY_CUSTOM            // a generated model's plug-in carries no predictive kernels
#include "exmc_predictive.hpp"      // predictive_kernel: Exmc.Predictive, one chain's generator per lane
#include "exmc_ppc.hpp"             // ppc_kernel: posterior predictive checks, the replicates reduced in place
#include "exmc_loo_pit.hpp"         // loo_pit_kernel: PSIS-LOO-PIT, the replicates weighted where they are drawn
#include "exmc_prior.hpp"           // prior_kernel: Exmc.Predictive.prior_samples, every lane fills its own row
#endif
