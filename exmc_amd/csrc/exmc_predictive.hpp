// exmc_predictive.hpp -- posterior predictive replicates on the device: Exmc.Predictive.posterior_predictive
// (lib/exmc/predictive.ex:44-63, 98-108) over a device trace, for the built-in kinds (DESIGN.md
// "Posterior predictive"; C ABI include/exmc_hip_predictive.h).
//
// One lane owns one chain and its generator; one wavefront (one workgroup) owns 64 consecutive chains.
// Nothing is summed across lanes, so a chain's replicates do not depend on the launch shape. Per draw s
// (steps 1 and 2 are pp_stage, which ppc_kernel of exmc_ppc.hpp calls too):
//   1. stage: the 64 chains' rows of draw s into the LDS tile [64][ic_ld(d)] (coalesced over chains): 64
//      consecutive pooled samples of one draw, the tile the sources of exmc_ic.hpp take;
//   2. Src::consts, one lane per row, then Src::prepare with the wave as the cooperating group (radon's
//      county intercepts, sv_ncp's walk as a wave scan per row);
//   3. every lane with a chain walks the datums i = 0 .. N - 1 in order: the datum (a wave-uniform load),
//      Src::params at its own row, the family's sample/2 on its own generator, and the store to
//      yrep[(s N + i) C + c] (coalesced over chains).
// The ziggurat tables (6 KB) are staged into LDS behind the tile once per workgroup: a variate's two
// dependent table reads are LDS reads, not trips to L2.
// Lanes past C hold rows of zeros and take part in every barrier and wave-wide scan; they load, draw and
// store nothing. The ziggurat's slow paths and the gamma rejection loop diverge per lane by construction:
// the wave waits for its slowest lane at every datum, and the work per chain is serial by contract (one
// generator), so the throughput grows with C and not with S N.
//
// tests/predictive_statement.py restates every sampler; build with -ffp-contract=off.
#pragma once

#include "../../include/exmc_hip_predictive.h"
#include "exmc_ic.hpp"

namespace exmc {

constexpr int kPpBlock = 64;                             // chains per workgroup: one wavefront
constexpr int kPpGammaCap = EXMC_PREDICTIVE_GAMMA_CAP;   // rejections in a row after which a gamma variate is NaN

struct PredictiveParams {
  const double* draws;   // dev [S][d][C]
  double* yrep;          // dev [S][N][C]
  uint64_t* rng_state;   // dev [2][C] or null: in with resume, out always
  int S, d, C, N;
  int chain_lo, resume;
  uint64_t base_seed;
  RngArgs rng;
};

struct PpRng {
  Rng& r;
  const ZigTables& zt;
  double nor_r;
  __device__ __forceinline__ double normal() const { return rng_normal(r, zt, nor_r); }
  __device__ __forceinline__ double uniform() const { return rng_uniform(r); }
};

// normal.ex:33-39: mu_f + sigma_f * z, the product and the sum rounded separately
__device__ __forceinline__ double pp_sample(const NormalParams& p, const PpRng& g) {
  const double z = g.normal();
  return p.loc + p.scale * z;
}

// bernoulli.ex:36-41: p unclipped; a NaN p compares false
__device__ __forceinline__ double pp_sample(const BernoulliParams& p, const PpRng& g) {
  const double u = g.uniform();
  return (u < p.p) ? 1.0 : 0.0;
}

// gamma.ex:43-72, Marsaglia-Tsang. An alpha that is not >= 1 takes the boost once, Gamma(alpha + 1) *
// u^(1 / alpha), the power as exp((1 / alpha) log u). After kPpGammaCap rejections in a row (v <= 0 or
// the log test) the variate is NaN; the boost's uniform is drawn all the same.
__device__ inline double pp_gamma(double alpha, double beta, const PpRng& g) {
  const bool boost = !(alpha >= 1.0);
  const double a = boost ? alpha + 1.0 : alpha;
  const double d = a - 1.0 / 3.0;
  const double c = 1.0 / sqrt(9.0 * d);
  double value = __builtin_nan("");
  for (int k = 0; k < kPpGammaCap; k++) {
    const double x = g.normal();
    const double v1 = 1.0 + c * x;
    if (v1 <= 0.0) continue;
    const double v = (v1 * v1) * v1;
    const double u = g.uniform();
    if (exmc_log(u) < (((0.5 * x) * x + d) - d * v) + d * exmc_log(v)) {
      value = (d * v) / beta;
      break;
    }
  }
  if (boost) {
    const double u = g.uniform();
    value = value * exmc_exp((1.0 / alpha) * exmc_log(u));
  }
  return value;
}

// student_t.ex:38-46: the normal first, then the chi-square as Gamma(df / 2, 0.5)
__device__ __forceinline__ double pp_sample(const StudentTParams& p, const PpRng& g) {
  const double z = g.normal();
  const double chi2 = pp_gamma(p.df / 2.0, 0.5, g);
  return p.loc + (p.scale * z) / sqrt(chi2 / p.df);
}

// datum i after datum i - 1 (prev): Src::load(i), except that radon's county search goes on from the
// county of the datum before (the datums are sorted by county; the result is load(i)'s)
template <class Src>
__device__ __forceinline__ typename Src::Datum pp_load(const Src& src, int i, const typename Src::Datum&) {
  return src.load(i);
}
__device__ __forceinline__ IcRadonSrc::Datum pp_load(const IcRadonSrc& src, int i, const IcRadonSrc::Datum& prev) {
  int j = (i == 0) ? 0 : prev.j;
  while (j + 1 < IcRadonSrc::J && (double)i >= src.cs[j + 1]) j++;
  return {src.fl[i], src.y[i], j};
}

// dynamic LDS: the tile and the constants of ic_lds_bytes(d), then the ziggurat tables ki, wi, fi [256] each
__host__ __device__ inline size_t pp_lds_bytes(int d) { return ic_lds_bytes(d) + (size_t)3 * 256 * 8; }

// The walk over a device trace that predictive_kernel and ppc_kernel (exmc_ppc.hpp) share: lane = chain,
// one wavefront per 64 consecutive chains. The LDS is carved by pp_tile_row / pp_const_row / pp_tables_at /
// pp_behind, pp_seed gives the lane its chain's generator and pp_stage readies draw s; what a kernel does
// with the replicates pp_sample(src.params(dat, q, cq), g) of the staged draw is its own. (Plain values, no
// walk object, and the table copy written out in both: DESIGN.md, profiles/fit_pp_refactor, for why.)
__device__ __forceinline__ double* pp_consts_at(double* lds, int d) { return lds + (size_t)kIcTile * ic_ld(d); }
__device__ __forceinline__ double* pp_tables_at(double* lds, int d) {
  return pp_consts_at(lds, d) + (size_t)kIcTile * (kIcConsts + 1);
}
__device__ __forceinline__ double* pp_behind(double* lds, int d) { return pp_tables_at(lds, d) + 3 * 256; }
// row `t` of the tile [64][ic_ld(d)] and of the constants [64][kIcConsts + 1]
__device__ __forceinline__ double* pp_tile_row(double* lds, int d, int t) { return lds + (size_t)t * ic_ld(d); }
__device__ __forceinline__ double* pp_const_row(double* lds, int d, int t) {
  return pp_consts_at(lds, d) + t * (kIcConsts + 1) + 1;
}
__device__ __forceinline__ int pp_rows(int C) {   // rows of the workgroup's tile that hold a chain
  const long long c0 = (long long)blockIdx.x * kPpBlock;
  return (int)((C - c0 < kPpBlock) ? C - c0 : kPpBlock);
}

// the generator of chain chain_lo + c (c < C), or with `resume` the one a call before left in state [2][C]
__device__ __forceinline__ void pp_seed(Rng& rng, long long c, int C, uint64_t base_seed, int chain_lo, bool resume,
                                        const uint64_t* state) {
  if (c < C) {
    if (resume) {
      rng.a = state[c];
      rng.b = state[(size_t)C + c];
    } else {
      rng_seed(rng, base_seed + 7919ULL * (uint64_t)(chain_lo + c));
    }
  }
}

// draw s of draws [S][d][C] into the tile, Src::consts and Src::prepare; every lane of the workgroup
// calls it for every draw (four barriers)
template <class Src>
__device__ __forceinline__ void pp_stage(const Src& src, double* lds, const double* draws, int s, int d, int C) {
  static_assert(kPpBlock == kIcTile, "one tile row per lane");
  const int ld = ic_ld(d), tid = threadIdx.x, nrow = pp_rows(C);
  const long long c0 = (long long)blockIdx.x * kPpBlock;
  __syncthreads();   // the previous draw's tile has been read
  for (int e = tid; e < kIcTile * d; e += kPpBlock) {
    const int j = e / kIcTile, t = e - j * kIcTile;
    lds[(size_t)t * ld + j] = (t < nrow) ? draws[((size_t)s * d + j) * C + (c0 + t)] : 0.0;
  }
  __syncthreads();
  src.consts(pp_tile_row(lds, d, tid), pp_const_row(lds, d, tid));
  __syncthreads();
  src.prepare(lds, pp_consts_at(lds, d), ld, kIcTile, tid, kPpBlock);
  __syncthreads();
}

template <class Src>
__global__ __launch_bounds__(kPpBlock) void predictive_kernel(Src src, PredictiveParams P) {
  extern __shared__ double ic_lds[];
  const int d = P.d, C = P.C, N = P.N;
  const int tid = threadIdx.x;
  const long long c = (long long)blockIdx.x * kPpBlock + tid;
  const bool live = c < C;
  double* lz = pp_tables_at(ic_lds, d);
  for (int i = tid; i < 256; i += kPpBlock) {
    lz[i] = __longlong_as_double((long long)P.rng.ki[i]);
    lz[256 + i] = P.rng.wi[i];
    lz[512 + i] = P.rng.fi[i];
  }
  const ZigTables zt{(const uint64_t*)lz, lz + 256, lz + 512};   // (read after pp_stage's first barrier)
  Rng rng{0, 0};
  pp_seed(rng, c, C, P.base_seed, P.chain_lo, P.resume, P.rng_state);
  const PpRng g{rng, zt, P.rng.nor_r};
  const double* q = pp_tile_row(ic_lds, d, tid);
  const double* cq = pp_const_row(ic_lds, d, tid);
  for (int s = 0; s < P.S; s++) {
    pp_stage(src, ic_lds, P.draws, s, d, C);
    if (!live) continue;   // after the draw's last barrier
    double* out = P.yrep + (size_t)s * N * C + c;
    typename Src::Datum dat{};
    for (int i = 0; i < N; i++) {
      dat = pp_load(src, i, dat);
      out[(size_t)i * C] = pp_sample(src.params(dat, q, cq), g);
    }
  }
  if (live && P.rng_state) {
    P.rng_state[c] = rng.a;
    P.rng_state[(size_t)C + c] = rng.b;
  }
}

}  // namespace exmc
