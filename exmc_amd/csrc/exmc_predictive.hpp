// exmc_predictive.hpp -- posterior predictive replicates on the device: Exmc.Predictive.posterior_predictive
// (lib/exmc/predictive.ex:44-63, 98-108) over a device trace, for the built-in kinds (DESIGN.md
// "Posterior predictive"; C ABI include/exmc_hip_predictive.h).
//
// One lane owns one chain and its generator; one wavefront (one workgroup) owns 64 consecutive chains.
// Nothing is summed across lanes, so a chain's replicates do not depend on the launch shape. Per draw s:
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
  const uint64_t* zig_ki;
  const double* zig_wi;
  const double* zig_fi;
  double nor_r;
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

template <class Src>
__global__ __launch_bounds__(kPpBlock) void predictive_kernel(Src src, PredictiveParams P) {
  static_assert(kPpBlock == kIcTile, "one tile row per lane");
  extern __shared__ double ic_lds[];
  const int d = P.d, C = P.C, N = P.N;
  const int ld = ic_ld(d);
  double* tile = ic_lds;
  double* cst = ic_lds + (size_t)kIcTile * ld;
  const int tid = threadIdx.x;
  const long long c0 = (long long)blockIdx.x * kPpBlock;
  const long long c = c0 + tid;
  const bool live = c < C;
  const int nrow = (int)((C - c0 < kPpBlock) ? C - c0 : kPpBlock);   // rows of the tile that hold a chain
  double* lz = cst + (size_t)kIcTile * (kIcConsts + 1);
  for (int i = tid; i < 256; i += kPpBlock) {
    lz[i] = __longlong_as_double((long long)P.zig_ki[i]);
    lz[256 + i] = P.zig_wi[i];
    lz[512 + i] = P.zig_fi[i];
  }
  const ZigTables zt{(const uint64_t*)lz, lz + 256, lz + 512};   // (read after the loop's first barrier)
  Rng rng{0, 0};
  if (live) {
    if (P.resume) {
      rng.a = P.rng_state[c];
      rng.b = P.rng_state[(size_t)C + c];
    } else {
      rng_seed(rng, P.base_seed + 7919ULL * (uint64_t)(P.chain_lo + c));
    }
  }
  const PpRng g{rng, zt, P.nor_r};
  double* q = tile + (size_t)tid * ld;
  double* cq = cst + tid * (kIcConsts + 1) + 1;
  for (int s = 0; s < P.S; s++) {
    __syncthreads();   // the previous draw's tile has been read
    for (int e = tid; e < kIcTile * d; e += kPpBlock) {
      const int j = e / kIcTile, t = e - j * kIcTile;
      tile[(size_t)t * ld + j] = (t < nrow) ? P.draws[((size_t)s * d + j) * C + (c0 + t)] : 0.0;
    }
    __syncthreads();
    src.consts(q, cq);
    __syncthreads();
    src.prepare(tile, cst, ld, kIcTile, tid, kPpBlock);
    __syncthreads();
    if (!live) continue;
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
