// exmc_prior.hpp -- prior and prior predictive samples on the device: Exmc.Predictive.prior_samples
// (lib/exmc/predictive.ex:19-33, 73-83, 140-196) for the built-in kinds (DESIGN.md "Prior predictive";
// C ABI include/exmc_hip_prior.h).
//
// The shape is predictive_kernel's (exmc_predictive.hpp): one lane owns one chain and its generator, one
// wavefront (one workgroup) owns 64 consecutive chains, the ziggurat tables sit in LDS behind the tile and
// the constants. Where predictive_kernel stages a trace row, every lane here FILLS its own row of the tile
// [64][ic_ld(d)] (the d | 1 stride: lane t's row starts t (d | 1) doubles in, an odd stride, so the 64 lanes'
// accesses to one dimension fall into 64 different bank pairs). Per draw s:
//   1. walk: the kind's prior program, one entry per free variable in the reference's Kahn order (the
//      host builds it, exmc_hip.hip prior_program). An entry names the variable's kernel dimension, its
//      family and two parameters, each a literal or the dimension of an earlier variable, whose
//      sampled constrained value the lane reads back from its row. The value goes into the row and to
//      x[(s d + j) C + c] (coalesced over chains);
//   2. the row is turned into the unconstrained position in place -- exmc_log for a :log variable -- and
//      goes to q[(s d + j) C + c];
//   3. Src::consts and Src::prepare with pp_stage's barriers: from here on the tile is what
//      predictive_kernel has after staging row q;
//   4. (sv_ncp) the walk s_2 .. s_100 that prepare reconstructed goes to x;
//   5. with yrep: the datums i = 0 .. N - 1 as predictive_kernel draws them, pp_sample(src.params(...)).
// The program is the same for every lane, so the family switch is wave-uniform; what diverges is what
// diverges in predictive_kernel: the ziggurat's slow paths and the gamma rejection loop.
// Lanes past C hold rows of zeros and take part in every barrier and wave-wide scan; they draw and store
// nothing.
//
// tests/prior_statement.py restates the walk; build with -ffp-contract=off.
#pragma once

#include "../../include/exmc_hip_prior.h"
#include "exmc_predictive.hpp"

namespace exmc {

enum PriorFamily : int { kPriorNormal = 0, kPriorHalfCauchy = 1, kPriorExponential = 2 };

// one free variable of the walk. A parameter is lit[k] where ref[k] < 0, else the sampled constrained
// value of kernel dimension ref[k] (an earlier entry: resolve_params, predictive.ex:115-120).
// Normal: (mu, sigma); HalfCauchy: (scale, -); Exponential: (lambda, -).
struct PriorEntry {
  int dim;      // kernel dimension of the variable
  int family;   // PriorFamily
  int log;      // 1: the variable's transform is :log, q = exmc_log(x)
  int ref[2];
  int pad;
  double lit[2];
};

struct PriorParams {
  const PriorEntry* prog;   // dev [d], walk order
  double* x;                // dev [S][d][C] constrained
  double* q;                // dev [S][d][C] unconstrained: a trace row of the handle
  double* yrep;             // dev [S][N][C] or null: no datum is drawn
  uint64_t* rng_state;      // dev [2][C] or null: in with resume, out always
  int S, d, C, N;
  int chain_lo, resume;
  int xwalk;                // sv_ncp: dimensions 1 .. xwalk - 1 of x are the walk prepare reconstructs (else 0)
  uint64_t base_seed;
  RngArgs rng;
};

// normal.ex:33-39, half_cauchy.ex:34-40 (the tangent: exmc_tan_halfpi, of the exact (pi/2) u),
// exponential.ex:26-31
__device__ __forceinline__ double prior_sample(int family, double p0, double p1, const PpRng& g) {
  if (family == kPriorNormal) {
    const double z = g.normal();
    return p0 + p1 * z;
  }
  const double u = g.uniform();
  if (family == kPriorHalfCauchy) return p0 * exmc_tan_halfpi(u);
  return (-exmc_log(u)) / p0;
}

template <class Src>
__global__ __launch_bounds__(kPpBlock) void prior_kernel(Src src, PriorParams P) {
  static_assert(kPpBlock == kIcTile, "one tile row per lane");
  extern __shared__ double ic_lds[];
  const int d = P.d, C = P.C, N = P.N;
  const int tid = threadIdx.x, ld = ic_ld(d);
  const long long c = (long long)blockIdx.x * kPpBlock + tid;
  const bool live = c < C;
  double* lz = pp_tables_at(ic_lds, d);
  for (int i = tid; i < 256; i += kPpBlock) {
    lz[i] = __longlong_as_double((long long)P.rng.ki[i]);
    lz[256 + i] = P.rng.wi[i];
    lz[512 + i] = P.rng.fi[i];
  }
  const ZigTables zt{(const uint64_t*)lz, lz + 256, lz + 512};   // (read after the first barrier)
  Rng rng{0, 0};
  pp_seed(rng, c, C, P.base_seed, P.chain_lo, P.resume, P.rng_state);
  const PpRng g{rng, zt, P.rng.nor_r};
  double* row = pp_tile_row(ic_lds, d, tid);
  const double* cq = pp_const_row(ic_lds, d, tid);
  for (int s = 0; s < P.S; s++) {
    __syncthreads();   // the previous draw's tile has been read (and, the first time, the tables are there)
    if (live) {
      double* xo = P.x + (size_t)s * d * C + c;
      double* qo = P.q + (size_t)s * d * C + c;
      for (int e = 0; e < d; e++) {
        const PriorEntry en = P.prog[e];   // wave-uniform
        const double p0 = (en.ref[0] < 0) ? en.lit[0] : row[en.ref[0]];
        const double p1 = (en.ref[1] < 0) ? en.lit[1] : row[en.ref[1]];
        const double v = prior_sample(en.family, p0, p1, g);
        row[en.dim] = v;
        if (!(en.dim >= 1 && en.dim < P.xwalk)) xo[(size_t)en.dim * C] = v;
      }
      for (int e = 0; e < d; e++) {
        const int j = P.prog[e].dim;
        double v = row[j];
        if (P.prog[e].log) {
          v = exmc_log(v);
          row[j] = v;
        }
        qo[(size_t)j * C] = v;
      }
    } else {
      for (int j = 0; j < d; j++) row[j] = 0.0;
    }
    __syncthreads();
    src.consts(row, pp_const_row(ic_lds, d, tid));
    __syncthreads();
    src.prepare(ic_lds, pp_consts_at(ic_lds, d), ld, kIcTile, tid, kPpBlock);
    __syncthreads();
    if (!live) continue;   // after the draw's last barrier
    {
      double* xo = P.x + (size_t)s * d * C + c;
      for (int j = 1; j < P.xwalk; j++) xo[(size_t)j * C] = row[j];
    }
    if (!P.yrep) continue;
    double* out = P.yrep + (size_t)s * N * C + c;
    typename Src::Datum dat{};
    for (int i = 0; i < N; i++) {
      dat = pp_load(src, i, dat);
      out[(size_t)i * C] = pp_sample(src.params(dat, row, cq), g);
    }
  }
  if (live && P.rng_state) {
    P.rng_state[c] = rng.a;
    P.rng_state[(size_t)C + c] = rng.b;
  }
}

}  // namespace exmc
