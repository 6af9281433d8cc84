// exmc_ppc.hpp -- posterior predictive checks on the device, without the replicate matrix: per datum
// where the observation falls among its replicates and the replicates' first two moments, per replicated
// data set four test statistics against the observed ones (DESIGN.md "Posterior predictive checks"; C ABI
// include/exmc_hip_ppc.h, which states the arithmetic).
//
// The walk over the trace and the replicates are predictive_kernel's, by the same calls (exmc_predictive.hpp,
// "The walk": the LDS carve-up with tile2 at pp_behind, pp_seed, pp_stage; per datum pp_load, Src::params
// and pp_sample on the chain's own generator). What a replicate goes into differs:
//   - its chain's statistics of the draw (A, Bq, mn, mx): lane-local, the datums ascending;
//   - its datum's running sums over chains and draws (E, E2, n_lt, n_eq): the transpose below.
// The datums are walked in groups of 64. Draw phase: every lane with a chain draws the group's datums in
// order and writes replicate k of the group to tile2[k * 65 + lane] (consecutive lanes, consecutive
// addresses). After a barrier, accumulate phase: lane j owns datum 64 g + j and holds its four
// accumulators from their one-writer slot of the global outputs (zeros at the first draw), walks the rows
// c = 0 .. nrow - 1 that hold a chain reading tile2[j * 65 + c], and stores them back: one running sum per
// (block, datum), strictly left to right over (draw, chain), no partial sums and nothing across lanes. The row stride of 65 doubles puts lane j's
// read at dword bank (2 j + 2 c) mod 64: the 32 lanes of a half of a ds_read_b64 hit 32 distinct bank
// pairs (the d | 1 stride of the parameter tile, for the same reason). A second barrier precedes the next
// group's stores.
// Lanes past C have no chain: they draw nothing and keep no statistics, but reach every barrier and own
// their datums in the accumulate phase. The generators diverge inside the draw phase (ziggurat tail, gamma
// loop) and reconverge at the barrier.
//
// tests/ppc_statement.py restates the reductions; build with -ffp-contract=off.
#pragma once

#include "../../include/exmc_hip_ppc.h"
#include "exmc_predictive.hpp"

namespace exmc {

constexpr int kPpcStats = EXMC_PPC_NSTAT;
constexpr int kPpcStride = kPpBlock + 1;   // doubles per row of the transpose tile
static_assert(kPpBlock == EXMC_PPC_BLOCK, "the blocks of the per-datum sums are the workgroups' chains");

struct PpcParams {
  const double* draws;       // dev [S][d][C]
  double* datum_sums;        // dev [B][N][2]: E, E2
  long long* datum_counts;   // dev [B][N][2]: n_lt, n_eq
  int* chain_counts;         // dev [4][C]
  double* tstat;             // dev [S][4][C] or null
  int S, d, C, N;
  int chain_lo;
  uint64_t base_seed;
  double m0;                 // the observed mean
  double t_obs[kPpcStats];   // the observed statistics: mean, var, min, max
  RngArgs rng;
};

// dynamic LDS: pp_lds_bytes(d) (the tile, the constants, the ziggurat tables), then tile2 [64][65] at pp_behind
__host__ __device__ inline size_t ppc_lds_bytes(int d) {
  return pp_lds_bytes(d) + (size_t)kPpBlock * kPpcStride * 8;
}

// the observed values in the handle's order, for the host (m0, t_obs and the finishing expressions)
template <class Src>
__global__ __launch_bounds__(256) void ppc_obs_kernel(Src src, int N, double* __restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) y[i] = src.obs(i);
}

template <class Src>
__global__ __launch_bounds__(kPpBlock) void ppc_kernel(Src src, PpcParams P) {
  extern __shared__ double ic_lds[];
  const int d = P.d, C = P.C, N = P.N;
  const int tid = threadIdx.x, nrow = pp_rows(C);
  const long long c = (long long)blockIdx.x * kPpBlock + tid;
  const bool live = c < C;
  double* const tile2 = pp_behind(ic_lds, d);
  double* lz = pp_tables_at(ic_lds, d);
  for (int i = tid; i < 256; i += kPpBlock) {
    lz[i] = __longlong_as_double((long long)P.rng.ki[i]);
    lz[256 + i] = P.rng.wi[i];
    lz[512 + i] = P.rng.fi[i];
  }
  const ZigTables zt{(const uint64_t*)lz, lz + 256, lz + 512};   // (read after pp_stage's first barrier)
  Rng rng{0, 0};
  pp_seed(rng, c, C, P.base_seed, P.chain_lo, false, nullptr);
  const PpRng g{rng, zt, P.rng.nor_r};
  const double* q = pp_tile_row(ic_lds, d, tid);
  const double* cq = pp_const_row(ic_lds, d, tid);
  const double Nd = (double)N, m0 = P.m0;
  int cnt[kPpcStats] = {0, 0, 0, 0};
  // the block's slots of the per-datum outputs: [N][2] each
  double* bsum = P.datum_sums + (size_t)blockIdx.x * N * 2;
  long long* bcnt = P.datum_counts + (size_t)blockIdx.x * N * 2;
  for (int s = 0; s < P.S; s++) {
    pp_stage(src, ic_lds, P.draws, s, d, C);
    double A = 0.0, Bq = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
    typename Src::Datum dat{};
    for (int i0 = 0; i0 < N; i0 += kPpBlock) {
      const int ng = (N - i0 < kPpBlock) ? N - i0 : kPpBlock;   // datums of the group
      if (live) {
        for (int k = 0; k < ng; k++) {
          dat = pp_load(src, i0 + k, dat);
          const double v = pp_sample(src.params(dat, q, cq), g);
          tile2[k * kPpcStride + tid] = v;
          const double e = v - m0;
          A = A + e;
          Bq = Bq + e * e;
          mn = (v < mn) ? v : mn;
          mx = (v > mx) ? v : mx;
        }
      }
      __syncthreads();
      if (tid < ng) {
        // (asking for the accumulators before the draw phase, to hide the trip, was measured: nothing for
        // eight_schools, and logistic's draw loop a third slower)
        const size_t slot = (size_t)(i0 + tid) * 2;
        const double y = src.obs(i0 + tid);
        double E = 0.0, E2 = 0.0;
        long long n_lt = 0, n_eq = 0;
        if (s > 0) {
          E = bsum[slot];
          E2 = bsum[slot + 1];
          n_lt = bcnt[slot];
          n_eq = bcnt[slot + 1];
        }
        const double* row = tile2 + tid * kPpcStride;
        for (int r = 0; r < nrow; r++) {
          const double v = row[r];
          const double e = v - y;
          E = E + e;
          E2 = E2 + e * e;
          n_lt += (v < y) ? 1 : 0;
          n_eq += (v == y) ? 1 : 0;
        }
        bsum[slot] = E;
        bsum[slot + 1] = E2;
        bcnt[slot] = n_lt;
        bcnt[slot + 1] = n_eq;
      }
      __syncthreads();   // the group's replicates have been read
    }
    if (live) {
      const double T[kPpcStats] = {m0 + A / Nd, (Bq - (A * A) / Nd) / (Nd - 1.0), mn, mx};
#pragma unroll
      for (int k = 0; k < kPpcStats; k++) {
        cnt[k] += (T[k] >= P.t_obs[k]) ? 1 : 0;
        if (P.tstat) P.tstat[((size_t)s * kPpcStats + k) * C + c] = T[k];
      }
    }
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < kPpcStats; k++) P.chain_counts[(size_t)k * C + c] = cnt[k];
  }
}

}  // namespace exmc
