// exmc_loo_pit.hpp -- PSIS-LOO-PIT on the device: where every observation falls among its posterior
// predictive replicates when each replicate carries the Pareto-smoothed leave-one-out weight of its sample
// (DESIGN.md "LOO-PIT"; C ABI include/exmc_hip_loo_pit.h, which states the arithmetic). It joins the two
// halves that exist: psis_tail_kernel (exmc_psis.hpp) leaves every datum's sorted, smoothed tail in global
// tables, and the walk of ppc_kernel (exmc_ppc.hpp) draws every replicate and transposes it so that one lane
// owns one datum. No replicate matrix and no pointwise matrix in the second pass.
//
//   loo_pit_kernel<Src>: ppc_kernel's walk (pp_seed, pp_stage, pp_load, pp_sample, groups of 64 datums).
//     Draw phase: every lane with a chain writes, per datum k of the group, its replicate to
//     tile2[k * 65 + lane] and its term src.term(dat, q, cq) to tile3[k * 65 + lane] (the bits of
//     pointwise_ll_range_kernel: the same tile row, constants and prepare). Accumulate phase: lane j owns
//     datum 64 g + j, holds (m, sA, sL, sQ) from its one-writer slot [B][N][4] (the initial state at s = 0),
//     walks the rows that hold a chain (loo_pit_rows) and stores back. Nothing is summed across lanes.
//   loo_pit_ll_kernel: the same contract from matrices ll, yrep [S][N][C] and y [N]: one workgroup per
//     (block of 64 chains, group of 64 datums) stages both [64 datums][64 chains] slabs of a draw through
//     the same stride-65 tiles (global reads coalesced over chains) and runs loo_pit_rows; the state stays
//     in registers over the draws.
//   loo_pit_merge_kernel: the blocks left to right (loo_pit_merge), then p_lt, p_eq, pit, k.
//
// The smoothed log weight of sample k is the x psis_weights_kernel pushes: -ll - max, for a tail sample of
// a smoothed datum the table entry found by binary search of (key, k) -- some M / n of the samples -- then
// fmin(x, 0.0). Build with -ffp-contract=off.
#pragma once

#include "../../include/exmc_hip_loo_pit.h"
#include "exmc_ppc.hpp"
#include "exmc_psis.hpp"

namespace exmc {

constexpr int kLooPitFields = 4;   // block state: m, sA, sL, sQ
constexpr int kLooPitRows = EXMC_LOO_PIT_ROWS;
static_assert(kPpBlock == EXMC_LOO_PIT_BLOCK, "the blocks of the per-datum states are the workgroups' chains");

// the tables psis_tail_kernel wrote for the datums of the call: rows of P entries, meta [N][kPsisMeta]
struct LooPitTables {
  const uint64_t* keys;
  const uint32_t* idx;
  const double* xs;
  const double* meta;
  int P;
};

struct LooPitParams {
  const double* draws;   // dev [S][d][C]
  double* state;         // dev [B][N][4]
  LooPitTables tab;
  int S, d, C, N;
  int chain_lo;
  uint64_t base_seed;
  RngArgs rng;
};

// dynamic LDS: ppc_kernel's (the tile, the constants, the ziggurat tables, tile2), then tile3 [64][65]
__host__ __device__ inline size_t loo_pit_lds_bytes(int d) {
  return ppc_lds_bytes(d) + (size_t)kPpBlock * kPpcStride * 8;
}

struct LooPitState {
  double m, sA, sL, sQ;
};

// include/exmc_hip_loo_pit.h "Accumulation": the branches of ic_lse_push, three sums on one maximum
__device__ __forceinline__ void loo_pit_push(LooPitState& st, double x, bool lt, bool eq) {
  const double fL = lt ? 1.0 : 0.0, fQ = eq ? 1.0 : 0.0;
  if (!(x == x)) {
    st.m = x;
    st.sA = x;
    st.sL = x;
    st.sQ = x;
  } else if (x == -__builtin_inf()) {
  } else if (x > st.m) {
    const double r = exmc_exp(st.m - x);
    st.sA = st.sA * r + 1.0;
    st.sL = st.sL * r + fL;
    st.sQ = st.sQ * r + fQ;
    st.m = x;
  } else if (x == st.m) {
    st.sA = st.sA + 1.0;
    st.sL = st.sL + fL;
    st.sQ = st.sQ + fQ;
  } else {
    const double e = exmc_exp(x - st.m);
    st.sA = st.sA + e;
    if (lt) st.sL = st.sL + e;
    if (eq) st.sQ = st.sQ + e;
  }
}

// "Finish": the common-maximum analogue of ic_lse_merge
__device__ __forceinline__ void loo_pit_merge(LooPitState& a, const LooPitState& b) {
  if (!(a.m == a.m) || !(b.m == b.m)) {
    const double nan = __builtin_nan("");
    a.m = nan;
    a.sA = nan;
    a.sL = nan;
    a.sQ = nan;
  } else if (b.m == -__builtin_inf()) {
  } else if (a.m == -__builtin_inf()) {
    a = b;
  } else if (a.m == b.m) {
    a.sA = a.sA + b.sA;
    a.sL = a.sL + b.sL;
    a.sQ = a.sQ + b.sQ;
  } else if (a.m > b.m) {
    const double r = exmc_exp(b.m - a.m);
    a.sA = a.sA + b.sA * r;
    a.sL = a.sL + b.sL * r;
    a.sQ = a.sQ + b.sQ * r;
  } else {
    const double r = exmc_exp(a.m - b.m);
    a.sA = a.sA * r + b.sA;
    a.sL = a.sL * r + b.sL;
    a.sQ = a.sQ * r + b.sQ;
    a.m = b.m;
  }
}

// what a lane keeps of its datum for the accumulate phase
struct LooPitDatum {
  const uint64_t* keys;
  const uint32_t* idx;
  const double* xs;
  double mx, cutoff, y;
  int T;
  bool smooth;
};
__device__ __forceinline__ LooPitDatum loo_pit_datum(const LooPitTables& tab, int i, double y) {
  const double* mt = tab.meta + (size_t)i * kPsisMeta;
  return {tab.keys + (size_t)i * tab.P, tab.idx + (size_t)i * tab.P, tab.xs + (size_t)i * tab.P,
          mt[0], mt[1], y, (int)mt[2], mt[4] != 0.0};
}

// the accumulate phase of one draw: the lane's datum against the nrow chains of its tile rows, replicates
// in vrow and terms in lrow, sample indices k0, k0 + 1, ... (A search of the table by the whole wavefront,
// 64 probes a round, was measured in place of the lane's own binary search: DESIGN.md "LOO-PIT".)
__device__ __forceinline__ void loo_pit_rows(LooPitState& st, const LooPitDatum& D, const double* vrow,
                                             const double* lrow, int nrow, uint32_t k0) {
  for (int r = 0; r < nrow; r++) {
    const double v = vrow[r];
    double x = -lrow[r] - D.mx;
    if (D.smooth && x > D.cutoff) {
      const uint64_t key = psis_key(x);
      const uint32_t k = k0 + (uint32_t)r;
      int lo = 0, hi = D.T;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (psis_pair_less(D.keys[mid], D.idx[mid], key, k)) lo = mid + 1;
        else hi = mid;
      }
      if (lo < D.T) x = D.xs[lo];
    }
    x = fmin(x, 0.0);
    loo_pit_push(st, x, v < D.y, v == D.y);
  }
}

template <class Src>
__global__ __launch_bounds__(kPpBlock) void loo_pit_kernel(Src src, LooPitParams P) {
  extern __shared__ double ic_lds[];
  const int d = P.d, C = P.C, N = P.N;
  const int tid = threadIdx.x, nrow = pp_rows(C);
  const long long c = (long long)blockIdx.x * kPpBlock + tid;
  const bool live = c < C;
  double* const tile2 = pp_behind(ic_lds, d);                    // the replicates
  double* const tile3 = tile2 + (size_t)kPpBlock * kPpcStride;   // the terms
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
  // the block's slots of the per-datum states: [N][4]
  double* bst = P.state + (size_t)blockIdx.x * N * kLooPitFields;
  const uint32_t c0 = (uint32_t)blockIdx.x * kPpBlock;
  for (int s = 0; s < P.S; s++) {
    pp_stage(src, ic_lds, P.draws, s, d, C);
    typename Src::Datum dat{};
    for (int i0 = 0; i0 < N; i0 += kPpBlock) {
      const int ng = (N - i0 < kPpBlock) ? N - i0 : kPpBlock;   // datums of the group
      if (live) {
        for (int k = 0; k < ng; k++) {
          dat = pp_load(src, i0 + k, dat);
          // (the term before the stores: a store into the tiles may alias the parameter tile for all the
          // compiler knows, and the parameters of the datum's distribution would be evaluated twice)
          const double l = src.term(dat, q, cq);
          tile2[k * kPpcStride + tid] = pp_sample(src.params(dat, q, cq), g);
          tile3[k * kPpcStride + tid] = l;
        }
      }
      __syncthreads();
      if (tid < ng) {
        const int i = i0 + tid;
        double* slot = bst + (size_t)i * kLooPitFields;
        LooPitState st{-__builtin_inf(), 0.0, 0.0, 0.0};
        if (s > 0) st = LooPitState{slot[0], slot[1], slot[2], slot[3]};
        const LooPitDatum D = loo_pit_datum(P.tab, i, src.obs(i));
        loo_pit_rows(st, D, tile2 + tid * kPpcStride, tile3 + tid * kPpcStride, nrow,
                     (uint32_t)s * (uint32_t)C + c0);
        slot[0] = st.m;
        slot[1] = st.sA;
        slot[2] = st.sL;
        slot[3] = st.sQ;
      }
      __syncthreads();   // the group's tiles have been read
    }
  }
}

// grid (B, ceil(N / 64)), 64 lanes; LDS: the two tiles [64][65]
__global__ __launch_bounds__(kPpBlock) void loo_pit_ll_kernel(const double* __restrict__ ll,
                                                             const double* __restrict__ yrep,
                                                             const double* __restrict__ y, int S, int N, int C,
                                                             LooPitTables tab, double* __restrict__ state) {
  __shared__ double tile2[kPpBlock * kPpcStride];
  __shared__ double tile3[kPpBlock * kPpcStride];
  const int tid = threadIdx.x, nrow = pp_rows(C);
  const int i0 = blockIdx.y * kPpBlock;
  const int ng = (N - i0 < kPpBlock) ? N - i0 : kPpBlock;
  const uint32_t c0 = (uint32_t)blockIdx.x * kPpBlock;
  const bool live = tid < nrow, own = tid < ng;
  const int i = own ? i0 + tid : i0;
  LooPitState st{-__builtin_inf(), 0.0, 0.0, 0.0};
  const LooPitDatum D = loo_pit_datum(tab, i, y[i]);
  for (int s = 0; s < S; s++) {
    if (live) {
      const size_t base = ((size_t)s * N + i0) * C + c0 + tid;
      for (int k = 0; k < ng; k++) {
        tile2[k * kPpcStride + tid] = yrep[base + (size_t)k * C];
        tile3[k * kPpcStride + tid] = ll[base + (size_t)k * C];
      }
    }
    __syncthreads();
    if (own)
      loo_pit_rows(st, D, tile2 + tid * kPpcStride, tile3 + tid * kPpcStride, nrow, (uint32_t)s * (uint32_t)C + c0);
    __syncthreads();   // the tiles have been read
  }
  if (own) {
    double* slot = state + ((size_t)blockIdx.x * N + i) * kLooPitFields;
    slot[0] = st.m;
    slot[1] = st.sA;
    slot[2] = st.sL;
    slot[3] = st.sQ;
  }
}

// state [B][N][4] -> out [4][N]
__global__ __launch_bounds__(256) void loo_pit_merge_kernel(const double* __restrict__ state, int B, int N,
                                                           const double* __restrict__ meta,
                                                           double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const double* p = state + (size_t)i * kLooPitFields;
  LooPitState st{p[0], p[1], p[2], p[3]};
  for (int b = 1; b < B; b++) {
    const double* q = state + ((size_t)b * N + i) * kLooPitFields;
    loo_pit_merge(st, LooPitState{q[0], q[1], q[2], q[3]});
  }
  const double* mt = meta + (size_t)i * kPsisMeta;
  const double nan = exmc_from_bits(EXMC_NAN_BITS);
  const bool bad = mt[5] != 0.0;
  const double p_lt = st.sL / st.sA, p_eq = st.sQ / st.sA;
  out[i] = bad ? nan : p_lt;
  out[(size_t)N + i] = bad ? nan : p_eq;
  out[(size_t)2 * N + i] = bad ? nan : p_lt + 0.5 * p_eq;
  out[(size_t)3 * N + i] = bad ? nan : mt[3];
}

}  // namespace exmc
