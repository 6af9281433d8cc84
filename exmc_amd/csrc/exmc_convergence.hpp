// exmc_convergence.hpp -- the kernels of exmc_hip_convergence (include/exmc_hip_convergence.h states
// the arithmetic, DESIGN.md "Convergence diagnostics across chains" the design): rank-normalised and
// folded split R-hat, bulk / tail / mean ESS and the MCSE of the mean per dimension of a trace
// [S][D][C], with the ranks taken over the pooled draws of all chains. Included by exmc_common.hip
// alone, which launches them over a block of `nb` dimensions at a time.
//
// Per dimension, n = S / 2 draws in each of M = 2 C split chains, N = M n pooled values. The pooled
// element e = i M + h is draw i of column h = half C + c (lanes sweep chains first, as rhat_kernel
// phase 0 does, so loads coalesce); the contract's split chain is k = 2 c + half, and every sum over
// k runs in that order.
//   pooled_ess_nan_kernel       whether a dimension holds a NaN, per slice of the pool (one writer a word)
//   pooled_ess_fill_kernel      (key, e) pairs: the value, or fabs(x - med) for the fold; padded with
//                               (+inf, e >= N) to a power of two P
//   pooled_ess_sort_local_kernel, pooled_ess_sort_global_kernel
//                               a bitonic sort ascending by (key, e): tiles of kConvTile pairs in LDS,
//                               the stages at a distance of a tile or more in global memory. P <=
//                               kConvTile is one workgroup per dimension and one launch.
//   pooled_ess_runs_kernel      tie runs by head flags and a scan: phase 0 leaves each tile's first and
//                               last head, pooled_ess_carry_kernel carries them over the tiles, phase 1
//                               gives every position its run [a, b), the average rank
//                               a + 1 + (b - a - 1) / 2, the score, and scatters it to z[i][h]. A
//                               constant dimension costs what any other does.
//   pooled_ess_quantile_kernel  med, q05, q95 off the sorted keys
//   pooled_ess_moments_kernel   mean_k and var_k of the five derived series, one lane per split chain
//   pooled_ess_acov_kernel      sixteen lags of acov_k per sweep, one lane per (series, dimension, split
//                               chain), the register ring of exmc_ess.hpp; skipped once a series has
//                               its cut
//   pooled_ess_decide_kernel    A(t) over k left to right (a lane per lag), then Geyer's pairs in order
//   pooled_ess_finish_kernel    the two R-hats and the six outputs, one lane per dimension
#pragma once

#include "exmc_device.hpp"
#include "exmc_diag.hpp"

namespace exmc {

constexpr int kConvTile = 4096;        // pairs a workgroup sorts in LDS: 48 KB
constexpr int kConvBlock = 256;
constexpr int kConvRunTile = 4 * kConvBlock;   // positions of a workgroup of pooled_ess_runs_kernel
constexpr int kConvNanSlices = 64;
constexpr int kConvLags = 16;          // lags per sweep
// the derived series; the four with an ESS first
enum { kConvZ = 0, kConvI05 = 1, kConvI95 = 2, kConvX = 3, kConvZf = 4, kConvSeries = 5, kConvEss = 4 };

struct ConvState {   // one per (dimension, ESS series)
  double W, var_plus, tau, prev, ess;
  int done, pad;
};

struct ConvBlk {
  const double* draws;   // [S][D][C]
  int D, C, n, M, N;     // N = M n <= 2^31 - 1
  unsigned P;            // power of two >= N
  int dim0, nb;          // this block: dimensions dim0 .. dim0 + nb - 1
  int n_tiles;           // ceil(N / kConvRunTile)
  double* keys;          // [nb][P]
  unsigned* idx;         // [nb][P]
  double* z;             // [nb][n][M]
  double* zf;            // [nb][n][M]
  int* tile_first;       // [nb][n_tiles] first head of a tile, N: none
  int* tile_last;        // [nb][n_tiles] last head of a tile, -1: none
  int* carry_start;      // [nb][n_tiles] last head in front of a tile
  int* carry_end;        // [nb][n_tiles] first head behind a tile, N: none
  double* qs;            // [nb][3] med, q05, q95
  int* nanpart;          // [nb][kConvNanSlices]
  double* mom;           // [nb][kConvSeries][2][M] mean_k, var_k at k = 2 c + half
  double* acov;          // [nb][kConvEss][M][kConvLags]
  ConvState* state;      // [nb][kConvEss]
};

// column h of dimension b: the lane's strided view of one derived series
struct ConvLane {
  const double* p;
  size_t stride;
  double q;
  bool ind;
  __device__ __forceinline__ double at(int i) const {
    const double v = p[(size_t)i * stride];
    return ind ? ((v <= q) ? 1.0 : 0.0) : v;
  }
};

__device__ __forceinline__ const double* conv_xcol(const ConvBlk& g, int b, int h) {
  const int c = h % g.C, half = h / g.C;
  return g.draws + ((size_t)half * g.n * g.D + (size_t)(g.dim0 + b)) * g.C + c;
}

__device__ __forceinline__ ConvLane conv_lane(const ConvBlk& g, int series, int b, int h) {
  ConvLane l;
  if (series == kConvZ || series == kConvZf) {
    l.p = (series == kConvZ ? g.z : g.zf) + (size_t)b * g.N + h;
    l.stride = (size_t)g.M;
    l.q = 0.0;
    l.ind = false;
  } else {
    l.p = conv_xcol(g, b, h);
    l.stride = (size_t)g.D * g.C;
    l.ind = series != kConvX;
    l.q = l.ind ? g.qs[b * 3 + (series == kConvI05 ? 1 : 2)] : 0.0;
  }
  return l;
}

// pooled element e of dimension b
__device__ __forceinline__ double conv_pool(const ConvBlk& g, int b, unsigned e) {
  const int i = (int)(e / (unsigned)g.M), h = (int)(e % (unsigned)g.M);
  return conv_xcol(g, b, h)[(size_t)i * g.D * g.C];
}

__global__ void __launch_bounds__(kConvBlock) pooled_ess_nan_kernel(ConvBlk g)
{
  const int b = blockIdx.y;
  int bad = 0;
  for (size_t e = (size_t)blockIdx.x * kConvBlock + threadIdx.x; e < (size_t)g.N;
       e += (size_t)kConvNanSlices * kConvBlock) {
    const double v = conv_pool(g, b, (unsigned)e);
    bad |= (v != v) ? 1 : 0;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) g.nanpart[b * kConvNanSlices + blockIdx.x] = bad ? 1 : 0;
}

__global__ void __launch_bounds__(kConvBlock) pooled_ess_fill_kernel(ConvBlk g, int fold)
{
  const int b = blockIdx.y;
  const size_t p = (size_t)blockIdx.x * kConvBlock + threadIdx.x;
  if (p >= (size_t)g.P) return;
  double v = __longlong_as_double(0x7FF0000000000000LL);
  if (p < (size_t)g.N) {
    v = conv_pool(g, b, (unsigned)p);
    if (fold) v = fabs(v - g.qs[b * 3]);
  }
  g.keys[(size_t)b * g.P + p] = v;
  g.idx[(size_t)b * g.P + p] = (unsigned)p;
}

__device__ __forceinline__ bool conv_after(double ka, unsigned ia, double kb, unsigned ib) {
  return (ka > kb) || (ka == kb && ia > ib);
}

// the stages k = k_lo .. k_hi of the network at the distances j < T inside tiles of T pairs held in
// LDS (T = min(P, kConvTile)): k_lo = 2, k_hi = T sorts every tile; k_lo = k_hi = k > T finishes the
// merge step k once pooled_ess_sort_global_kernel has done its distances j >= T.
__global__ void __launch_bounds__(kConvBlock)
pooled_ess_sort_local_kernel(ConvBlk g, unsigned T, unsigned long long k_lo, unsigned long long k_hi)
{
  extern __shared__ double conv_lds[];       // T keys, then T indices
  unsigned* const li = (unsigned*)(conv_lds + T);
  const int b = blockIdx.y;
  const size_t base = (size_t)b * g.P + (size_t)blockIdx.x * T;
  const unsigned long long pos0 = (unsigned long long)blockIdx.x * T;
  for (unsigned i = threadIdx.x; i < T; i += kConvBlock) {
    conv_lds[i] = g.keys[base + i];
    li[i] = g.idx[base + i];
  }
  __syncthreads();
  for (unsigned long long k = k_lo; k <= k_hi; k <<= 1) {
    const unsigned j0 = (k >> 1) < (unsigned long long)(T >> 1) ? (unsigned)(k >> 1) : (T >> 1);
    for (unsigned j = j0; j > 0; j >>= 1) {
      for (unsigned t = threadIdx.x; t < (T >> 1); t += kConvBlock) {
        const unsigned a = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const unsigned c = a + j;
        const bool up = ((pos0 + a) & k) == 0;
        const double ka = conv_lds[a], kb = conv_lds[c];
        const unsigned ia = li[a], ib = li[c];
        if (conv_after(ka, ia, kb, ib) == up) {
          conv_lds[a] = kb; conv_lds[c] = ka;
          li[a] = ib; li[c] = ia;
        }
      }
      __syncthreads();
    }
  }
  for (unsigned i = threadIdx.x; i < T; i += kConvBlock) {
    g.keys[base + i] = conv_lds[i];
    g.idx[base + i] = li[i];
  }
}

// one compare-exchange per thread at distance j >= kConvTile of merge step k, in global memory
__global__ void __launch_bounds__(kConvBlock)
pooled_ess_sort_global_kernel(ConvBlk g, unsigned long long k, unsigned j)
{
  const int b = blockIdx.y;
  const unsigned t = blockIdx.x * kConvBlock + threadIdx.x;
  if (t >= (g.P >> 1)) return;
  const unsigned a = ((t & ~(j - 1)) << 1) | (t & (j - 1));
  const unsigned c = a + j;
  double* const K = g.keys + (size_t)b * g.P;
  unsigned* const I = g.idx + (size_t)b * g.P;
  const bool up = ((unsigned long long)a & k) == 0;
  const double ka = K[a], kb = K[c];
  const unsigned ia = I[a], ib = I[c];
  if (conv_after(ka, ia, kb, ib) == up) {
    K[a] = kb; K[c] = ka;
    I[a] = ib; I[c] = ia;
  }
}

// Tie runs of the sorted keys (the N real elements are the first N positions: a padding pair has
// e >= N and sorts behind every real +inf). A head is a position whose key differs (by !=) from its
// left neighbour's; position 0 is one. Thread t owns four positions; the last head at or before, and
// the first head behind, come from a max-scan and a min-scan over the workgroup's threads and, where
// a tile has none, from the carries. phase 0: the tile's first and last head. phase 1: the scores.
__global__ void __launch_bounds__(kConvBlock) pooled_ess_runs_kernel(ConvBlk g, int phase, double* out)
{
  __shared__ int sL[kConvBlock], sF[kConvBlock];
  const int b = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
  const int N = g.N;
  const double* const K = g.keys + (size_t)b * g.P;
  const unsigned* const I = g.idx + (size_t)b * g.P;
  const long long base = (long long)tile * kConvRunTile + 4 * t;
  double prev = (base > 0 && base < N) ? K[base - 1] : 0.0;
  bool head[4];
  int last[4];
  int L = -1, F = N;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const long long p = base + q;
    head[q] = false;
    if (p < N) {
      const double kv = K[p];
      head[q] = (p == 0) || (kv != prev);
      prev = kv;
      if (head[q]) {
        L = (int)p;
        if (F == N) F = (int)p;
      }
    }
    last[q] = L;
  }
  sL[t] = L;
  sF[t] = F;
  __syncthreads();
  for (int off = 1; off < kConvBlock; off <<= 1) {
    const int a = sL[t], c = (t >= off) ? sL[t - off] : -1;
    const int e = sF[t], f = (t + off < kConvBlock) ? sF[t + off] : N;
    __syncthreads();
    sL[t] = a > c ? a : c;
    sF[t] = e < f ? e : f;
    __syncthreads();
  }
  if (phase == 0) {
    if (t == 0) {
      g.tile_last[(size_t)b * g.n_tiles + tile] = sL[kConvBlock - 1];
      g.tile_first[(size_t)b * g.n_tiles + tile] = sF[0];
    }
    return;
  }
  int before = (t > 0) ? sL[t - 1] : -1;
  if (before < 0) before = g.carry_start[(size_t)b * g.n_tiles + tile];
  int nxt = (t + 1 < kConvBlock) ? sF[t + 1] : N;
  if (nxt == N) nxt = g.carry_end[(size_t)b * g.n_tiles + tile];
#pragma unroll
  for (int q = 3; q >= 0; q--) {
    const long long p = base + q;
    if (p < N) {
      const int lo = last[q] >= 0 ? last[q] : before;   // the run is [lo, nxt)
      const int eq = nxt - lo;
      const double avg = (double)(lo + 1) + (double)(eq - 1) / 2.0;
      const double pr = (avg - 0.375) / ((double)N + 0.25);
      const unsigned e = I[p];
      // a dimension with a NaN is not sorted (its outputs are NaN whatever is written here)
      if (e < (unsigned)N)
        out[(size_t)b * N + e] = (pr < 0.5) ? -probit_inner_dev(pr) : probit_inner_dev(1.0 - pr);
      if (head[q]) nxt = (int)p;
    }
  }
}

__global__ void __launch_bounds__(64) pooled_ess_carry_kernel(ConvBlk g)
{
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= g.nb) return;
  const size_t o = (size_t)b * g.n_tiles;
  int cur = -1;
  for (int t = 0; t < g.n_tiles; t++) {
    g.carry_start[o + t] = cur;
    const int l = g.tile_last[o + t];
    if (l >= 0) cur = l;
  }
  cur = g.N;
  for (int t = g.n_tiles - 1; t >= 0; t--) {
    g.carry_end[o + t] = cur;
    const int f = g.tile_first[o + t];
    if (f < g.N) cur = f;
  }
}

// Diagnostics.quantile (diagnostics.ex:170-180) of the sorted pool
__global__ void __launch_bounds__(64) pooled_ess_quantile_kernel(ConvBlk g)
{
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= g.nb) return;
  const double* const K = g.keys + (size_t)b * g.P;
  const double ps[3] = {0.5, 0.05, 0.95};
  for (int r = 0; r < 3; r++) {
    const double h = (double)(g.N - 1) * ps[r];
    const double lo = floor(h), hi = ceil(h);
    const double frac = h - lo;
    const double lo_val = K[(size_t)lo], hi_val = K[(size_t)hi];
    g.qs[b * 3 + r] = lo_val + frac * (hi_val - lo_val);
  }
}

__global__ void __launch_bounds__(kConvBlock) pooled_ess_moments_kernel(ConvBlk g)
{
  const int h = blockIdx.x * kConvBlock + threadIdx.x;
  const int b = blockIdx.y, series = blockIdx.z;
  if (h >= g.M) return;
  const ConvLane y = conv_lane(g, series, b, h);
  const int n = g.n;
  double sum = 0.0;
  for (int i = 0; i < n; i++) sum += y.at(i);
  const double mean = sum / n;
  double ss = 0.0;
  for (int i = 0; i < n; i++) {
    const double dv = y.at(i) - mean;
    ss += dv * dv;
  }
  const int k = 2 * (h % g.C) + h / g.C;
  double* const mo = g.mom + ((size_t)b * kConvSeries + series) * 2 * g.M;
  mo[k] = mean;
  mo[g.M + k] = ss / (n - 1);
}

// acov_k(l0 .. l0 + 15) of one split chain per lane: the sweep of exmc_ess.hpp (j = i + lag walks
// from l0 up, c[j - l0] enters a ring of sixteen registers, lag l0 + t multiplies c[j] with
// ring[(u - t) & 15]; ring entries for i < 0 are zeros and leave their sums unchanged), every sum
// left to right over i as `acc + c[i] * c[i + lag]`.
__global__ void __launch_bounds__(64) pooled_ess_acov_kernel(ConvBlk g, int l0)
{
  const int h = blockIdx.x * 64 + threadIdx.x;
  const int b = blockIdx.y, series = blockIdx.z;
  const int sd = b * kConvEss + series;
  if (h >= g.M || g.state[sd].done) return;
  const ConvLane y = conv_lane(g, series, b, h);
  const int n = g.n;
  const int k = 2 * (h % g.C) + h / g.C;
  const double mean = g.mom[((size_t)b * kConvSeries + series) * 2 * g.M + k];
  double acc[kConvLags], ring[kConvLags];
#pragma unroll
  for (int t = 0; t < kConvLags; t++) acc[t] = ring[t] = 0.0;
  for (int j0 = l0; j0 < n; j0 += kConvLags) {
    double xa[kConvLags], xb[kConvLags];
#pragma unroll
    for (int u = 0; u < kConvLags; u++) {
      const int j = (j0 + u < n) ? (j0 + u) : (n - 1);
      xa[u] = y.at(j);
    }
#pragma unroll
    for (int u = 0; u < kConvLags; u++) {
      const int j = (j0 + u < n) ? (j0 + u) : (n - 1);
      xb[u] = (l0 != 0) ? y.at(j - l0) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kConvLags; u++) {
      if (j0 + u < n) {
        const double cj = xa[u] - mean;
        ring[u] = (l0 == 0) ? cj : (xb[u] - mean);
#pragma unroll
        for (int t = 0; t < kConvLags; t++) acc[t] = acc[t] + ring[(u - t) & (kConvLags - 1)] * cj;
      }
    }
  }
  double* const o = g.acov + ((size_t)sd * g.M + k) * kConvLags;
#pragma unroll
  for (int t = 0; t < kConvLags; t++) o[t] = acc[t] / n;
}

// One workgroup per (dimension, ESS series) that has not met its cut: lane t < 16 sums acov_k(l0 + t)
// over k ascending; in the first block lane 16 sums W's terms and lane 17 forms gm and Bn; lane 0 then
// takes Geyer's pairs of this block in order.
__global__ void __launch_bounds__(64) pooled_ess_decide_kernel(ConvBlk g, int l0)
{
  __shared__ double sA[kConvLags], sW, sBn;
  const int sd = blockIdx.x, t = threadIdx.x;
  const int b = sd / kConvEss, series = sd % kConvEss;
  ConvState* const st = g.state + sd;
  if (st->done) return;
  const int n = g.n, M = g.M;
  const double* const ac = g.acov + (size_t)sd * M * kConvLags;
  if (t < kConvLags) {
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < M; k++) s += ac[(size_t)k * kConvLags + t];
    sA[t] = s / M;
  } else if (l0 == 0 && t == kConvLags) {
    double s = 0.0;
    for (int k = 0; k < M; k++) s += ac[(size_t)k * kConvLags] * n / (n - 1);
    sW = s / M;
  } else if (l0 == 0 && t == kConvLags + 1) {
    const double* const means = g.mom + ((size_t)b * kConvSeries + series) * 2 * M;
    double gm = 0.0;
    for (int k = 0; k < M; k++) gm += means[k];
    gm = gm / M;
    double bn = 0.0;
    for (int k = 0; k < M; k++) {
      const double dm = means[k] - gm;
      bn += dm * dm;
    }
    sBn = bn / (M - 1);
  }
  __syncthreads();
  if (t != 0) return;
  double W, var_plus, tau, prev;
  if (l0 == 0) {
    W = sW;
    var_plus = W * (n - 1) / n + sBn;
    tau = -1.0;
    prev = __longlong_as_double(0x7FF0000000000000LL);
    st->W = W;
    st->var_plus = var_plus;
    if (!(var_plus > 0)) {
      st->ess = __longlong_as_double(0x7FF8000000000000LL);
      st->done = 1;
      return;
    }
  } else {
    W = st->W; var_plus = st->var_plus; tau = st->tau; prev = st->prev;
  }
  bool cut = false;
  for (int jj = 0; jj < kConvLags / 2 && !cut; jj++) {
    const int j = l0 / 2 + jj;
    if (2 * j + 1 > n - 1) {
      cut = true;
    } else {
      const double r0 = (j == 0) ? 1.0 : 1.0 - (W - sA[2 * jj]) / var_plus;
      const double r1 = 1.0 - (W - sA[2 * jj + 1]) / var_plus;
      double P = r0 + r1;
      if (!(P > 0)) {
        cut = true;
      } else {
        P = (P < prev) ? P : prev;
        tau = tau + 2 * P;
        prev = P;
      }
    }
  }
  if (cut) {
    const double cap = exmc_log(10.0) / exmc_log((double)g.N);
    tau = (tau > cap) ? tau : cap;
    st->ess = (double)g.N / tau;
    st->done = 1;
  } else {
    st->tau = tau;
    st->prev = prev;
  }
}

// rhat_kernel phase 1's expressions over the M split chains of a derived series
__device__ __forceinline__ double conv_rhat(const double* means, int M, int n) {
  const double* const vars = means + M;
  double gm = 0.0;
  for (int k = 0; k < M; k++) gm += means[k];
  gm /= M;
  double bsum = 0.0, w = 0.0;
  for (int k = 0; k < M; k++) {
    const double dm = means[k] - gm;
    bsum += dm * dm;
    w += vars[k];
  }
  bsum = (double)n / (M - 1) * bsum;
  w /= M;
  const double var_hat = (double)(n - 1) / n * w + bsum / n;
  return __dsqrt_rn(var_hat / w);
}

// out [6][D], the columns dim0 .. dim0 + nb - 1
__global__ void __launch_bounds__(64) pooled_ess_finish_kernel(ConvBlk g, double* out)
{
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= g.nb) return;
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
  int bad = 0;
  for (int s = 0; s < kConvNanSlices; s++) bad |= g.nanpart[b * kConvNanSlices + s];
  double r[6];
  if (bad) {
    for (int i = 0; i < 6; i++) r[i] = nan;
  } else {
    const double* const mo = g.mom + (size_t)b * kConvSeries * 2 * g.M;
    const ConvState* const st = g.state + b * kConvEss;
    r[0] = conv_rhat(mo + (size_t)kConvZ * 2 * g.M, g.M, g.n);
    r[1] = conv_rhat(mo + (size_t)kConvZf * 2 * g.M, g.M, g.n);
    r[2] = st[kConvZ].ess;
    const double e05 = st[kConvI05].ess, e95 = st[kConvI95].ess;
    r[3] = (e05 != e05 || e95 != e95) ? nan : ((e05 < e95) ? e05 : e95);
    r[4] = st[kConvX].ess;
    r[5] = __dsqrt_rn(st[kConvX].var_plus / r[4]);
  }
  for (int i = 0; i < 6; i++) out[(size_t)i * g.D + g.dim0 + b] = r[i];
}

}  // namespace exmc
