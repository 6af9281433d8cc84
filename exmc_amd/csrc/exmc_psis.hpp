// exmc_psis.hpp -- Pareto-smoothed importance-sampling LOO with the Pareto k diagnostic per datum
// (Vehtari, Simpson, Gelman, Yao, Gabry; the generalised-Pareto fit of Zhang & Stephens 2009) over a
// device matrix ll[S][Nb][C]; DESIGN.md "PSIS-LOO" is the contract, include/exmc_hip_compare.h the
// C ABI, tests/host/psis_host_checker.c the host statement. r_eff = 1.
//
// Per datum, over the n = S C pooled samples k = s C + c, with lr = -ll and x = lr - max lr:
//   psis_tail_kernel, one workgroup per datum:
//     1. max lr, and whether every term is finite (if not, the datum's outputs are NaN);
//     2. the (M + 1)-th largest x, exactly, by a radix select on order-preserving 64-bit keys: six
//        histogram passes over the samples (five digits of 11 bits, one of 9), the histogram in LDS;
//        cutoff = max(that x, log DBL_MIN);
//     3. the tail {x > cutoff} (T <= M samples) compacted as (key, k) pairs and sorted ascending by
//        (x, k) -- a bitonic network over the next power of two, in LDS while the pairs fit
//        (kPsisLdsPairs), else in the datum's rows of the global table;
//     4. t_j = exp(x_(j)) - exp(cutoff) and the Zhang-Stephens fit: wave w takes the grid points
//        j = w, w + 16, ...; a tail sum is 64 lane sums (lane l adds the terms i = l, l + 64, ... in
//        that order, from 0.0) joined by the xor butterfly group_allsum<64>, i.e. adjacent pairs,
//        then pairs of pairs; the sums over the grid run left to right in one lane;
//     5. the T smoothed values log(G^-1((j - 1/2) / T) + exp(cutoff)) into the datum's table row.
//   psis_weights_kernel, one lane per datum and a chunk of samples per workgroup (ic_chunk, the
//     chunks of exmc_ic.hpp): every sample's x is min(x, 0), or min(table entry, 0) for a tail sample,
//     found by binary search of (key, k) in the sorted tail; x + ll, x and ll go into three online
//     log-sum-exps (ic_lse_push) in sample order.
//   psis_merge_kernel: chunk states left to right (ic_lse_merge), then elpd_loo, p_loo, k.
//
// Every transcendental is the general exmc_detmath.h function; sqrt and / are IEEE; build with
// -ffp-contract=off.
#pragma once

#include "exmc_ic.hpp"

namespace exmc {

#ifndef EXMC_ONLY_CUSTOM   // a generated model's plug-in carries no model-comparison kernels

constexpr int kPsisBlock = 1024;       // lanes of the per-datum workgroup (16 wavefronts)
constexpr int kPsisWaves = kPsisBlock / 64;
constexpr int kPsisDigit = 11;         // bits of a radix-select digit
constexpr int kPsisBins = 1 << kPsisDigit;
constexpr int kPsisLdsPairs = 8192;    // tail pairs one workgroup sorts in LDS: 12 B each, 96 KB
constexpr int kPsisFitMax = 448;       // grid points m = 30 + floor(sqrt T); T <= 3 sqrt(2^31) gives 402
constexpr int kPsisMeta = 6;           // per datum: max lr, cutoff, T, k, smoothed?, non-finite?
constexpr int kPsisFields = 6;         // chunk state: (m, s) of x + ll, of x, of ll
constexpr double kPsisLogMin = -0x1.6232bdd7abcd2p+9;   // log(DBL_MIN)

// M = ceil(min(n / 5, 3 sqrt n)): the most samples a tail holds
inline int psis_tail_len(long long n) {
  const double a = (double)n / 5.0, b = 3.0 * std::sqrt((double)n);
  return (int)std::ceil(a < b ? a : b);
}
inline int psis_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}
inline size_t psis_tail_lds_bytes(int P) { return (size_t)P * 12; }

// doubles in their order as unsigned integers (-0.0 below +0.0; no NaN reaches a key)
__device__ __forceinline__ uint64_t psis_key(double x) {
  const uint64_t u = exmc_to_bits(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ double psis_unkey(uint64_t k) {
  return exmc_from_bits((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k);
}
// a lane's walk over the samples k = tid, tid + kPsisBlock, ... of datum i: (s, c) advance by the
// quotient and the remainder of kPsisBlock / C, one division per pass instead of one per sample
struct PsisWalk {
  const double* p;   // ll + i C: element (s, c) is p[s Nb C + c]
  size_t row;        // Nb C
  unsigned s, c, ds, dc, C;
  __device__ PsisWalk(const double* ll, int Nb, int C_, int i, int tid)
      : p(ll + (size_t)i * C_), row((size_t)Nb * C_), s((unsigned)tid / (unsigned)C_),
        c((unsigned)tid % (unsigned)C_), ds(kPsisBlock / (unsigned)C_), dc(kPsisBlock % (unsigned)C_),
        C((unsigned)C_) {}
  __device__ double get() const { return p[(size_t)s * row + c]; }
  __device__ void next() {
    s += ds;
    c += dc;
    if (c >= C) {
      c -= C;
      s++;
    }
  }
};
__device__ __forceinline__ bool psis_pair_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// sum of log1p(-b t_i) over the tail in the contract's order; every lane of the wavefront calls it
__device__ __forceinline__ double psis_tail_sum(const double* t, int T, double b, int lane) {
  double acc = 0.0;
  for (int i = lane; i < T; i += 64) acc = acc + exmc_log1p(-b * t[i]);
  return group_allsum<64>(acc);
}

// kLds: the pairs (and then t) live in dynamic LDS, keys [P] then indices [P]; else in the datum's
// table rows, t in its row of tab_xs. P is a power of two >= M, the row length of the tables.
// kRatio (exmc_psis_ratio.hpp): `ll` holds log ratios lr themselves, read as ll = -lr. A ratio of -inf
// is admitted -- it counts in n, x = -inf lies below every cutoff and never enters the tail -- and a
// group with a NaN or +inf ratio, or without a finite one, is the one whose outputs are NaN.
template <bool kLds, bool kRatio = false>
__global__ __launch_bounds__(kPsisBlock) void psis_tail_kernel(const double* __restrict__ ll, int S, int Nb, int C,
                                                              int M, int P, uint64_t* __restrict__ tab_keys,
                                                              uint32_t* __restrict__ tab_idx,
                                                              double* __restrict__ tab_xs,
                                                              double* __restrict__ meta) {
  extern __shared__ double psis_lds[];   // keys [P] (8 B each), then indices [P]
  __shared__ unsigned hist[kPsisBins];
  __shared__ unsigned part[64];
  __shared__ double red[kPsisWaves];
  __shared__ int redi[kPsisWaves];
  __shared__ double fit_b[kPsisFitMax], fit_L[kPsisFitMax], fit_w[kPsisFitMax];
  __shared__ unsigned long long sel_prefix;
  __shared__ unsigned sel_rank, tail_cnt;
  __shared__ double fit_bhat;

  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned n = (unsigned)S * (unsigned)C;
  uint64_t* keys = kLds ? (uint64_t*)psis_lds : tab_keys + (size_t)i * P;
  uint32_t* idx = kLds ? (uint32_t*)(psis_lds + P) : tab_idx + (size_t)i * P;
  double* mt = meta + (size_t)i * kPsisMeta;

  // 1. max lr; any non-finite term
  double mx = -__builtin_inf();
  int bad = 0;
  PsisWalk w0(ll, Nb, C, i, tid);
  for (unsigned k = tid; k < n; k += kPsisBlock, w0.next()) {
    const double v = kRatio ? -w0.get() : w0.get();
    if (kRatio ? (!(v == v) || v == -__builtin_inf()) : !exmc_isfinite(v)) bad = 1;
    mx = fmax(mx, -v);
  }
  for (int o = 32; o >= 1; o >>= 1) {
    mx = fmax(mx, __shfl_xor(mx, o));
    bad |= __shfl_xor(bad, o);
  }
  if (lane == 0) {
    red[wave] = mx;
    redi[wave] = bad;
  }
  if (tid == 0) {
    sel_prefix = 0;
    sel_rank = (unsigned)M + 1u;
    tail_cnt = 0;
  }
  __syncthreads();
  for (int w = 0; w < kPsisWaves; w++) {
    mx = fmax(mx, red[w]);
    bad |= redi[w];
  }
  if (kRatio && mx == -__builtin_inf()) bad = 1;   // no finite ratio
  if (bad) {
    if (tid == 0) {
      mt[0] = mx; mt[1] = 0.0; mt[2] = 0.0; mt[3] = exmc_from_bits(EXMC_NAN_BITS); mt[4] = 0.0; mt[5] = 1.0;
    }
    return;
  }

  // 2. the (M + 1)-th largest key: digit by digit from the top
  for (int done = 0; done < 64;) {
    const int w = (64 - done >= kPsisDigit) ? kPsisDigit : 64 - done;
    const int shift = 64 - done - w, nb = 1 << w;
    for (int b = tid; b < nb; b += kPsisBlock) hist[b] = 0;
    __syncthreads();
    const unsigned long long prefix = sel_prefix;
    PsisWalk wk(ll, Nb, C, i, tid);
    for (unsigned k = tid; k < n; k += kPsisBlock, wk.next()) {
      const uint64_t key = psis_key((kRatio ? wk.get() : -wk.get()) - mx);
      if (done == 0 || (key >> (shift + w)) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & (nb - 1)], 1u);
    }
    __syncthreads();
    const int per = nb / 64;   // lane g of the first wave sums bins [g per, (g + 1) per)
    if (tid < 64) {
      unsigned s = 0;
      for (int b = 0; b < per; b++) s += hist[tid * per + b];
      part[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
      unsigned r = sel_rank;
      int g = 63;
      while (g > 0 && part[g] < r) r -= part[g--];
      int b = g * per + per - 1;
      while (b > g * per && hist[b] < r) r -= hist[b--];
      sel_prefix = (prefix << w) | (unsigned long long)b;
      sel_rank = r;
    }
    __syncthreads();
    done += w;
  }
  const double cutoff = fmax(psis_unkey(sel_prefix), kPsisLogMin);

  // 3. the tail, compacted and sorted by (x, k)
  PsisWalk wt(ll, Nb, C, i, tid);
  for (unsigned k = tid; k < n; k += kPsisBlock, wt.next()) {
    const double x = (kRatio ? wt.get() : -wt.get()) - mx;
    if (x > cutoff) {
      const unsigned pos = atomicAdd(&tail_cnt, 1u);
      if (pos < (unsigned)P) {
        keys[pos] = psis_key(x);
        idx[pos] = k;
      }
    }
  }
  __syncthreads();
  const int T = (int)tail_cnt;   // <= M: a value equal to the (M + 1)-th largest is not in the tail
  int Pt = 1;
  while (Pt < T) Pt <<= 1;
  for (int j = T + tid; j < Pt; j += kPsisBlock) {
    keys[j] = ~0ULL;
    idx[j] = ~0u;
  }
  for (int size = 2; size <= Pt; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < Pt / 2; t += kPsisBlock) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const uint64_t ka = keys[lo], kb = keys[hi];
        const uint32_t ia = idx[lo], ib = idx[hi];
        const bool up = (lo & size) == 0;
        if (psis_pair_less(kb, ib, ka, ia) == up) {
          keys[lo] = kb; idx[lo] = ib;
          keys[hi] = ka; idx[hi] = ia;
        }
      }
    }
  __syncthreads();
  if (T <= 4) {   // nothing to fit: no smoothing, k = +inf
    if (tid == 0) {
      mt[0] = mx; mt[1] = cutoff; mt[2] = (double)T; mt[3] = __builtin_inf(); mt[4] = 0.0; mt[5] = 0.0;
    }
    return;
  }

  // 4. t_j (over the keys in LDS; in the datum's tab_xs row otherwise) and the fit
  const double ec = exmc_exp(cutoff);
  double* t = kLds ? (double*)keys : tab_xs + (size_t)i * P;
  for (int j = tid; j < T; j += kPsisBlock) {
    const uint64_t key = keys[j];
    if (kLds) {
      tab_keys[(size_t)i * P + j] = key;
      tab_idx[(size_t)i * P + j] = idx[j];
    }
    t[j] = exmc_exp(psis_unkey(key)) - ec;
  }
  __syncthreads();
  const double dT = (double)T;
  const int m = 30 + (int)__dsqrt_rn(dT);
  const double tT = t[T - 1], tq = t[(int)(dT / 4.0 + 0.5) - 1];
  for (int j = wave; j < m; j += kPsisWaves) {
    const double bj = 1.0 / tT + (1.0 - __dsqrt_rn((double)m / ((double)(j + 1) - 0.5))) / (3.0 * tq);
    const double kap = psis_tail_sum(t, T, bj, lane) / dT;
    if (lane == 0) {
      fit_b[j] = bj;
      fit_L[j] = dT * ((exmc_log(-bj / kap) - kap) - 1.0);
    }
  }
  __syncthreads();
  if (tid < m) {
    double s = 0.0;
    for (int q = 0; q < m; q++) s = s + exmc_exp(fit_L[q] - fit_L[tid]);
    const double w = 1.0 / s;
    fit_w[tid] = (w < 10.0 * 0x1p-52) ? 0.0 : w;
  }
  __syncthreads();
  if (tid == 0) {
    double W = 0.0, b = 0.0;
    for (int j = 0; j < m; j++) W = W + fit_w[j];
    for (int j = 0; j < m; j++) b = b + (fit_w[j] / W) * fit_b[j];
    fit_bhat = b;
  }
  __syncthreads();
  const double bh = fit_bhat;
  const double kap = psis_tail_sum(t, T, bh, lane) / dT;   // every wave forms it: the same bits
  const double sigma = -kap / bh;
  double khat = (dT * kap + 10.0 * 0.5) / (dT + 10.0);
  if (!(khat == khat)) khat = exmc_from_bits(EXMC_NAN_BITS);
  const bool smooth = exmc_isfinite(khat);
  __syncthreads();   // t has been read: its slots may take the smoothed values

  // 5. the smoothed tail
  if (smooth) {
    double* xs = tab_xs + (size_t)i * P;
    for (int j = tid; j < T; j += kPsisBlock) {
      const double p = ((double)(j + 1) - 0.5) / dT;
      const double lq = exmc_log1p(-p);
      const double g = (khat == 0.0) ? -sigma * lq : (sigma * exmc_expm1(-khat * lq)) / khat;
      xs[j] = exmc_log(g + ec);
    }
  }
  if (tid == 0) {
    mt[0] = mx; mt[1] = cutoff; mt[2] = dT; mt[3] = khat; mt[4] = smooth ? 1.0 : 0.0; mt[5] = 0.0;
  }
}

// chunk partials part[chunk][kPsisFields][Nb]
__global__ __launch_bounds__(kIcBlock) void psis_weights_kernel(const double* __restrict__ ll, int S, int Nb, int C,
                                                               long long chunk, int P,
                                                               const uint64_t* __restrict__ tab_keys,
                                                               const uint32_t* __restrict__ tab_idx,
                                                               const double* __restrict__ tab_xs,
                                                               const double* __restrict__ meta,
                                                               double* __restrict__ part) {
  const int i = blockIdx.y * blockDim.x + threadIdx.x;
  if (i >= Nb) return;
  const long long n = (long long)S * C;
  const long long k0 = (long long)blockIdx.x * chunk;
  const long long k1 = (k0 + chunk < n) ? k0 + chunk : n;
  const double* mt = meta + (size_t)i * kPsisMeta;
  const double mx = mt[0], cutoff = mt[1];
  const int T = (int)mt[2];
  const bool smooth = mt[4] != 0.0;
  const uint64_t* keys = tab_keys + (size_t)i * P;
  const uint32_t* idx = tab_idx + (size_t)i * P;
  const double* xs = tab_xs + (size_t)i * P;
  double st[kPsisFields] = {-__builtin_inf(), 0.0, -__builtin_inf(), 0.0, -__builtin_inf(), 0.0};
  long long s = k0 / C;
  int c = (int)(k0 - s * C);
  for (long long k = k0; k < k1; k++) {
    const double v = ll[((size_t)s * Nb + i) * C + c];
    double x = -v - mx;
    if (smooth && x > cutoff) {
      const uint64_t key = psis_key(x);
      int lo = 0, hi = T;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (psis_pair_less(keys[mid], idx[mid], key, (uint32_t)k)) lo = mid + 1;
        else hi = mid;
      }
      if (lo < T) x = xs[lo];
    }
    x = fmin(x, 0.0);
    ic_lse_push(x + v, st[0], st[1]);
    ic_lse_push(x, st[2], st[3]);
    ic_lse_push(v, st[4], st[5]);
    if (++c == C) {
      c = 0;
      s++;
    }
  }
  double* p = part + (size_t)blockIdx.x * kPsisFields * Nb + i;
#pragma unroll
  for (int f = 0; f < kPsisFields; f++) p[(size_t)f * Nb] = st[f];
}

// out[3][N], this block's datums at i0 ..: elpd_loo = lse(x + ll) - lse(x), p_loo = lppd - elpd_loo with
// lppd as ic_merge_kernel forms it, k
__global__ __launch_bounds__(256) void psis_merge_kernel(const double* __restrict__ part, int n_chunks, long long n,
                                                        int Nb, const double* __restrict__ meta, int N, int i0,
                                                        double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Nb) return;
  const double* p = part + i;
  double st[kPsisFields];
#pragma unroll
  for (int f = 0; f < kPsisFields; f++) st[f] = p[(size_t)f * Nb];
  for (int b = 1; b < n_chunks; b++) {
    const double* q = part + (size_t)b * kPsisFields * Nb + i;
#pragma unroll
    for (int f = 0; f < kPsisFields; f += 2) ic_lse_merge(st[f], st[f + 1], q[(size_t)f * Nb], q[(size_t)(f + 1) * Nb]);
  }
  const double* mt = meta + (size_t)i * kPsisMeta;
  const double nan = exmc_from_bits(EXMC_NAN_BITS);
  const bool bad = mt[5] != 0.0;
  const double lppd = (st[4] + exmc_log(st[5])) - exmc_log((double)n);
  const double elpd = (st[0] + exmc_log(st[1])) - (st[2] + exmc_log(st[3]));
  out[(size_t)i0 + i] = bad ? nan : elpd;
  out[(size_t)N + i0 + i] = bad ? nan : lppd - elpd;
  out[(size_t)2 * N + i0 + i] = bad ? nan : mt[3];
}

#endif

}  // namespace exmc
