// exmc_psis_ratio.hpp -- Pareto-smoothed importance sampling over a device array of log importance
// ratios lr, with the per-sample weights kept, and systematic resampling from them. Model-free;
// DESIGN.md "Importance diagnostics of the fits" is the contract, include/exmc_hip_fit_psis.h the C
// ABI, tests/host/fit_psis_host_checker.c the host statement.
//
// A group is the set of samples smoothed together, expressed through the (S, Nb, C) walk of
// exmc_psis.hpp: element (s, i, c) of lr is lr[(s Nb + i) C + c], group i holds the n = S C samples
// k = s C + c. Per fit: Nb = n_fits, C = 1. Pooled: Nb = 1, C = n_fits.
//
//   psis_tail_kernel<kLds, true>   the tail of x = lr - max lr, the fit, the smoothed tail
//   ratio_weights_kernel           every sample's smoothed x_k = min(x or its table entry, 0) into xs
//                                  (the layout of lr); per chunk of ic_chunk(n) samples, in sample order,
//                                  the online log-sum-exps of x and of 2 x and the count of -inf ratios
//   ratio_merge_kernel             chunk states left to right; L1 = lse(x), L2 = lse(2 x); out[5][Nb] =
//                                  khat, (max lr + L1) - log n, exp(2 L1 - L2), n_zero, T; L1 (NaN for
//                                  a NaN group) into l1[Nb]
//   ratio_normalise_kernel         lw_k = x_k - L1 in place, NaN in a NaN group
//   ratio_scan_kernel              w_k = exp(lw_k) (or lw_k itself with `linear`: the caller's array holds
//                                  the weights, exmc_smc.hpp); one lane per block of kRatioScan consecutive samples
//                                  of a group: r_k = the running sum inside the block, left to right
//                                  from 0.0, into r (the layout of lr); the block's total into tot[b][Nb]
//   ratio_resample_kernel          one workgroup per group g: base_b = the earlier blocks' totals left to
//                                  right from 0.0; u = the first rng_uniform of a generator seeded with
//                                  seed + 7919 g; pos_j = (u + j) / R; idx_j = the first k with
//                                  base_b + r_k >= pos_j (binary search over the blocks, then inside the
//                                  block), n - 1 if there is none, -1 in a NaN group
//   ratio_gather_kernel            out[j][r][g] = the draw idx[j][g] of the group, NaN where idx < 0
// ratio_bases and ratio_search are the two steps of the resampling as device functions: the tempered
// SMC (exmc_smc.hpp) searches the same cumulative sums with positions of its own.
// Every output word has one writer; no atomics outside the tail kernel's LDS histogram.
#pragma once

#include "exmc_psis.hpp"

namespace exmc {

#ifndef EXMC_ONLY_CUSTOM

constexpr int kRatioFields = 5;      // chunk state: (m, s) of x, (m, s) of 2 x, the count of -inf ratios
constexpr int kRatioOut = 5;         // khat, log_mean_ratio, ess, n_zero, T
constexpr int kRatioScan = 4096;     // samples per block of the cumulative sum
constexpr int kRatioBlock = 256;     // lanes of the resampling workgroup

// part[chunk][kRatioFields][Nb]; xs, if given, takes every sample's smoothed x
__global__ __launch_bounds__(kIcBlock) void ratio_weights_kernel(const double* __restrict__ lr, int S, int Nb, int C,
                                                                long long chunk, int P,
                                                                const uint64_t* __restrict__ tab_keys,
                                                                const uint32_t* __restrict__ tab_idx,
                                                                const double* __restrict__ tab_xs,
                                                                const double* __restrict__ meta,
                                                                double* __restrict__ part, double* __restrict__ xs_out) {
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
  double st[kRatioFields] = {-__builtin_inf(), 0.0, -__builtin_inf(), 0.0, 0.0};
  long long s = k0 / C;
  int c = (int)(k0 - s * C);
  for (long long k = k0; k < k1; k++) {
    const size_t at = ((size_t)s * Nb + i) * C + c;
    const double v = lr[at];
    double x = v - mx;
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
    ic_lse_push(x, st[0], st[1]);
    ic_lse_push(2.0 * x, st[2], st[3]);
    st[4] = st[4] + ((v == -__builtin_inf()) ? 1.0 : 0.0);
    if (xs_out) xs_out[at] = x;
    if (++c == C) {
      c = 0;
      s++;
    }
  }
  double* p = part + (size_t)blockIdx.x * kRatioFields * Nb + i;
#pragma unroll
  for (int f = 0; f < kRatioFields; f++) p[(size_t)f * Nb] = st[f];
}

__global__ __launch_bounds__(256) void ratio_merge_kernel(const double* __restrict__ part, int n_chunks, long long n,
                                                         int Nb, const double* __restrict__ meta,
                                                         double* __restrict__ out, double* __restrict__ l1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Nb) return;
  const double* p = part + i;
  double st[kRatioFields];
#pragma unroll
  for (int f = 0; f < kRatioFields; f++) st[f] = p[(size_t)f * Nb];
  for (int b = 1; b < n_chunks; b++) {
    const double* q = part + (size_t)b * kRatioFields * Nb + i;
    ic_lse_merge(st[0], st[1], q[0], q[(size_t)Nb]);
    ic_lse_merge(st[2], st[3], q[(size_t)2 * Nb], q[(size_t)3 * Nb]);
    st[4] = st[4] + q[(size_t)4 * Nb];
  }
  const double* mt = meta + (size_t)i * kPsisMeta;
  const double nan = exmc_from_bits(EXMC_NAN_BITS);
  const bool bad = mt[5] != 0.0;
  const double L1 = st[0] + exmc_log(st[1]), L2 = st[2] + exmc_log(st[3]);
  out[i] = bad ? nan : mt[3];
  out[(size_t)Nb + i] = bad ? nan : (mt[0] + L1) - exmc_log((double)n);
  out[(size_t)2 * Nb + i] = bad ? nan : exmc_exp(2.0 * L1 - L2);
  out[(size_t)3 * Nb + i] = bad ? nan : st[4];
  out[(size_t)4 * Nb + i] = bad ? nan : mt[2];
  l1[i] = bad ? nan : L1;
}

// lw [S][Nb][C] holds the smoothed x on entry
__global__ __launch_bounds__(256) void ratio_normalise_kernel(double* __restrict__ lw, long long total, int Nb, int C,
                                                             const double* __restrict__ l1) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int i = (int)((e / C) % Nb);
  const double L = l1[i];
  lw[e] = (L == L) ? lw[e] - L : exmc_from_bits(EXMC_NAN_BITS);
}

// lane t: group t % Nb, block t / Nb
__global__ __launch_bounds__(256) void ratio_scan_kernel(const double* __restrict__ lw, int S, int Nb, int C,
                                                        int n_blocks, int linear, double* __restrict__ r_out,
                                                        double* __restrict__ tot) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)Nb * n_blocks) return;
  const int i = (int)(t % Nb), b = (int)(t / Nb);
  const long long n = (long long)S * C;
  const long long k0 = (long long)b * kRatioScan;
  const long long k1 = (k0 + kRatioScan < n) ? k0 + kRatioScan : n;
  long long s = k0 / C;
  int c = (int)(k0 - s * C);
  double r = 0.0;
  for (long long k = k0; k < k1; k++) {
    const size_t at = ((size_t)s * Nb + i) * C + c;
    r = r + (linear ? lw[at] : exmc_exp(lw[at]));
    r_out[at] = r;
    if (++c == C) {
      c = 0;
      s++;
    }
  }
  tot[(size_t)b * Nb + i] = r;
}

// bs[b] = the totals of the blocks before b of group i, left to right from 0.0; one lane writes them
__device__ inline void ratio_bases(const double* __restrict__ tot, double* __restrict__ bs, int n_blocks, int Nb,
                                   int i) {
  double acc = 0.0;
  bs[0] = acc;
  for (int b = 0; b < n_blocks; b++) {
    acc = acc + tot[(size_t)b * Nb + i];
    bs[b + 1] = acc;
  }
}

// the first sample k of group i with bs[block of k] + r_k >= pos (binary search over the blocks, then
// inside the block), n - 1 if there is none
__device__ inline long long ratio_search(const double* __restrict__ r, const double* __restrict__ bs, double pos,
                                         long long n, int n_blocks, int Nb, int C, int i) {
  int lo = 0, hi = n_blocks;   // the first block whose last cumulative value reaches pos
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (bs[mid + 1] >= pos) hi = mid;
    else lo = mid + 1;
  }
  long long pick = n - 1;
  if (lo < n_blocks) {
    const double b0 = bs[lo];
    long long ka = (long long)lo * kRatioScan;
    long long kb = (ka + kRatioScan < n) ? ka + kRatioScan : n;
    const long long kend = kb;
    while (ka < kb) {
      const long long mid = (ka + kb) >> 1;
      const long long s = mid / C;
      const int c = (int)(mid - s * C);
      if (b0 + r[((size_t)s * Nb + i) * C + c] >= pos) kb = mid;
      else ka = mid + 1;
    }
    pick = (ka < kend) ? ka : kend - 1;
  }
  return pick;
}

// base [Nb][n_blocks + 1] is scratch of the launch; idx [R][Nb]
__global__ __launch_bounds__(kRatioBlock) void ratio_resample_kernel(const double* __restrict__ r, const double* __restrict__ tot,
                                                                    double* __restrict__ base, int S, int Nb, int C,
                                                                    int n_blocks, int R, uint64_t seed,
                                                                    const double* __restrict__ l1,
                                                                    int32_t* __restrict__ idx) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const long long n = (long long)S * C;
  const double L = l1[i];
  if (!(L == L)) {
    for (int j = tid; j < R; j += kRatioBlock) idx[(size_t)j * Nb + i] = -1;
    return;
  }
  double* bs = base + (size_t)i * ((size_t)n_blocks + 1);
  if (tid == 0) ratio_bases(tot, bs, n_blocks, Nb, i);
  __syncthreads();
  Rng rng;
  rng_seed(rng, seed + 7919ULL * (uint64_t)i);
  const double u = rng_uniform(rng);
  for (int j = tid; j < R; j += kRatioBlock) {
    const double pos = (u + (double)j) / (double)R;
    idx[(size_t)j * Nb + i] = (int32_t)ratio_search(r, bs, pos, n, n_blocks, Nb, C, i);
  }
}

// draws [S][d][F]; idx [R][G] with G = 1 (pooled: k = s F + c) or G = F (per fit: k = s, c = g); out [R][d][G]
__global__ __launch_bounds__(256) void ratio_gather_kernel(const double* __restrict__ draws, const int32_t* __restrict__ idx,
                                                          int S, int d, int F, int pooled, int R,
                                                          double* __restrict__ out) {
  const int G = pooled ? 1 : F;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)R * d * G) return;
  const int g = (int)(e % G), dim = (int)((e / G) % d);
  const long long j = e / ((long long)G * d);
  const long long k = idx[(size_t)j * G + g];
  const long long n = pooled ? (long long)S * F : (long long)S;
  double v = exmc_from_bits(EXMC_NAN_BITS);
  if (k >= 0 && k < n) {
    const long long s = pooled ? k / F : k;
    const int c = pooled ? (int)(k - s * F) : g;
    v = draws[((size_t)s * d + dim) * F + c];
  }
  out[e] = v;
}

#endif

}  // namespace exmc
