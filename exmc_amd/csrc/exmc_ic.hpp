// exmc_ic.hpp -- model comparison on the device: per-datum log-likelihoods of the built-in kinds and
// their WAIC / IS-LOO statistics (Exmc.ModelComparison, lib/exmc/model_comparison.ex; DESIGN.md
// "Model comparison"; C ABI include/exmc_hip_compare.h).
//
// One lane owns one datum i; a workgroup of up to kIcBlock lanes owns a block of consecutive datums
// (grid.y) and a chunk of samples (grid.x). Samples are the pooled (draw, chain) pairs of a trace
// [S][d][C] in draw-major, chain-minor order, k = s C + c. A chunk is kIcChunk(S C) consecutive
// samples, a function of S and C only. The workgroup walks its chunk in tiles of kIcTile samples:
//   1. stage: the tile's parameters into LDS, [t][d] (coalesced over chains);
//   2. per-sample constants, one thread per sample (Src::consts), then in-place rewrites of the
//      tile that several datums share (Src::prepare: radon's county intercepts, sv_ncp's walk as a
//      wave scan with lane = t);
//   3. every lane walks the tile in sample order: ll = Src::term(...), pushed into its datum's
//      online state (ic_push) or written to the matrix ll[S][N][C].
// ic_merge_kernel merges the chunk states left to right, one lane per datum, in a second launch
// (workgroups of one launch never talk to each other).
//
// Every term uses the general exmc_detmath.h functions and tests/host/ic_host_checker.c restates it;
// build with -ffp-contract=off (fma only where written).
#pragma once

#include "../../include/exmc_detmath.h"

namespace exmc {

constexpr int kIcBlock = 512;          // datums per workgroup (8 wavefronts)
constexpr int kIcTile = 64;            // samples per LDS tile
constexpr int kIcTargetChunks = 1024;  // chunks the samples are cut into (at most)
constexpr int kIcConsts = 4;           // per-sample constants of a tile row (after the 1/k slot)
constexpr int kIcFields = 6;           // online state: max / sum of exp for +ll and -ll, mean, M2

// samples per chunk: a multiple of the tile, from the sample count alone
__host__ __device__ inline long long ic_chunk(long long n) {
  const long long per = (long long)kIcTile * kIcTargetChunks;
  return (long long)kIcTile * ((n + per - 1) / per);
}

__device__ __forceinline__ double ic_clamp200(double z) { return fmax(-200.0, fmin(z, 200.0)); }

// ---- the online state of one datum over one chunk -------------------------------------------------
// log-sum-exp: m = running max, s = sum of exp(x - m). A -inf term adds nothing (a leading one
// leaves m = -inf, s = 0: nothing is rescaled by exp(-inf - -inf)); x == m adds exactly 1 (so two
// +inf terms add 1 each); a NaN term makes m and s NaN, and they stay NaN.
__device__ __forceinline__ void ic_lse_push(double x, double& m, double& s) {
  if (!(x == x)) {
    m = x;
    s = x;
  } else if (x == -__builtin_inf()) {
  } else if (x > m) {
    s = s * exmc_exp(m - x) + 1.0;
    m = x;
  } else if (x == m) {
    s = s + 1.0;
  } else {
    s = s + exmc_exp(x - m);
  }
}
// Welford with the reciprocal of the sample's position in the chunk, rk = 1.0 / k (a per-sample
// constant): mean += (x - mean) * rk; M2 += delta * (x - mean_new)
__device__ __forceinline__ void ic_push(double x, double rk, double (&st)[kIcFields]) {
  ic_lse_push(x, st[0], st[1]);
  ic_lse_push(-x, st[2], st[3]);
  const double delta = x - st[4];
  st[4] = st[4] + delta * rk;
  st[5] = st[5] + delta * (x - st[4]);
}
__device__ __forceinline__ void ic_lse_merge(double& m, double& s, double m2, double s2) {
  if (!(m == m) || !(m2 == m2)) {
    const double nan = __builtin_nan("");
    m = nan;
    s = nan;
  } else if (m2 == -__builtin_inf()) {
  } else if (m == -__builtin_inf()) {
    m = m2;
    s = s2;
  } else if (m == m2) {
    s = s + s2;
  } else if (m > m2) {
    s = s + s2 * exmc_exp(m2 - m);
  } else {
    s = s * exmc_exp(m - m2) + s2;
    m = m2;
  }
}

// ---- the likelihood families of the kinds: what params() of a source returns ---------------------
// (the parameters of the datum's distribution at a sample: term() takes its ll from them, and
// exmc_predictive.hpp draws the datum's replicate from them)
struct NormalParams { double loc, scale; };
struct BernoulliParams { double p; };            // unclipped
struct StudentTParams { double df, loc, scale; };

// ---- sources of ll: one struct per kind --------------------------------------------------------
// consts(q, c): sample t's constants from its parameter row q (one thread per sample);
// prepare(...): in-place rewrites of the tile (cooperative; may be empty);
// Datum: what a lane keeps of its datum; load(i) fills it; params(dat, q, c) = the parameters of the
// datum's distribution at the sample; term(dat, q, c) = ll_i at the sample; obs(i) = the observed value
// of datum i alone (the Datum's y or r: what exmc_ppc.hpp holds the replicates against).
struct IcSimpleSrc {
  static constexpr bool kStaged = true;
  const double* y;   // dev [N]
  double log2pi32, tiny32;
  struct Datum { double y; };
  __device__ Datum load(int i) const { return {y[i]}; }
  __device__ double obs(int i) const { return y[i]; }
  __device__ void consts(const double* q, double* c) const {
    const double sigma = exmc_exp(ic_clamp200(q[1]));
    const double ss = fmax(sigma, tiny32);
    c[0] = q[0];
    c[1] = ss;
    c[2] = log2pi32 + 2.0 * exmc_log(ss);
  }
  __device__ void prepare(double*, const double*, int, int, int, int) const {}
  __device__ NormalParams params(const Datum&, const double*, const double* c) const { return {c[0], c[1]}; }
  __device__ double term(const Datum& a, const double* q, const double* c) const {
    const NormalParams p = params(a, q, c);
    const double z = (a.y - p.loc) / p.scale;
    return -0.5 * (z * z + c[2]);
  }
};

struct IcEightSchoolsSrc {
  static constexpr bool kStaged = true;
  const double* ys;   // dev [16]: y[8], sigma[8]
  double log2pi32;
  struct Datum { double y, sg, cn; int j; };
  __device__ Datum load(int i) const {
    const double sg = ys[8 + i];
    return {ys[i], sg, log2pi32 + 2.0 * exmc_log(sg), i};
  }
  __device__ double obs(int i) const { return ys[i]; }
  __device__ void consts(const double* q, double* c) const {
    c[0] = q[0];
    c[1] = exmc_exp(ic_clamp200(q[1]));
  }
  __device__ void prepare(double*, const double*, int, int, int, int) const {}
  __device__ NormalParams params(const Datum& a, const double* q, const double* c) const {
    return {c[0] + c[1] * q[2 + a.j], a.sg};
  }
  __device__ double term(const Datum& a, const double* q, const double* c) const {
    const NormalParams p = params(a, q, c);
    const double z = (a.y - p.loc) / p.scale;
    return -0.5 * (z * z + a.cn);
  }
};

// sv: r_t ~ StudentT(nu, 0, exp(s_t)) with log scale s_t (student_t.ex:15-29 as the kind writes it)
struct IcSvSrc {
  static constexpr bool kStaged = true;
  const double* r;   // dev [100]
  double lz[9];      // f32-rounded Lanczos coefficients (math.ex:27-52)
  double half_log_2pi32, pi32, tiny32;
  bool ncp;          // EXMC_MODEL_SV_NCP: dims 1..99 are z_t, s_t = s_{t-1} + sigma z_t
  struct Datum { double r; int t; };
  __device__ Datum load(int i) const { return {r[i], i}; }
  __device__ double obs(int i) const { return r[i]; }
  __device__ double lgam(double x) const {
    const double t = x + 6.5;
    double ag = lz[0];
    for (int i = 1; i < 9; i++) ag = ag + lz[i] / (x + (double)(i - 1) * 1.0);
    return ((half_log_2pi32 + (x - 0.5) * exmc_log(t)) - t) + exmc_log(ag);
  }
  __device__ void consts(const double* q, double* c) const {
    const double nu = exmc_exp(ic_clamp200(q[101]));
    const double sdf = fmax(nu, tiny32);
    const double hp1 = (sdf + 1.0) / 2.0, h = sdf / 2.0;
    c[0] = (lgam(hp1) - lgam(h)) - 0.5 * exmc_log(sdf * pi32);
    c[1] = hp1;
    c[2] = sdf;
    c[3] = exmc_exp(ic_clamp200(q[100]));   // sigma (the ncp walk)
  }
  // sv_ncp: the walk x = (s_1, sigma z_2, ..., sigma z_100) summed by wave_scan_fwd (the kind's
  // association order, include/exmc_scan.h), one wavefront per sample, lane l holding x_l, x_{64+l}
  __device__ void prepare(double* tile, const double* cst, int ld, int nt, int tid, int nthreads) const {
    if (!ncp) return;
    const int lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;
    for (int t = wave; t < nt; t += nwaves) {
      double* q = tile + (size_t)t * ld;
      const double sigma = cst[t * (kIcConsts + 1) + 1 + 3];
      double v[2];
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const int i = lane + 64 * k;
        v[k] = (i == 0) ? q[0] : ((i < 100) ? sigma * q[i] : 0.0);
      }
      wave_scan_fwd(v);
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const int i = lane + 64 * k;
        if (i < 100) q[i] = v[k];
      }
    }
  }
  // (term works with exp(-s_t), the reciprocal of this scale, and does not call it)
  __device__ StudentTParams params(const Datum& a, const double* q, const double* c) const {
    return {c[2], 0.0, exmc_exp(q[a.t])};
  }
  __device__ double term(const Datum& a, const double* q, const double* c) const {
    const double s = q[a.t];
    const double z = a.r * exmc_exp(-s);
    const double w = (z * z) / c[2];
    const double l = exmc_log(1.0 + w);
    return (c[0] - s) - c[1] * l;
  }
};

// logistic: y_i ~ Bernoulli(sigmoid(alpha + x_i . beta)), p clipped (bernoulli.ex:17-27). For
// y in {0, 1} the logpdf y log pc + (1 - y) log(1 - pc) is the one logarithm bit for bit (the other
// product is a signed zero), so only that one is evaluated.
struct IcLogisticSrc {
  static constexpr bool kStaged = true;
  static constexpr int K = 20;
  const double* X;   // dev [N][20]
  const double* y;   // dev [N]
  double lo, hi;
  struct Datum { double x[K]; double y; };
  __device__ Datum load(int i) const {
    Datum a;
#pragma unroll
    for (int j = 0; j < K; j++) a.x[j] = X[(size_t)i * K + j];
    a.y = y[i];
    return a;
  }
  __device__ double obs(int i) const { return y[i]; }
  __device__ void consts(const double*, double*) const {}
  __device__ void prepare(double*, const double*, int, int, int, int) const {}
  __device__ BernoulliParams params(const Datum& a, const double* q, const double*) const {
    double eta = q[0];
#pragma unroll
    for (int j = 0; j < K; j++) eta = __builtin_fma(a.x[j], q[1 + j], eta);
    return {1.0 / (1.0 + exmc_exp(-eta))};
  }
  __device__ double term(const Datum& a, const double* q, const double* c) const {
    const double p = params(a, q, c).p;
    const double pc = fmin(fmax(p, lo), hi);
    if (a.y == 1.0 || a.y == 0.0) return exmc_log(a.y == 1.0 ? pc : 1.0 - pc);
    return a.y * exmc_log(pc) + (1.0 - a.y) * exmc_log(1.0 - pc);
  }
};

// radon: y_i ~ Normal(alpha_j(i) + beta floor_i, sigma_y); prepare turns the tile's alpha_raw_j into
// alpha_j = (mu_alpha + gamma_u u_j) + sigma_alpha alpha_raw_j, once per (sample, county)
struct IcRadonSrc {
  static constexpr bool kStaged = true;
  static constexpr int J = 85;
  const double* u;    // dev [85]
  const double* cs;   // dev [86] county offsets (sorted observations)
  const double* fl;   // dev [N]
  const double* y;    // dev [N]
  double log2pi32, tiny32;
  struct Datum { double fl, y; int j; };
  __device__ Datum load(int i) const {
    int j = 0;
    while (j + 1 < J && (double)i >= cs[j + 1]) j++;
    return {fl[i], y[i], j};
  }
  __device__ double obs(int i) const { return y[i]; }
  __device__ void consts(const double* q, double* c) const {
    const double sy = exmc_exp(ic_clamp200(q[J + 3]));
    const double ssy = fmax(sy, tiny32);
    c[0] = exmc_exp(ic_clamp200(q[J + 2]));   // sigma_alpha
    c[1] = ssy;
    c[2] = log2pi32 + 2.0 * exmc_log(ssy);
    c[3] = q[J + 4];                          // beta
  }
  __device__ void prepare(double* tile, const double* cst, int ld, int nt, int tid, int nthreads) const {
    for (int e = tid; e < nt * J; e += nthreads) {
      const int t = e / J, j = e - t * J;
      double* q = tile + (size_t)t * ld;
      const double sa = cst[t * (kIcConsts + 1) + 1];
      q[j] = (q[J] + q[J + 1] * u[j]) + sa * q[j];
    }
  }
  __device__ NormalParams params(const Datum& a, const double* q, const double* c) const {
    return {q[a.j] + c[3] * a.fl, c[1]};
  }
  __device__ double term(const Datum& a, const double* q, const double* c) const {
    const NormalParams p = params(a, q, c);
    const double z = (a.y - p.loc) / p.scale;
    return -0.5 * (z * z + c[2]);
  }
};

// a matrix ll[S][N][C] the caller provides: the same reduction, no model
struct IcMatrixSrc {
  static constexpr bool kStaged = false;
  const double* ll;
  struct Datum { int i; };
  __device__ Datum load(int i) const { return {i}; }
  __device__ void consts(const double*, double*) const {}
  __device__ void prepare(double*, const double*, int, int, int, int) const {}
};

// ---- the kernels ---------------------------------------------------------------------------------
// LDS: tile [kIcTile][ld] (ld = d | 1), then per sample [1 / k, consts...]
__host__ __device__ inline int ic_ld(int d) { return d | 1; }
__host__ __device__ inline size_t ic_lds_bytes(int d) {
  return ((size_t)kIcTile * ic_ld(d) + (size_t)kIcTile * (kIcConsts + 1)) * 8;
}

// kOut = false: chunk partials [chunk][kIcFields][N] (ic_partials_kernel);
// kOut = true: the matrix out[S][N][C] (pointwise_ll_kernel). The N datums are the model's datums
// i0 .. i0 + N - 1 (pointwise_ll_range_kernel: a block of datums; i0 = 0 and all of them elsewhere).
template <class Src, bool kOut>
__device__ __forceinline__ void ic_body(const Src& src, const double* __restrict__ draws, int S, int d, int C,
                                        int N, long long chunk, double* __restrict__ out, int i0 = 0) {
  extern __shared__ double ic_lds[];
  const int ld = ic_ld(d);
  double* tile = ic_lds;
  double* cst = ic_lds + (size_t)kIcTile * ld;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int i = blockIdx.y * nthreads + tid;
  const bool own = i < N;
  const long long n = (long long)S * C;
  const long long k0 = (long long)blockIdx.x * chunk;
  const long long k1 = (k0 + chunk < n) ? k0 + chunk : n;
  typename Src::Datum dat = src.load(own ? i0 + i : 0);
  double st[kIcFields] = {-__builtin_inf(), 0.0, -__builtin_inf(), 0.0, 0.0, 0.0};
  for (long long kt = k0; kt < k1; kt += kIcTile) {
    const int nt = (int)((k1 - kt < kIcTile) ? k1 - kt : kIcTile);
    __syncthreads();   // the previous tile has been read
    if constexpr (Src::kStaged) {
      for (int e = tid; e < nt * d; e += nthreads) {
        const int j = e / nt, t = e - j * nt;
        const long long k = kt + t;
        const long long s = k / C, c = k - s * C;
        tile[(size_t)t * ld + j] = draws[((size_t)s * d + j) * C + c];
      }
      __syncthreads();
      if (tid < nt) src.consts(tile + (size_t)tid * ld, cst + tid * (kIcConsts + 1) + 1);
    }
    if (tid < nt) cst[tid * (kIcConsts + 1)] = 1.0 / (double)(kt + tid - k0 + 1);
    __syncthreads();
    if constexpr (Src::kStaged) {
      src.prepare(tile, cst, ld, nt, tid, nthreads);
      __syncthreads();
    }
    if (!own) continue;
    for (int t = 0; t < nt; t++) {
      const double* c = cst + t * (kIcConsts + 1);
      double x;
      if constexpr (Src::kStaged) {
        x = src.term(dat, tile + (size_t)t * ld, c + 1);
      } else {
        const long long k = kt + t;
        const long long s = k / C, cc = k - s * C;
        x = src.ll[((size_t)s * N + i) * C + cc];
      }
      if constexpr (kOut) {
        const long long k = kt + t;
        const long long s = k / C, cc = k - s * C;
        out[((size_t)s * N + i) * C + cc] = x;
      } else {
        ic_push(x, c[0], st);
      }
    }
  }
  if constexpr (!kOut) {
    if (own) {
      double* p = out + (size_t)blockIdx.x * kIcFields * N + i;
#pragma unroll
      for (int f = 0; f < kIcFields; f++) p[(size_t)f * N] = st[f];
    }
  }
}

template <class Src>
__global__ __launch_bounds__(kIcBlock) void ic_partials_kernel(Src src, const double* __restrict__ draws, int S,
                                                              int d, int C, int N, long long chunk,
                                                              double* __restrict__ part) {
  ic_body<Src, false>(src, draws, S, d, C, N, chunk, part);
}

template <class Src>
__global__ __launch_bounds__(kIcBlock) void pointwise_ll_kernel(Src src, const double* __restrict__ draws, int S,
                                                               int d, int C, int N, long long chunk,
                                                               double* __restrict__ ll) {
  ic_body<Src, true>(src, draws, S, d, C, N, chunk, ll);
}

// the matrix of the datums i0 .. i0 + Nb - 1 alone, out[S][Nb][C]: what PSIS-LOO (exmc_psis.hpp) walks
// the model's datums in
template <class Src>
__global__ __launch_bounds__(kIcBlock) void pointwise_ll_range_kernel(Src src, const double* __restrict__ draws,
                                                                     int S, int d, int C, int i0, int Nb,
                                                                     long long chunk, double* __restrict__ ll) {
  ic_body<Src, true>(src, draws, S, d, C, Nb, chunk, ll, i0);
}

#ifndef EXMC_ONLY_CUSTOM   // a generated model's plug-in carries no model-comparison kernels
// chunk states left to right (Chan et al.'s pairwise Welford update), then the statistics:
// stats[0][i] lppd_i = (m + log s) - log n           (log_mean_exp, model_comparison.ex:253-258)
// stats[1][i] p_waic_i = M2 / (n - 1)                 (variance, :260-269)
// stats[2][i] elpd_loo_i = -((m' + log s') - log n)   (loo_i_basic, :271-276; m', s' of -ll)
// stats[3][i] p_loo_i = lppd_i - elpd_loo_i
__global__ __launch_bounds__(256) void ic_merge_kernel(const double* __restrict__ part, int n_chunks, long long n,
                                                      long long chunk, int N, double* __restrict__ stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const double* p = part + i;
  double m = p[0], s = p[(size_t)N], mn = p[(size_t)2 * N], sn = p[(size_t)3 * N];
  double mean = p[(size_t)4 * N], m2 = p[(size_t)5 * N];
  double na = (double)((chunk < n) ? chunk : n);
  for (int b = 1; b < n_chunks; b++) {
    const double* q = part + (size_t)b * kIcFields * N + i;
    const long long kb0 = (long long)b * chunk;
    const double nb = (double)((kb0 + chunk < n) ? chunk : n - kb0);
    ic_lse_merge(m, s, q[0], q[(size_t)N]);
    ic_lse_merge(mn, sn, q[(size_t)2 * N], q[(size_t)3 * N]);
    const double nab = na + nb;
    const double delta = q[(size_t)4 * N] - mean;
    mean = mean + delta * (nb / nab);
    m2 = (m2 + q[(size_t)5 * N]) + delta * delta * ((na * nb) / nab);
    na = nab;
  }
  const double logn = exmc_log(na);
  const double lppd = (m + exmc_log(s)) - logn;
  const double elpd = -((mn + exmc_log(sn)) - logn);
  stats[i] = lppd;
  stats[(size_t)N + i] = m2 / (na - 1.0);
  stats[(size_t)2 * N + i] = elpd;
  stats[(size_t)3 * N + i] = lppd - elpd;
}
#endif

}  // namespace exmc
