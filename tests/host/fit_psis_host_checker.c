/* fit_psis_host_checker.c -- the host statement of the smoothing and the resampling of log importance
 * ratios on the device (exmc_amd/csrc/exmc_psis_ratio.hpp, include/exmc_hip_fit_psis.h, DESIGN.md
 * "Importance diagnostics of the fits"), written again in plain C from the contract with the
 * exmc_detmath.h functions and the stated orders. Test infrastructure only (tests/fit_psis_checker.py
 * loads it with ctypes); never linked into the product. Build with -ffp-contract=off against
 * include/exmc_detmath.h.
 *
 * The tail fit, its sums and the log-sum-exp steps are those of psis_host_checker.c, taken from there.
 * Orders restated here:
 *   L1 = lse(x), L2 = lse(2 x): chunks of ic_chunk(n) samples in sample order, merged left to right;
 *   the cumulative sum: blocks of 4096 consecutive samples, r_k the running sum inside the block from
 *     0.0, base_b the earlier blocks' totals left to right from 0.0, cum_k = base_b + r_k;
 *   the search: the first k in sample order with cum_k >= pos_j, by a plain scan. */
#include "psis_host_checker.c" /* chunk_of, lse_push, lse_merge, psis_fit, pair_t, cmp_pair, cmp_desc */

enum { SCAN = 4096 };

/* OTP :rand exsss (Xorshift116**) seeded through splitmix64, as exmc_device.hpp restates it */
#define MASK58 ((1ULL << 58) - 1)
static uint64_t splitmix64(uint64_t* x) {
  uint64_t z = (*x += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
static uint64_t rotl58(uint64_t x, int n) { return ((x << n) & MASK58) | (x >> (58 - n)); }
double fit_psis_first_uniform(uint64_t seed) {
  uint64_t x = seed, w[2];
  for (int i = 0; i < 2; i++) {
    uint64_t z;
    do z = splitmix64(&x) & MASK58;
    while (z == 0);
    w[i] = z;
  }
  const uint64_t s0 = w[1];
  const uint64_t v1 = (s0 + ((s0 << 2) & MASK58)) & MASK58;
  const uint64_t v2 = rotl58(v1, 7);
  const uint64_t out = (v2 + ((v2 << 3) & MASK58)) & MASK58;
  return (double)(out >> 5) * 0x1p-53;
}

/* lr [S][Nb][C], group i the samples k = s C + c -> out [5][Nb] (khat, log_mean_ratio, ess, n_zero, T);
 * lw (the layout of lr) and idx [R][Nb] where given */
int fit_psis_groups(const double* lr, int S, int Nb, int C, int R, uint64_t seed, double* out, double* lw,
                    int32_t* idx) {
  const long long n = (long long)S * C, chunk = chunk_of(n);
  const int n_chunks = (int)((n + chunk - 1) / chunk);
  const int M = psis_tail_len(n);
  const double nan = exmc_from_bits(EXMC_NAN_BITS);
  double* x = (double*)malloc(sizeof(double) * (size_t)n);
  double* v = (double*)malloc(sizeof(double) * (size_t)n);
  double* srt = (double*)malloc(sizeof(double) * (size_t)n);
  double* cum = (double*)malloc(sizeof(double) * (size_t)n);
  pair_t* tail = (pair_t*)malloc(sizeof(pair_t) * (size_t)(M + 1));
  double* t = (double*)malloc(sizeof(double) * (size_t)(M + 1));
  if (!x || !v || !srt || !cum || !tail || !t) return -1;
  for (int i = 0; i < Nb; i++) {
    int bad = 0;
    double mx = -INFINITY;
    for (long long k = 0; k < n; k++) {
      const long long s = k / C, c = k - s * C;
      v[k] = lr[((size_t)s * Nb + i) * C + c];
      if (!(v[k] == v[k]) || v[k] == INFINITY) bad = 1;
      mx = fmax(mx, v[k]);
    }
    if (mx == -INFINITY) bad = 1; /* no finite ratio */
    if (bad) {
      for (int f = 0; f < 5; f++) out[(size_t)f * Nb + i] = nan;
      for (long long k = 0; lw && k < n; k++) {
        const long long s = k / C, c = k - s * C;
        lw[((size_t)s * Nb + i) * C + c] = nan;
      }
      for (int j = 0; idx && j < R; j++) idx[(size_t)j * Nb + i] = -1;
      continue;
    }
    for (long long k = 0; k < n; k++) srt[k] = x[k] = v[k] - mx;
    qsort(srt, (size_t)n, sizeof(double), cmp_desc);
    const double cutoff = fmax(M < n ? srt[M] : -INFINITY, LOG_DBL_MIN); /* the (M + 1)-th largest */
    int T = 0;
    for (long long k = 0; k < n; k++)
      if (x[k] > cutoff) {
        tail[T].x = x[k];
        tail[T].k = (uint32_t)k;
        T++;
      }
    double khat = INFINITY;
    if (T > 4) {
      qsort(tail, (size_t)T, sizeof(pair_t), cmp_pair);
      const double ec = exmc_exp(cutoff);
      double sigma;
      for (int j = 0; j < T; j++) t[j] = exmc_exp(tail[j].x) - ec;
      psis_fit(t, T, &khat, &sigma);
      if (!(khat == khat)) khat = nan;
      if (exmc_isfinite(khat)) {
        for (int j = 0; j < T; j++) {
          const double p = ((double)(j + 1) - 0.5) / (double)T;
          const double lq = exmc_log1p(-p);
          const double g = (khat == 0.0) ? -sigma * lq : (sigma * exmc_expm1(-khat * lq)) / khat;
          x[tail[j].k] = exmc_log(g + ec);
        }
      }
    }
    double st[4], acc[4] = {0}, zeros = 0.0;
    for (int b = 0; b < n_chunks; b++) {
      const long long k0 = (long long)b * chunk, k1 = (k0 + chunk < n) ? k0 + chunk : n;
      double z = 0.0;
      st[0] = st[2] = -INFINITY;
      st[1] = st[3] = 0.0;
      for (long long k = k0; k < k1; k++) {
        x[k] = fmin(x[k], 0.0);
        lse_push(x[k], &st[0], &st[1]);
        lse_push(2.0 * x[k], &st[2], &st[3]);
        z = z + ((v[k] == -INFINITY) ? 1.0 : 0.0);
      }
      if (b == 0) {
        memcpy(acc, st, sizeof(acc));
        zeros = z;
      } else {
        lse_merge(&acc[0], &acc[1], st[0], st[1]);
        lse_merge(&acc[2], &acc[3], st[2], st[3]);
        zeros = zeros + z;
      }
    }
    const double L1 = acc[0] + exmc_log(acc[1]), L2 = acc[2] + exmc_log(acc[3]);
    out[i] = khat;
    out[(size_t)Nb + i] = (mx + L1) - exmc_log((double)n);
    out[(size_t)2 * Nb + i] = exmc_exp(2.0 * L1 - L2);
    out[(size_t)3 * Nb + i] = zeros;
    out[(size_t)4 * Nb + i] = (double)T;
    for (long long k = 0; k < n; k++) x[k] = x[k] - L1;
    for (long long k = 0; lw && k < n; k++) {
      const long long s = k / C, c = k - s * C;
      lw[((size_t)s * Nb + i) * C + c] = x[k];
    }
    if (!idx || R < 1) continue;
    double base = 0.0, r = 0.0;
    for (long long k = 0; k < n; k++) {
      if (k % SCAN == 0) {
        base = base + r; /* the total of the block before */
        r = 0.0;
      }
      r = r + exmc_exp(x[k]);
      cum[k] = base + r;
    }
    const double u = fit_psis_first_uniform(seed + 7919ULL * (uint64_t)i);
    long long k = 0;
    for (int j = 0; j < R; j++) {
      const double pos = (u + (double)j) / (double)R;
      while (k < n && !(cum[k] >= pos)) k++; /* pos ascends with j: the scan goes on where it stood */
      idx[(size_t)j * Nb + i] = (int32_t)(k < n ? k : n - 1);
    }
  }
  free(x);
  free(v);
  free(srt);
  free(cum);
  free(tail);
  free(t);
  return 0;
}
