/* psis_host_checker.c -- the host statement of PSIS-LOO on the device (exmc_amd/csrc/exmc_psis.hpp,
 * include/exmc_hip_compare.h, DESIGN.md "PSIS-LOO"): the estimator written again in plain C from the
 * contract, with the exmc_detmath.h functions and the stated accumulation orders. Test
 * infrastructure only (tests/psis_checker.py loads it with ctypes); never linked into the product.
 * Build with -ffp-contract=off against include/exmc_detmath.h.
 *
 * Orders restated here:
 *   tail sums (kappa_j, kappa): 64 partial sums, term i into partial i mod 64 in ascending i, each
 *     from 0.0; then adjacent pairs, pairs of pairs, ... (p[l] += p[l + w] for w = 1, 2, .., 32);
 *   sums over the grid (the weights' denominators, their total, b): left to right from 0.0;
 *   the log-sum-exps: chunks of ic_chunk(n) samples in sample order, merged left to right. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "exmc_detmath.h"

enum { TILE = 64, TARGET_CHUNKS = 1024 };
#define LOG_DBL_MIN (-0x1.6232bdd7abcd2p+9)

static long long chunk_of(long long n) {
  const long long per = (long long)TILE * TARGET_CHUNKS;
  return (long long)TILE * ((n + per - 1) / per);
}

double psis_expm1(double x) { return exmc_expm1(x); }
void psis_expm1_v(const double* x, long n, double* out) {
  for (long i = 0; i < n; i++) out[i] = exmc_expm1(x[i]);
}

int psis_tail_len(long long n) { return (int)ceil(fmin((double)n / 5.0, 3.0 * sqrt((double)n))); }

static void lse_push(double x, double* m, double* s) {
  if (!(x == x)) {
    *m = x;
    *s = x;
  } else if (x == -INFINITY) {
  } else if (x > *m) {
    *s = *s * exmc_exp(*m - x) + 1.0;
    *m = x;
  } else if (x == *m) {
    *s = *s + 1.0;
  } else {
    *s = *s + exmc_exp(x - *m);
  }
}
static void lse_merge(double* m, double* s, double m2, double s2) {
  if (!(*m == *m) || !(m2 == m2)) {
    *m = NAN;
    *s = NAN;
  } else if (m2 == -INFINITY) {
  } else if (*m == -INFINITY) {
    *m = m2;
    *s = s2;
  } else if (*m == m2) {
    *s = *s + s2;
  } else if (*m > m2) {
    *s = *s + s2 * exmc_exp(m2 - *m);
  } else {
    *s = *s * exmc_exp(*m - m2) + s2;
    *m = m2;
  }
}

static double tail_sum(const double* t, int T, double b) {
  double p[64];
  for (int l = 0; l < 64; l++) p[l] = 0.0;
  for (int i = 0; i < T; i++) p[i & 63] = p[i & 63] + exmc_log1p(-b * t[i]);
  for (int w = 1; w < 64; w *= 2)
    for (int l = 0; l < 64; l += 2 * w) p[l] = p[l] + p[l + w];
  return p[0];
}

/* Zhang & Stephens' posterior-mean fit of (k, sigma) to t[T] ascending, with PSIS' prior on k */
void psis_fit(const double* t, int T, double* k_out, double* sigma_out) {
  const double dT = (double)T;
  const int m = 30 + (int)sqrt(dT);
  const double tT = t[T - 1], tq = t[(int)(dT / 4.0 + 0.5) - 1];
  double* b = (double*)malloc(sizeof(double) * 3 * (size_t)m);
  double *L = b + m, *w = b + 2 * m;
  for (int j = 0; j < m; j++) {
    b[j] = 1.0 / tT + (1.0 - sqrt((double)m / ((double)(j + 1) - 0.5))) / (3.0 * tq);
    const double kap = tail_sum(t, T, b[j]) / dT;
    L[j] = dT * ((exmc_log(-b[j] / kap) - kap) - 1.0);
  }
  for (int j = 0; j < m; j++) {
    double s = 0.0;
    for (int q = 0; q < m; q++) s = s + exmc_exp(L[q] - L[j]);
    const double wj = 1.0 / s;
    w[j] = (wj < 10.0 * DBL_EPSILON) ? 0.0 : wj;
  }
  double W = 0.0, bh = 0.0;
  for (int j = 0; j < m; j++) W = W + w[j];
  for (int j = 0; j < m; j++) bh = bh + (w[j] / W) * b[j];
  const double kap = tail_sum(t, T, bh) / dT;
  *sigma_out = -kap / bh;
  *k_out = (dT * kap + 10.0 * 0.5) / (dT + 10.0);
  free(b);
}

typedef struct { double x; uint32_t k; } pair_t;
static int cmp_pair(const void* a, const void* b) {
  const pair_t *p = (const pair_t*)a, *q = (const pair_t*)b;
  if (p->x != q->x) return p->x < q->x ? -1 : 1;
  return p->k < q->k ? -1 : (p->k > q->k);
}
static int cmp_desc(const void* a, const void* b) {
  const double p = *(const double*)a, q = *(const double*)b;
  return p > q ? -1 : (p < q);
}

/* out[3][N] (elpd_loo, p_loo, k) of ll [S][N][C]; tails[N], if given, receives each datum's T */
int psis_stats(const double* ll, int S, int N, int C, double* out, int* tails) {
  const long long n = (long long)S * C, chunk = chunk_of(n);
  const int n_chunks = (int)((n + chunk - 1) / chunk);
  const int M = psis_tail_len(n);
  double* x = (double*)malloc(sizeof(double) * (size_t)n);
  double* v = (double*)malloc(sizeof(double) * (size_t)n);
  double* srt = (double*)malloc(sizeof(double) * (size_t)n);
  pair_t* tail = (pair_t*)malloc(sizeof(pair_t) * (size_t)(M + 1));
  double* t = (double*)malloc(sizeof(double) * (size_t)(M + 1));
  if (!x || !v || !srt || !tail || !t) return -1;
  for (int i = 0; i < N; i++) {
    int bad = 0;
    double mx = -INFINITY;
    for (long long k = 0; k < n; k++) {
      const long long s = k / C, c = k - s * C;
      v[k] = ll[((size_t)s * N + i) * C + c];
      if (!exmc_isfinite(v[k])) bad = 1;
      mx = fmax(mx, -v[k]);
    }
    if (tails) tails[i] = 0;
    if (bad) {
      out[i] = out[(size_t)N + i] = out[(size_t)2 * N + i] = exmc_from_bits(EXMC_NAN_BITS);
      continue;
    }
    for (long long k = 0; k < n; k++) srt[k] = x[k] = -v[k] - mx;
    qsort(srt, (size_t)n, sizeof(double), cmp_desc);
    const double cutoff = fmax(srt[M], LOG_DBL_MIN);   /* the (M + 1)-th largest */
    int T = 0;
    for (long long k = 0; k < n; k++)
      if (x[k] > cutoff) {
        tail[T].x = x[k];
        tail[T].k = (uint32_t)k;
        T++;
      }
    if (tails) tails[i] = T;
    double khat = INFINITY;
    if (T > 4) {
      qsort(tail, (size_t)T, sizeof(pair_t), cmp_pair);
      const double ec = exmc_exp(cutoff);
      double sigma;
      for (int j = 0; j < T; j++) t[j] = exmc_exp(tail[j].x) - ec;
      psis_fit(t, T, &khat, &sigma);
      if (!(khat == khat)) khat = exmc_from_bits(EXMC_NAN_BITS);
      if (exmc_isfinite(khat)) {
        for (int j = 0; j < T; j++) {
          const double p = ((double)(j + 1) - 0.5) / (double)T;
          const double lq = exmc_log1p(-p);
          const double g = (khat == 0.0) ? -sigma * lq : (sigma * exmc_expm1(-khat * lq)) / khat;
          x[tail[j].k] = exmc_log(g + ec);
        }
      }
    }
    double st[6] = {0}, acc[6] = {0};
    for (int b = 0; b < n_chunks; b++) {
      const long long k0 = (long long)b * chunk, k1 = (k0 + chunk < n) ? k0 + chunk : n;
      st[0] = st[2] = st[4] = -INFINITY;
      st[1] = st[3] = st[5] = 0.0;
      for (long long k = k0; k < k1; k++) {
        const double xk = fmin(x[k], 0.0);
        lse_push(xk + v[k], &st[0], &st[1]);
        lse_push(xk, &st[2], &st[3]);
        lse_push(v[k], &st[4], &st[5]);
      }
      if (b == 0) memcpy(acc, st, sizeof(acc));
      else
        for (int f = 0; f < 6; f += 2) lse_merge(&acc[f], &acc[f + 1], st[f], st[f + 1]);
    }
    const double lppd = (acc[4] + exmc_log(acc[5])) - exmc_log((double)n);
    const double elpd = (acc[0] + exmc_log(acc[1])) - (acc[2] + exmc_log(acc[3]));
    out[i] = elpd;
    out[(size_t)N + i] = lppd - elpd;
    out[(size_t)2 * N + i] = khat;
  }
  free(x);
  free(v);
  free(srt);
  free(tail);
  free(t);
  return 0;
}
