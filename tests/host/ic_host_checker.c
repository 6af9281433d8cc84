/* ic_host_checker.c -- the host statement of model comparison on the device (exmc_amd/csrc/exmc_ic.hpp,
 * include/exmc_hip_compare.h, DESIGN.md "Model comparison"): every built-in kind's per-datum term,
 * and the chunked accumulation and left-to-right merge, written again in plain C from the contract.
 * Test infrastructure only (tests/test_ic_host.py, tests/test_gpu_model_comparison.py load it with
 * ctypes); never linked into the product. Build with -ffp-contract=off against
 * include/exmc_detmath.h and include/exmc_scan.h. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "exmc_detmath.h"
#include "exmc_scan.h"

enum { K_SIMPLE = 1, K_EIGHT_SCHOOLS = 2, K_SV = 3, K_LOGISTIC = 4, K_RADON = 5, K_SV_NCP = 7 };
enum { TILE = 64, TARGET_CHUNKS = 1024 };

static double f32r(double x) { return (double)(float)x; }
static double log2pi32(void) { return f32r(log(f32r(2.0 * M_PI))); }
static double tiny32(void) { return f32r(1.0e-30); }
static double clamp200(double z) { return fmax(-200.0, fmin(z, 200.0)); }

long long ic_chunk(long long n) {
  const long long per = (long long)TILE * TARGET_CHUNKS;
  return (long long)TILE * ((n + per - 1) / per);
}

/* number of datums of a kind's data blob (the exmc_hip_model_create data), -1 if none */
int ic_n_data(int kind, int n_blob) {
  switch (kind) {
    case K_SIMPLE: return n_blob;
    case K_EIGHT_SCHOOLS: return 8;
    case K_SV: case K_SV_NCP: return 100;
    case K_LOGISTIC: return n_blob / 21;
    case K_RADON: return (n_blob - 171) / 2;
    default: return -1;
  }
}

static const double LANCZOS[9] = {0.99999999999980993,  676.5203681218851,     -1259.1392167224028,
                                  771.32342877765313,   -176.61502916214059,   12.507343278686905,
                                  -0.13857109526572012, 9.9843695780195716e-6, 1.5056327351493116e-7};

static double lgam(double x) {
  const double t = x + 6.5;
  double ag = f32r(LANCZOS[0]);
  for (int i = 1; i < 9; i++) ag = ag + f32r(LANCZOS[i]) / (x + (double)(i - 1) * 1.0);
  return ((f32r(0.5 * log(2.0 * M_PI)) + (x - 0.5) * exmc_log(t)) - t) + exmc_log(ag);
}

/* ll[N] of one sample q[d] (kernel order), datums in the handle's order */
int ic_terms(int kind, const double* blob, int n_blob, const double* q, double* ll) {
  const int N = ic_n_data(kind, n_blob);
  if (N < 0) return -1;
  if (kind == K_SIMPLE) {
    const double ss = fmax(exmc_exp(clamp200(q[1])), tiny32());
    const double cn = log2pi32() + 2.0 * exmc_log(ss);
    for (int i = 0; i < N; i++) {
      const double z = (blob[i] - q[0]) / ss;
      ll[i] = -0.5 * (z * z + cn);
    }
  } else if (kind == K_EIGHT_SCHOOLS) {
    const double mu = q[0], tau = exmc_exp(clamp200(q[1]));
    for (int j = 0; j < 8; j++) {
      const double sg = blob[8 + j];
      const double theta = mu + tau * q[2 + j];
      const double z = (blob[j] - theta) / sg;
      ll[j] = -0.5 * (z * z + (log2pi32() + 2.0 * exmc_log(sg)));
    }
  } else if (kind == K_SV || kind == K_SV_NCP) {
    const double sdf = fmax(exmc_exp(clamp200(q[101])), tiny32());
    const double hp1 = (sdf + 1.0) / 2.0, h = sdf / 2.0;
    const double An = (lgam(hp1) - lgam(h)) - 0.5 * exmc_log(sdf * f32r(M_PI));
    double s[128];
    if (kind == K_SV_NCP) {
      const double sigma = exmc_exp(clamp200(q[100]));
      for (int i = 0; i < 128; i++) s[i] = (i == 0) ? q[0] : ((i < 100) ? sigma * q[i] : 0.0);
      exmc_scan_fwd64(s, 2);
    } else {
      for (int i = 0; i < 100; i++) s[i] = q[i];
    }
    for (int t = 0; t < 100; t++) {
      const double z = blob[t] * exmc_exp(-s[t]);
      const double w = (z * z) / sdf;
      ll[t] = (An - s[t]) - hp1 * exmc_log(1.0 + w);
    }
  } else if (kind == K_LOGISTIC) {
    const double* X = blob;
    const double* y = blob + (size_t)N * 20;
    const double lo = f32r(1.0e-7), hi = 1.0 - f32r(1.0e-7);
    for (int i = 0; i < N; i++) {
      double eta = q[0];
      for (int j = 0; j < 20; j++) eta = __builtin_fma(X[(size_t)i * 20 + j], q[1 + j], eta);
      const double p = 1.0 / (1.0 + exmc_exp(-eta));
      const double pc = fmin(fmax(p, lo), hi);
      ll[i] = y[i] * exmc_log(pc) + (1.0 - y[i]) * exmc_log(1.0 - pc);   /* bernoulli.ex:17-27 */
    }
  } else if (kind == K_RADON) {
    const int J = 85;
    const double* u = blob;
    const double* cs = blob + J;
    const double* fl = blob + 2 * J + 1;
    const double* y = fl + N;
    const double sa = exmc_exp(clamp200(q[J + 2]));
    const double ssy = fmax(exmc_exp(clamp200(q[J + 3])), tiny32());
    const double cn = log2pi32() + 2.0 * exmc_log(ssy);
    for (int j = 0; j < J; j++) {
      const double alpha = (q[J] + q[J + 1] * u[j]) + sa * q[j];
      for (int i = (int)cs[j]; i < (int)cs[j + 1]; i++) {
        const double mean = alpha + q[J + 4] * fl[i];
        const double z = (y[i] - mean) / ssy;
        ll[i] = -0.5 * (z * z + cn);
      }
    }
  }
  return N;
}

/* ---- the online state and its merge ---- */
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

/* stats[4][N] of ll [S][N][C] (or, with ll == NULL, of the kind's terms over draws [S][d][C]):
 * samples k = s C + c, chunks of ic_chunk(S C), Welford with 1.0 / (position in chunk), chunk
 * states merged left to right */
int ic_stats(const double* ll, int kind, const double* blob, int n_blob, const double* draws, int d, int S,
             int N, int C, double* stats) {
  const long long n = (long long)S * C, chunk = ic_chunk(n);
  const int n_chunks = (int)((n + chunk - 1) / chunk);
  double* st = (double*)malloc(sizeof(double) * 6 * (size_t)N * n_chunks);
  double* row = (double*)malloc(sizeof(double) * (size_t)N);
  double* q = (double*)malloc(sizeof(double) * (size_t)(d > 0 ? d : 1));
  if (!st || !row || !q) return -1;
  for (int b = 0; b < n_chunks; b++) {
    double* p = st + (size_t)b * 6 * N;
    for (int i = 0; i < N; i++) {
      p[i] = -INFINITY; p[(size_t)N + i] = 0.0; p[(size_t)2 * N + i] = -INFINITY;
      p[(size_t)3 * N + i] = 0.0; p[(size_t)4 * N + i] = 0.0; p[(size_t)5 * N + i] = 0.0;
    }
    const long long k0 = (long long)b * chunk, k1 = (k0 + chunk < n) ? k0 + chunk : n;
    for (long long k = k0; k < k1; k++) {
      const long long s = k / C, c = k - s * C;
      if (ll) {
        for (int i = 0; i < N; i++) row[i] = ll[((size_t)s * N + i) * C + c];
      } else {
        for (int j = 0; j < d; j++) q[j] = draws[((size_t)s * d + j) * C + c];
        ic_terms(kind, blob, n_blob, q, row);
      }
      const double rk = 1.0 / (double)(k - k0 + 1);
      for (int i = 0; i < N; i++) {
        const double x = row[i];
        lse_push(x, &p[i], &p[(size_t)N + i]);
        lse_push(-x, &p[(size_t)2 * N + i], &p[(size_t)3 * N + i]);
        const double delta = x - p[(size_t)4 * N + i];
        p[(size_t)4 * N + i] = p[(size_t)4 * N + i] + delta * rk;
        p[(size_t)5 * N + i] = p[(size_t)5 * N + i] + delta * (x - p[(size_t)4 * N + i]);
      }
    }
  }
  for (int i = 0; i < N; i++) {
    double m = st[i], s = st[(size_t)N + i], mn = st[(size_t)2 * N + i], sn = st[(size_t)3 * N + i];
    double mean = st[(size_t)4 * N + i], m2 = st[(size_t)5 * N + i];
    double na = (double)(chunk < n ? chunk : n);
    for (int b = 1; b < n_chunks; b++) {
      const double* p = st + (size_t)b * 6 * N + i;
      const long long kb0 = (long long)b * chunk;
      const double nb = (double)((kb0 + chunk < n) ? chunk : n - kb0);
      lse_merge(&m, &s, p[0], p[(size_t)N]);
      lse_merge(&mn, &sn, p[(size_t)2 * N], p[(size_t)3 * N]);
      const double nab = na + nb;
      const double delta = p[(size_t)4 * N] - mean;
      mean = mean + delta * (nb / nab);
      m2 = (m2 + p[(size_t)5 * N]) + delta * delta * ((na * nb) / nab);
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
  free(st);
  free(row);
  free(q);
  return 0;
}

/* ll [S][N][C] of the kind's terms over draws [S][d][C] */
int ic_pointwise(int kind, const double* blob, int n_blob, const double* draws, int d, int S, int C, double* ll) {
  const int N = ic_n_data(kind, n_blob);
  double* q = (double*)malloc(sizeof(double) * (size_t)d);
  double* row = (double*)malloc(sizeof(double) * (size_t)(N > 0 ? N : 1));
  if (!q || !row) return -1;
  for (int s = 0; s < S; s++)
    for (int c = 0; c < C; c++) {
      for (int j = 0; j < d; j++) q[j] = draws[((size_t)s * d + j) * C + c];
      ic_terms(kind, blob, n_blob, q, row);
      for (int i = 0; i < N; i++) ll[((size_t)s * N + i) * C + c] = row[i];
    }
  free(q);
  free(row);
  return N;
}
