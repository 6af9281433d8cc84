/* loo_pit_host_checker.c -- the host statement of PSIS-LOO-PIT on the device (exmc_amd/csrc/exmc_loo_pit.hpp,
 * include/exmc_hip_loo_pit.h, DESIGN.md "LOO-PIT"): the contract written again in plain C, with the
 * exmc_detmath.h functions and the stated orders. Test infrastructure only (tests/loo_pit_checker.py loads
 * it with ctypes); never linked into the product. Build with -ffp-contract=off against
 * include/exmc_detmath.h.
 *
 * The tail (its length, the cutoff, the order by (x, k), the fit psis_fit and the smoothed values) is
 * PSIS-LOO's, with the functions of psis_host_checker.c, which this file includes. Orders restated here:
 *   the state (m, sA, sL, sQ) per datum and block of 64 chains: draws ascending, within a draw the
 *     block's chains ascending;
 *   the blocks merged left to right. */
#include "psis_host_checker.c"

enum { LOO_PIT_BLOCK = 64 };

typedef struct { double m, sA, sL, sQ; } pit_state;

static void pit_push(pit_state* st, double x, int lt, int eq) {
  const double fL = lt ? 1.0 : 0.0, fQ = eq ? 1.0 : 0.0;
  if (!(x == x)) {
    st->m = st->sA = st->sL = st->sQ = x;
  } else if (x == -INFINITY) {
  } else if (x > st->m) {
    const double r = exmc_exp(st->m - x);
    st->sA = st->sA * r + 1.0;
    st->sL = st->sL * r + fL;
    st->sQ = st->sQ * r + fQ;
    st->m = x;
  } else if (x == st->m) {
    st->sA = st->sA + 1.0;
    st->sL = st->sL + fL;
    st->sQ = st->sQ + fQ;
  } else {
    const double e = exmc_exp(x - st->m);
    st->sA = st->sA + e;
    if (lt) st->sL = st->sL + e;
    if (eq) st->sQ = st->sQ + e;
  }
}

static void pit_merge(pit_state* a, const pit_state* b) {
  if (!(a->m == a->m) || !(b->m == b->m)) {
    a->m = a->sA = a->sL = a->sQ = NAN;
  } else if (b->m == -INFINITY) {
  } else if (a->m == -INFINITY) {
    *a = *b;
  } else if (a->m == b->m) {
    a->sA = a->sA + b->sA;
    a->sL = a->sL + b->sL;
    a->sQ = a->sQ + b->sQ;
  } else if (a->m > b->m) {
    const double r = exmc_exp(b->m - a->m);
    a->sA = a->sA + b->sA * r;
    a->sL = a->sL + b->sL * r;
    a->sQ = a->sQ + b->sQ * r;
  } else {
    const double r = exmc_exp(a->m - b->m);
    a->sA = a->sA * r + b->sA;
    a->sL = a->sL * r + b->sL;
    a->sQ = a->sQ * r + b->sQ;
    a->m = b->m;
  }
}

/* out[4][N] (p_lt, p_eq, pit, k) of ll, yrep [S][N][C] and y [N]; tails[N], if given, receives each
 * datum's T */
int loo_pit(const double* ll, const double* yrep, const double* y, int S, int N, int C, double* out, int* tails) {
  const long long n = (long long)S * C;
  const int M = psis_tail_len(n);
  const int B = (C + LOO_PIT_BLOCK - 1) / LOO_PIT_BLOCK;
  double* x = (double*)malloc(sizeof(double) * (size_t)n);
  double* srt = (double*)malloc(sizeof(double) * (size_t)n);
  pair_t* tail = (pair_t*)malloc(sizeof(pair_t) * (size_t)(M + 1));
  double* t = (double*)malloc(sizeof(double) * (size_t)(M + 1));
  if (!x || !srt || !tail || !t) return -1;
  for (int i = 0; i < N; i++) {
    int bad = 0;
    double mx = -INFINITY;
    for (long long k = 0; k < n; k++) {
      const long long s = k / C, c = k - s * C;
      const double v = ll[((size_t)s * N + i) * C + c];
      if (!exmc_isfinite(v)) bad = 1;
      mx = fmax(mx, -v);
    }
    if (tails) tails[i] = 0;
    if (bad) {
      for (int r = 0; r < 4; r++) out[(size_t)r * N + i] = exmc_from_bits(EXMC_NAN_BITS);
      continue;
    }
    for (long long k = 0; k < n; k++) {
      const long long s = k / C, c = k - s * C;
      srt[k] = x[k] = -ll[((size_t)s * N + i) * C + c] - mx;
    }
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
    pit_state acc = {-INFINITY, 0.0, 0.0, 0.0};
    for (int b = 0; b < B; b++) {
      const int c0 = b * LOO_PIT_BLOCK, c1 = (c0 + LOO_PIT_BLOCK < C) ? c0 + LOO_PIT_BLOCK : C;
      pit_state st = {-INFINITY, 0.0, 0.0, 0.0};
      for (int s = 0; s < S; s++)
        for (int c = c0; c < c1; c++) {
          const double v = yrep[((size_t)s * N + i) * C + c];
          pit_push(&st, fmin(x[(long long)s * C + c], 0.0), v < y[i], v == y[i]);
        }
      if (b == 0) acc = st;
      else pit_merge(&acc, &st);
    }
    const double p_lt = acc.sL / acc.sA, p_eq = acc.sQ / acc.sA;
    out[i] = p_lt;
    out[(size_t)N + i] = p_eq;
    out[(size_t)2 * N + i] = p_lt + 0.5 * p_eq;
    out[(size_t)3 * N + i] = khat;
  }
  free(x);
  free(srt);
  free(tail);
  free(t);
  return 0;
}
