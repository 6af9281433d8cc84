/* sv_ncp_checker.c — host statement of the non-centred stochastic-volatility kind
 * (EXMC_MODEL_SV_NCP, exmc_amd/csrc/exmc_models.hpp SVNcp<64>). TEST INFRASTRUCTURE: built by
 * tests/sv_ncp_checker.py with gcc -O2 -ffp-contract=off against include/exmc_detmath.h and hooked
 * into the checker as EXO_MODEL_CUSTOM. Product code never links it.
 *
 * Data r[100]; kernel order s_1, z_2..z_100, log sigma, log nu: what the reference's compiler makes
 * of sv with ncp: true. Its non-centring pass rewrites a Normal whose mu AND sigma are references
 * (rewrite/non_centered_parameterization.ex:50-55), so s_1 ~ Normal(0.0, sigma) stays centred and
 * s_t ~ Normal(s_{t-1}, sigma), t >= 2, becomes z_t ~ Normal(0, 1) with
 *   s_t = s_{t-1} + sigma z_t   (compiler.ex:444-463)
 *   r_t ~ StudentT(nu, 0, exp(s_t)), sigma ~ Exponential(50), nu ~ Exponential(0.1), both :log;
 *   the Normal terms by dist/normal.ex:15-24 with its f32 literals, as the centred kind takes them.
 * Gradient in reverse mode through the walk: A_t = sum_{u >= t} dL/ds_u (likelihood),
 *   d/ds_1 = A_1 - e_1 / sigma,  d/dz_t = -z_t + sigma A_t,
 *   d/dlog sigma = (e_1^2 - 1) + sum_{t >= 2} (sigma z_t) A_t + the prior's terms (e_1 = s_1 / sigma).
 *
 * Two association orders of the same expressions:
 *   sv_ncp_dev  the kernel's: the walk and A as wave-wide scans (in-row Hillis-Steele stages,
 *               then the row carries, then the carry between the two register slots), the four
 *               chain sums as lane partials over slots and the 64-lane xor butterfly; detmath;
 *   sv_ncp_ref  the reference's: the walk and A in sequence, sums left to right; libm. */
#include <math.h>
#include <string.h>
#include "exmc_detmath.h"

#define T 100
#define D (T + 2)
#define W 64          /* lanes of the chain group */
#define NS 2          /* register slots per lane: dimension i in slot i / 64 of lane i % 64 */

static double f32r(double x) { return (double)(float)x; }
static double ex(double x, int mm) { return mm ? exmc_exp(x) : exp(x); }
static double lg(double x, int mm) { return mm ? exmc_log(x) : log(x); }
static double clamp200(double z) { return fmax(-200.0, fmin(z, 200.0)); }

static const double LANCZOS[9] = {0.99999999999980993,  676.5203681218851,     -1259.1392167224028,
                                  771.32342877765313,   -176.61502916214059,   12.507343278686905,
                                  -0.13857109526572012, 9.9843695780195716e-6, 1.5056327351493116e-7};

/* math.ex:27-52, value and derivative (the kernel's lanczos_pair_d adds the terms in this order) */
static double lanczos(double x, int mm, double* dx) {
  const double half_log_2pi = f32r(0.5 * log(2.0 * M_PI));
  const double t = x + 6.5;
  double ag = f32r(LANCZOS[0]), dag = 0.0;
  for (int i = 1; i < 9; i++) {
    const double den = x + (double)(i - 1) * 1.0;
    const double term = f32r(LANCZOS[i]) / den;
    ag = ag + term;
    dag = dag - term / den;
  }
  const double lt = lg(t, mm);
  *dx = ((lt + (x - 0.5) / t) - 1.0) + dag / ag;
  return ((half_log_2pi + (x - 0.5) * lt) - t) + lg(ag, mm);
}

/* ---- the kernel's scans over one 64-lane slot (exmc_device.hpp wave_scan_fwd / wave_scan_bwd) */
static void scan_fwd_slot(double* v) {
  double n[W], t[W], t2[W];
  for (int d = 1; d < 16; d <<= 1) {          /* row_shr:d */
    for (int l = 0; l < W; l++) n[l] = ((l & 15) >= d) ? v[l] + v[l - d] : v[l];
    memcpy(v, n, sizeof n);
  }
  for (int l = 0; l < W; l++) t[l] = v[(l & ~15) + 15];                  /* row totals */
  for (int l = 0; l < W; l++) {                                          /* rows 1, 3 += row below */
    const double p = t[l ^ 16];
    if (l & 16) v[l] = v[l] + p;
    t2[l] = t[l] + p;
  }
  for (int l = 0; l < W; l++)                                            /* rows 2, 3 += rows 0 + 1 */
    if (l & 32) v[l] = v[l] + t2[l ^ 32];
}

static void scan_bwd_slot(double* v) {
  double n[W], t[W], t2[W];
  for (int d = 1; d < 16; d <<= 1) {          /* row_shl:d */
    for (int l = 0; l < W; l++) n[l] = ((l & 15) + d < 16) ? v[l] + v[l + d] : v[l];
    memcpy(v, n, sizeof n);
  }
  for (int l = 0; l < W; l++) t[l] = v[l & ~15];                         /* row totals */
  for (int l = 0; l < W; l++) {                                          /* rows 0, 2 += row above */
    const double p = t[l ^ 16];
    if (!(l & 16)) v[l] = v[l] + p;
    t2[l] = t[l] + p;
  }
  for (int l = 0; l < W; l++)                                            /* rows 0, 1 += rows 2 + 3 */
    if (!(l & 32)) v[l] = v[l] + t2[l ^ 32];
}

/* x[NS * W] in slot-major order (x[k * 64 + l] = slot k of lane l = dimension k * 64 + l) */
static void scan_fwd(double* x) {
  for (int k = 0; k < NS; k++) scan_fwd_slot(x + k * W);
  for (int k = 1; k < NS; k++) {
    const double carry = x[(k - 1) * W + W - 1];
    for (int l = 0; l < W; l++) x[k * W + l] = x[k * W + l] + carry;
  }
}
static void scan_bwd(double* x) {
  for (int k = 0; k < NS; k++) scan_bwd_slot(x + k * W);
  for (int k = NS - 2; k >= 0; k--) {
    const double carry = x[(k + 1) * W];
    for (int l = 0; l < W; l++) x[k * W + l] = x[k * W + l] + carry;
  }
}

/* group_sum_slots / rs64_allsum4: lane partials over the slots (dimensions < D), xor butterfly */
static double lane_sum64(const double* v) {
  double part[W], nxt[W];
  for (int l = 0; l < W; l++) {
    double acc = 0.0;
    for (int i = l; i < D; i += W) acc = acc + v[i];
    part[l] = acc;
  }
  for (int m = 1; m < W; m <<= 1) {
    for (int l = 0; l < W; l++) nxt[l] = part[l] + part[l ^ m];
    memcpy(part, nxt, sizeof part);
  }
  return part[0];
}
static double seq_sum(const double* v) {
  double acc = 0.0;
  for (int i = 0; i < D; i++) acc = acc + v[i];
  return acc;
}

/* dev = 1: the kernel's order and detmath; dev = 0: the reference's order and libm */
static double sv_ncp(const double* r, const double* q, double* g, int dev) {
  const int mm = dev;
  const double tiny = f32r(1.0e-30);
  const double lam_s = 50.0, lam_n = f32r(0.1);
  const double zs = clamp200(q[T]), zn = clamp200(q[T + 1]);
  const double sigma = ex(zs, mm), nu = ex(zn, mm);
  const double ss = fmax(sigma, tiny), sdf = fmax(nu, tiny);
  const double t_sigma = (f32r(log(lam_s)) - lam_s * sigma) + zs;
  const double t_nu = (f32r(log(lam_n)) - lam_n * nu) + zn;
  const double hp1 = (sdf + 1.0) / 2.0, h = sdf / 2.0;
  double d1, d0;
  const double lg1 = lanczos(hp1, mm, &d1), lg0 = lanczos(h, mm, &d0);
  const double An = (lg1 - lg0) - 0.5 * lg(sdf * f32r(M_PI), mm);
  const double dAn = (0.5 * d1 - 0.5 * d0) - 0.5 / sdf;
  /* Normal(s_1; 0.0, sigma) and Normal(z; 0.0, 1.0): z / 1.0 = z, log_term = log(2pi)_f32 + 2 log(1.0) */
  const double cn = f32r(log(f32r(2.0 * M_PI))) + 2.0 * lg(ss, mm);
  const double c1 = f32r(log(f32r(2.0 * M_PI))) + 2.0 * lg(1.0, mm);
  const double e1 = (q[0] - 0.0) / ss;
  double x[NS * W], s[NS * W], a[NS * W], P[NS * W], LL[NS * W], ZA[NS * W], DN[NS * W];
  for (int i = 0; i < NS * W; i++) x[i] = (i == 0) ? q[0] : ((i < T) ? sigma * q[i] : 0.0);
  memcpy(s, x, sizeof s);
  if (dev) {
    scan_fwd(s);
  } else {
    for (int t = 1; t < T; t++) s[t] = s[t - 1] + s[t];
  }
  for (int i = 0; i < NS * W; i++) {
    P[i] = LL[i] = ZA[i] = DN[i] = a[i] = 0.0;
    if (i >= T) continue;
    const double z = r[i] * ex(-s[i], mm);
    const double w = (z * z) / sdf;
    const double l = lg(1.0 + w, mm);
    const double wr = w / (1.0 + w);
    P[i] = (i == 0) ? (-0.5 * (e1 * e1 + cn)) : (-0.5 * (q[i] * q[i] + c1));
    LL[i] = (An - s[i]) - hp1 * l;
    DN[i] = (dAn - 0.5 * l) + (hp1 * wr) / sdf;
    a[i] = -1.0 + (sdf + 1.0) * wr;          /* dL/ds_t */
  }
  if (dev) {
    scan_bwd(a);
  } else {
    double nxt = 0.0;
    for (int t = T - 1; t >= 0; t--) { a[t] = a[t] + nxt; nxt = a[t]; }
  }
  g[0] = a[0] + (-(e1 / ss));
  ZA[0] = e1 * e1 - 1.0;
  for (int t = 1; t < T; t++) {
    g[t] = (-q[t]) + sigma * a[t];
    ZA[t] = x[t] * a[t];
  }
  const double sp = dev ? lane_sum64(P) : seq_sum(P);
  const double sl = dev ? lane_sum64(LL) : seq_sum(LL);
  const double sz = dev ? lane_sum64(ZA) : seq_sum(ZA);
  const double sn = dev ? lane_sum64(DN) : seq_sum(DN);
  const int in_s = (q[T] > -200.0) && (q[T] < 200.0);
  const int in_n = (q[T + 1] > -200.0) && (q[T + 1] < 200.0);
  g[T] = in_s ? ((sz - lam_s * sigma) + 1.0) : 0.0;
  g[T + 1] = in_n ? ((sn * nu - lam_n * nu) + 1.0) : 0.0;
  return ((t_sigma + t_nu) + sp) + sl;
}

double sv_ncp_dev(const double* r, const double* q, double* g) { return sv_ncp(r, q, g, 1); }
double sv_ncp_ref(const double* r, const double* q, double* g) { return sv_ncp(r, q, g, 0); }
/* the walk of a point, in either order (s[T]) */
void sv_ncp_walk(const double* q, double* out, int dev) {
  double s[NS * W];
  const double sigma = dev ? exmc_exp(clamp200(q[T])) : exp(clamp200(q[T]));
  for (int i = 0; i < NS * W; i++) s[i] = (i == 0) ? q[0] : ((i < T) ? sigma * q[i] : 0.0);
  if (dev) {
    scan_fwd(s);
  } else {
    for (int t = 1; t < T; t++) s[t] = s[t - 1] + s[t];
  }
  memcpy(out, s, sizeof(double) * T);
}
