"""Exact laws for the random draws the device makes, and the acceptance functions that hold a sample to
them. TEST INFRASTRUCTURE: the product never imports it.

Three parts.

Reference CDFs, survival functions and quantiles of Normal, Student-t (any df > 0), Gamma(shape, rate) and
Bernoulli, from scipy (tests/test_exact_distributions.py holds them to mpmath at 50 digits).

Acceptance functions. Each returns (statistic, bound); the caller asserts statistic <= bound (or, for
tail_count, lo <= count <= hi). Every bound follows from the sample size n and a significance level alpha
passed in, never from a sample:
  ks                 sup |F_n - F| against the Dvoretzky-Kiefer-Wolfowitz radius sqrt(ln(2 / alpha) / (2 n))
                     (Massart 1990: P(D > r) <= 2 exp(-2 n r^2) for every n, so the level is exact, not
                     asymptotic)
  chi2_equiprobable  Pearson's statistic over `bins` cells cut at exact quantiles, against
                     chi2.isf(alpha, bins - 1)
  tail_count         the number of values above each threshold against the exact two-sided binomial limits
                     of Binomial(n, sf(threshold)), alpha split over the thresholds
  z_mean, chi2_var   the sample mean and variance, standardised with the exact moments, against the
                     two-sided normal quantile (central limit: the fourth moment must exist, and for
                     chi2_var the level is nominal where the eighth does not)
  sign_count, pearson_pooled, binomial_limits, hoeffding_radius, correlation_bound   the same idea
A file of tests spends a family-wise level FAMILY = 1e-6, split by Bonferroni over its assertions
(`level(m)`); its seeds are fixed, so the outcome is deterministic.

Plain numpy samplers, written from the papers and not from tests/predictive_statement.py:
  Marsaglia, Tsang: A simple method for generating gamma variables, ACM TOMS 26 (2000), section 3 (d = a -
  1/3, c = 1 / sqrt(9 d), v = (1 + c x)^3, accept log u < x^2 / 2 + d - d v + d log v) and its section 6
  note for a < 1 (gamma(a) = gamma(a + 1) u^(1/a)); Student's t as z / sqrt(chi2 / df) with chi2 =
  gamma(df / 2, rate 1/2). They show that the references alone stay inside every bound at the sizes the
  GPU tests use, and their keyword arguments carry the mutants of the teeth test."""
import math

import numpy as np
from scipy import special, stats

FAMILY = 1.0e-6
ZIG_R = 3.6541528853610088     # where the 256-layer ziggurat's layer 0 hands over to its tail sampler


def level(m, family=FAMILY):
    """Bonferroni: the level of one of m assertions that together spend `family`"""
    return family / m


# ---- reference laws ------------------------------------------------------------------------------------------
def normal_cdf(x, loc=0.0, scale=1.0):
    return special.ndtr((np.asarray(x, dtype=np.float64) - loc) / scale)


def normal_sf(x, loc=0.0, scale=1.0):
    return special.ndtr(-(np.asarray(x, dtype=np.float64) - loc) / scale)


def normal_ppf(p, loc=0.0, scale=1.0):
    return loc + scale * special.ndtri(np.asarray(p, dtype=np.float64))


def abs_normal_sf(x):
    """P(|z| > x) of a standard normal z, x >= 0"""
    return 2.0 * special.ndtr(-np.asarray(x, dtype=np.float64))


def t_cdf(x, df):
    return stats.t.cdf(np.asarray(x, dtype=np.float64), df)


def t_sf(x, df):
    return stats.t.sf(np.asarray(x, dtype=np.float64), df)


def t_ppf(p, df):
    return stats.t.ppf(np.asarray(p, dtype=np.float64), df)


def t_var(df):
    return df / (df - 2.0)


def t_excess_kurtosis(df):
    return 6.0 / (df - 4.0)


def gamma_cdf(x, shape, rate=1.0):
    return special.gammainc(shape, rate * np.asarray(x, dtype=np.float64))


def gamma_sf(x, shape, rate=1.0):
    return special.gammaincc(shape, rate * np.asarray(x, dtype=np.float64))


def gamma_ppf(p, shape, rate=1.0):
    return special.gammaincinv(shape, np.asarray(p, dtype=np.float64)) / rate


def bernoulli_cdf(x, p):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x < 0.0, 0.0, np.where(x < 1.0, 1.0 - p, 1.0))


# ---- bounds --------------------------------------------------------------------------------------------------
def dkw_radius(n, alpha):
    return math.sqrt(math.log(2.0 / alpha) / (2.0 * n))


def hoeffding_radius(n, alpha):
    """P(|mean of n values in [0, 1] - its expectation| > r) <= 2 exp(-2 n r^2) = alpha"""
    return math.sqrt(math.log(2.0 / alpha) / (2.0 * n))


def normal_bound(alpha):
    """the two-sided standard normal quantile: P(|z| > bound) = alpha"""
    return float(stats.norm.isf(alpha / 2.0))


def binomial_limits(n, p, alpha):
    """(lo, hi) with P(K < lo) <= alpha / 2 and P(K > hi) <= alpha / 2 for K ~ Binomial(n, p); p may be an
    array. At p = 0 both are 0, at p = 1 both are n."""
    p = np.asarray(p, dtype=np.float64)
    lo = stats.binom.ppf(alpha / 2.0, n, p)
    hi = stats.binom.isf(alpha / 2.0, n, p)
    return np.maximum(lo, 0.0), np.minimum(hi, float(n))


def poisson_limits(mean, alpha):
    """the same for a Poisson count (a rare event pooled over cells of different probability)"""
    return float(stats.poisson.ppf(alpha / 2.0, mean)), float(stats.poisson.isf(alpha / 2.0, mean))


# ---- acceptance functions ------------------------------------------------------------------------------------
def ks(x, cdf, alpha):
    """(sup_x |F_n(x) - cdf(x)|, the DKW radius). x is flattened; it must hold no NaN."""
    v = np.sort(np.asarray(x, dtype=np.float64), axis=None)
    n = v.size
    assert n > 0 and not np.isnan(v[-1]), "ks: empty sample or NaN"
    F = np.asarray(cdf(v), dtype=np.float64)
    i = np.arange(1, n + 1, dtype=np.float64)
    d = max(float(np.max(i / n - F)), float(np.max(F - (i - 1.0) / n)))
    return d, dkw_radius(n, alpha)


def chi2_equiprobable(x, ppf, bins, alpha):
    """(Pearson's statistic over `bins` equiprobable cells cut at ppf(k / bins), chi2.isf(alpha, bins - 1))"""
    v = np.asarray(x, dtype=np.float64).ravel()
    edges = np.asarray(ppf(np.arange(1, bins, dtype=np.float64) / bins), dtype=np.float64)
    counts = np.bincount(np.searchsorted(edges, v, side="right"), minlength=bins)
    e = v.size / float(bins)
    return float(np.sum((counts - e) ** 2) / e), float(stats.chi2.isf(alpha, bins - 1))


def tail_count(x, thresholds, sf, alpha):
    """(counts of x > t per threshold t, (lo, hi) arrays): the exact two-sided binomial limits of
    Binomial(n, sf(t)) at alpha / len(thresholds) each"""
    v = np.asarray(x, dtype=np.float64).ravel()
    th = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
    counts = np.array([int(np.count_nonzero(v > t)) for t in th])
    lo, hi = binomial_limits(v.size, np.asarray(sf(th), dtype=np.float64), alpha / th.size)
    return counts, (lo, hi)


def within(counts, limits):
    lo, hi = limits
    return bool(np.all(counts >= lo) and np.all(counts <= hi))


def sign_count(x, alpha):
    """(the number of x > 0, (lo, hi)) for a law that is symmetric about 0 and has no atom there"""
    v = np.asarray(x, dtype=np.float64).ravel()
    return int(np.count_nonzero(v > 0.0)), binomial_limits(v.size, 0.5, alpha)


def z_mean(x, mean, sd, alpha):
    """(|sample mean - mean| in standard errors, the two-sided normal quantile)"""
    v = np.asarray(x, dtype=np.float64).ravel()
    return abs(float(v.mean()) - mean) / (sd / math.sqrt(v.size)), normal_bound(alpha)


def chi2_var(x, var, excess_kurtosis, alpha):
    """(|s^2 / var - 1| in standard errors, the two-sided normal quantile). Var(s^2) = var^2 (2 + excess
    kurtosis) / n to first order; for a normal sample this is the chi-square (n - 1) law's own normal limit,
    and n here is 10^5 and more."""
    v = np.asarray(x, dtype=np.float64).ravel()
    s2 = float(v.var(ddof=1))
    return abs(s2 / var - 1.0) / math.sqrt((2.0 + excess_kurtosis) / v.size), normal_bound(alpha)


def normal_var_limits(n, alpha):
    """(lo, hi) for s^2 / sigma^2 of n normal values: (n - 1) s^2 / sigma^2 is chi-square (n - 1), exactly"""
    return float(stats.chi2.ppf(alpha / 2.0, n - 1)) / (n - 1.0), float(stats.chi2.isf(alpha / 2.0, n - 1)) / (n - 1.0)


def pearson_pooled(k, n, p, alpha):
    """(sum over cells of (k_i - n p_i)^2 / (n p_i (1 - p_i)), chi2.isf(alpha, cells)): independent binomial
    counts k_i of n trials each. Cells with p_i of 0 or 1 carry no variance and must be exact; they are
    not part of the sum (the caller asserts them)."""
    k, p = np.asarray(k, dtype=np.float64), np.asarray(p, dtype=np.float64)
    live = (p > 0.0) & (p < 1.0)
    stat = float(np.sum((k[live] - n * p[live]) ** 2 / (n * p[live] * (1.0 - p[live]))))
    return stat, float(stats.chi2.isf(alpha, int(live.sum())))


def correlation_bound(n, alpha):
    """the sample correlation r of n independent pairs, one margin normal: r sqrt((n - 2) / (1 - r^2)) is
    Student-t with n - 2 degrees of freedom, exactly. The |r| at which that reaches its two-sided quantile."""
    t = float(stats.t.isf(alpha / 2.0, n - 2))
    return t / math.sqrt(n - 2.0 + t * t)


def correlation(a, b, axis=-1):
    a = a - a.mean(axis=axis, keepdims=True)
    b = b - b.mean(axis=axis, keepdims=True)
    return (a * b).sum(axis=axis) / np.sqrt((a * a).sum(axis=axis) * (b * b).sum(axis=axis))


# ---- plain numpy samplers (and, through their keyword arguments, the mutants) ----------------------------------
def np_gamma(rng, shape, rate, n, third=1.0 / 3.0, boost_exponent=None):
    """n Gamma(shape, rate) variates by Marsaglia-Tsang. The mutants: `third` (the paper's 1/3 in d = a -
    1/3), `boost_exponent` (the paper's 1 / a in gamma(a) = gamma(a + 1) u^(1 / a))."""
    boost = shape < 1.0
    a = shape + 1.0 if boost else shape
    d = a - third
    c = 1.0 / math.sqrt(9.0 * d)
    out = np.empty(n)
    have = 0
    while have < n:
        m = int((n - have) * 1.1) + 64
        x = rng.standard_normal(m)
        v = 1.0 + c * x
        u = rng.random(m)
        ok = v > 0.0
        v = np.where(ok, v, 1.0) ** 3
        with np.errstate(divide="ignore"):
            ok &= np.log(u) < 0.5 * x * x + d - d * v + d * np.log(v)
        g = (d * v[ok])[:n - have]
        out[have:have + g.size] = g
        have += g.size
    out /= rate
    if boost:
        e = 1.0 / shape if boost_exponent is None else boost_exponent(shape)
        out *= rng.random(n) ** e
    return out


def np_student_t(rng, df, n, chi2_rate=0.5, scale=1.0, **gamma_mutant):
    """n Student-t variates z / sqrt(chi2 / df), chi2 = Gamma(df / 2, rate 1/2)"""
    z = rng.standard_normal(n)
    chi2 = np_gamma(rng, df / 2.0, chi2_rate, n, **gamma_mutant)
    return scale * z / np.sqrt(chi2 / df)


def np_normal(rng, n, clamp_tail=False, moved_mass=None):
    """n standard normals. The mutants: clamp_tail puts every |z| > ZIG_R at +-ZIG_R (a ziggurat whose tail
    sampler returns its start); moved_mass = (bins, k, share) moves `share` of equiprobable bin k's
    variates into bin k + 1 (mirrored about the edge between them)."""
    z = rng.standard_normal(n)
    if clamp_tail:
        z = np.clip(z, -ZIG_R, ZIG_R)
    if moved_mass is not None:
        bins, k, share = moved_mass
        lo, edge = normal_ppf(k / bins), normal_ppf((k + 1.0) / bins)
        pick = (z >= lo) & (z < edge) & (rng.random(n) < share)
        z[pick] = edge + (edge - z[pick]) * 0.5       # stays inside bin k + 1, which is wider than half of bin k
    return z


def np_bernoulli(rng, p, n, inclusive=False, uniforms=None):
    """n Bernoulli(p) replicates 1.0 if u < p else 0.0. The mutant: inclusive compares u <= p. `uniforms`
    replaces the generator's (a stream that holds u = 0.0 shows the difference at p = 0)."""
    u = rng.random(n) if uniforms is None else np.asarray(uniforms, dtype=np.float64)
    return ((u <= p) if inclusive else (u < p)).astype(np.float64)


# ---- the working points of the GPU tests -----------------------------------------------------------------------
# tests/test_exact_distributions.py shows on the CPU, with the samplers above, that at exactly these sizes and
# levels the correct samplers pass and the listed wrong ones do not.
PRED_ASSERTIONS = 80                      # tests/test_gpu_predictive_distributions.py spends FAMILY over these
PRED_ALPHA = level(PRED_ASSERTIONS)
N_RADON = 919 * 280 * 40                  # normal replicates of one radon call
NORMAL_BINS = 1024
NORMAL_TAILS = (3.0, ZIG_R, 4.5)
T_DRAWS, T_DATUMS = 250, 100
T_DF = (0.3, 1.0, 2.0, 10.0, 200.0, math.exp(200.0))
# chains per df group: 66 gives 1.65e6 variates; at df = 0.3 a scale that is 2 % off moves the CDF by 1.9e-3
# only, inside the DKW radius of 1.65e6 variates (2.4e-3), so that group has four times the chains
T_CHAINS = (264, 66, 66, 66, 66, 66)
T_TAIL_P = 1.0e-4
BERN_DATUMS, BERN_N = 500, 130 * 160      # per-datum replicates of the logistic case


def t_group_n(k):
    return T_CHAINS[k] * T_DRAWS * T_DATUMS
