"""Posterior predictive checks on the device (predictive.ppc, the fused ppc kernel) against values known in
closed form. The trace is one parameter point, the same for every draw of every chain, so the n = S C
replicated data sets are i.i.d. and every number ppc returns estimates a quantity with an exact value:
  per datum   p_lt_i = P(yrep_i < y_i), p_eq_i = P(yrep_i = y_i), pit_i = p_lt_i + p_eq_i / 2, each a share of n
              independent indicators: within the Hoeffding radius at the level split over the N datums;
              mean_i and var_i against the family's moments (normal kinds: the mean is normal and
              (n - 1) var_i / sigma_i^2 chi-square exactly; t at df = 10: central limit, nominal level)
  p_value     the share of data sets with T(yrep) >= T(y): a binomial count about the exact probability,
              mean: normal (normal kinds); max: 1 - prod F_i(t_obs); min: prod (1 - F_i(t_obs-)); var (simple,
              N = 12): (N - 1) T_var / sigma^2 is chi-square (N - 1)
The observations of simple and eight_schools are constructed so that the exact p-values sit at 0.05, 0.5 and
0.95 (CASES: a data set in the middle, one shifted up, one down, a wide and a narrow one; twelve values with
so small a variance cannot also have extremes at 0.05 and 0.95, the narrow one has them at 0.2 and 0.8). The parameters of the laws are computed in plain numpy from the data blob
(tests/test_gpu_predictive_distributions.py); nothing compares the device with the statement. Every call has
200 or more chains: four blocks of PPC_BLOCK = 64, the last partial.

Level: 1e-6 over at most 128 statistical assertions (simple 5 x 9, eight_schools 5 x 8, sv 7, radon 8, logistic
3: 103), 7.8e-9 each, split again over the datums where an assertion covers all of them. Seeds are fixed."""
import math

import numpy as np
import pytest
from scipy import optimize, stats

import exact_distributions as E
import test_gpu_predictive_distributions as PD
from exmc_amd import _lib, models, sampler
from exmc_amd import predictive as PP

pytestmark = pytest.mark.gpu

A = E.level(128)
# exact p-values (mean, min, max, var) the observations are built for; p_min is small where the smallest
# observation is high, p_var is small where the observations are spread out
CASES = dict(mid=(0.5, 0.5, 0.5, 0.5), up=(0.05, 0.05, 0.05, 0.5), down=(0.95, 0.95, 0.95, 0.5),
             wide=(0.5, 0.95, 0.05, 0.05), narrow=(0.5, 0.2, 0.8, 0.95))


def _ppc(spec, q, S, Cn, seed):
    """predictive.ppc at the one point q [d], S draws of Cn chains"""
    import torch
    assert _lib.PPC_BLOCK == 64 and Cn > 3 * 64 and Cn % 64 != 0
    cm = sampler.compile(spec)
    try:
        x = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(q[None, :, None], (S, q.size, Cn)))).cuda()
        return PP.ppc(cm, x, seed=seed)
    finally:
        cm.close()


def _shares(out, n, N, p_lt, p_eq, what):
    """p_lt, p_eq and pit of every datum within the Hoeffding radius, the level split over the N datums"""
    r = E.hoeffding_radius(n, A / N)
    dev = [float(np.max(np.abs(out["p_lt"] - p_lt))), float(np.max(np.abs(out["p_eq"] - p_eq))),
           float(np.max(np.abs(out["pit"] - (p_lt + 0.5 * p_eq))))]
    print("%s n=%d: max |p_lt - exact| %.3g, |p_eq - exact| %.3g, |pit - exact| %.3g <= %.3g" % ((what, n) + tuple(dev) + (r,)))
    assert dev[0] <= r
    assert dev[1] <= r
    assert dev[2] <= r


def _normal_moments(out, n, N, loc, scale, what):
    zm = np.abs(out["mean"] - loc) / (scale / math.sqrt(n))
    zb = E.normal_bound(A / N)
    ratio = out["var"] / scale ** 2
    lo, hi = E.normal_var_limits(n, A / N)
    print("%s: max |mean_i - loc_i| %.2f <= %.2f sigma; var_i / sigma_i^2 in %.5f..%.5f inside %.5f..%.5f"
          % (what, zm.max(), zb, ratio.min(), ratio.max(), lo, hi))
    assert zm.max() <= zb, int(np.argmax(zm))
    assert lo <= ratio.min() and ratio.max() <= hi


def _p_value(out, stat, n, exact, t_want, what):
    """the count of data sets at or above t_obs inside the exact binomial limits"""
    assert math.isclose(out["t_obs"][stat], t_want, rel_tol=1e-12, abs_tol=1e-12), (stat, out["t_obs"][stat], t_want)
    k = out["p_value"][stat] * n
    assert abs(k - round(k)) < 1e-6
    lo, hi = E.binomial_limits(n, exact, A)
    print("%s p_value[%s] = %.5f, exact %.5f (count %d in %d..%d)" % (what, stat, out["p_value"][stat], exact, round(k), lo, hi))
    assert lo <= round(k) <= hi, stat


def _max_min_exact(y, cdf_i):
    """P(max yrep >= max y) = 1 - prod F_i(max y); P(min yrep >= min y) = prod (1 - F_i(min y)) (continuous laws)"""
    return 1.0 - float(np.prod(cdf_i(y.max()))), float(np.prod(1.0 - cdf_i(y.min())))


def _observations(N, cdf_i, mean_law, targets, var_target=None, sigma=None):
    """N observations whose exact p-values are the targets (mean, min, max[, var]): the extremes solve their
    closed forms, the other N - 2 values are a + b w with w fixed, (a, b) solved for the mean (and variance)"""
    t_mean, t_min, t_max = targets
    span = (-1e3, 1e3)
    y_max = optimize.brentq(lambda t: 1.0 - np.prod(cdf_i(t)) - t_max, *span, xtol=1e-13)
    y_min = optimize.brentq(lambda t: np.prod(1.0 - cdf_i(t)) - t_min, *span, xtol=1e-13)
    want_mean = mean_law.isf(t_mean)
    w = np.linspace(-1.0, 1.0, N - 2)
    a = (N * want_mean - y_max - y_min) / (N - 2)
    b = 0.0
    if var_target is not None:
        want_var = sigma ** 2 * stats.chi2.isf(var_target, N - 1) / (N - 1)
        rest = (N - 1) * want_var - (y_max - want_mean) ** 2 - (y_min - want_mean) ** 2 - (N - 2) * (a - want_mean) ** 2
        assert rest > 0.0, "no such data set"
        b = math.sqrt(rest / float(np.sum(w * w)))
    else:
        b = 0.25 * min(y_max - a, a - y_min)
    y = np.concatenate([[y_min], a + b * w, [y_max]])
    assert y_min < y[1:-1].min() and y[1:-1].max() < y_max, "no such data set"
    return y


# ---- simple: N = 12 observations of our choosing, all four statistics in closed form --------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_simple_all_four_statistics(case, hip):
    N, S, Cn = 12, 2000, 200
    mu, sigma = 2.0, 1.3
    tg = CASES[case]                                          # mean, min, max, var
    rot = list(CASES).index(case)
    cdf_i = lambda t: np.full(N, float(E.normal_cdf(t, mu, sigma)))   # noqa: E731
    y = _observations(N, cdf_i, stats.norm(mu, sigma / math.sqrt(N)), tg[:3], var_target=tg[3], sigma=sigma)
    rng = np.random.default_rng(600 + rot)
    y = y[rng.permutation(N)]
    spec = models.simple(y=list(y))
    q = np.array([mu, math.log(sigma)])
    loc, scale = PD.simple_params(spec.data, q[None])
    n = S * Cn
    out = _ppc(spec, q, S, Cn, seed=90 + rot)
    what = "simple[%s]" % case
    _shares(out, n, N, E.normal_cdf(y, loc[0], scale[0]), np.zeros(N), what)
    _normal_moments(out, n, N, np.full(N, loc[0]), np.full(N, scale[0]), what)
    p_max, p_min = _max_min_exact(y, lambda t: E.normal_cdf(t, loc[0], scale[0]) * np.ones(N))
    exact = dict(mean=float(E.normal_sf(y.mean(), loc[0], scale[0] / math.sqrt(N))),
                 var=float(stats.chi2.sf((N - 1) * y.var(ddof=1) / scale[0] ** 2, N - 1)), min=p_min, max=p_max)
    for k, t in zip(("mean", "min", "max", "var"), tg):
        assert abs(exact[k] - t) < 1e-6, (k, exact[k], t)     # the observations sit where they were put
    t_obs = dict(mean=y.mean(), var=y.var(ddof=1), min=y.min(), max=y.max())
    for k in ("mean", "var", "min", "max"):
        _p_value(out, k, n, exact[k], t_obs[k], what)


# ---- eight_schools: heteroscedastic normals ------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_eight_schools_mean_min_max(case, hip):
    N, S, Cn = 8, 2500, 200
    sigma = np.array(models.EIGHT_SCHOOLS_SIGMA)
    q = np.array([4.0, math.log(3.0), 0.5, -1.2, 0.3, 2.0, -0.4, 0.0, 1.1, -2.2])
    loc = q[0] + 3.0 * q[2:]
    tg = CASES[case][:3]                                      # mean, min, max
    rot = list(CASES).index(case)
    cdf_i = lambda t: E.normal_cdf(t, loc, sigma)   # noqa: E731
    mean_law = stats.norm(loc.mean(), math.sqrt(np.sum(sigma ** 2)) / N)
    y = _observations(N, cdf_i, mean_law, tg)
    y = y[np.random.default_rng(610 + rot).permutation(N)]
    spec = models.eight_schools(y=list(y), sigma=list(sigma))
    loc2, scale = PD.eight_schools_params(spec.data, q[None])
    assert np.allclose(loc2[:, 0], loc, rtol=1e-14) and np.array_equal(scale, sigma)
    n = S * Cn
    out = _ppc(spec, q, S, Cn, seed=93 + rot)
    what = "eight_schools[%s]" % case
    _shares(out, n, N, E.normal_cdf(y, loc2[:, 0], scale), np.zeros(N), what)
    _normal_moments(out, n, N, loc2[:, 0], scale, what)
    p_max, p_min = _max_min_exact(y, lambda t: E.normal_cdf(t, loc2[:, 0], scale))
    exact = dict(mean=float(mean_law.sf(y.mean())), min=p_min, max=p_max)
    for k, t in zip(("mean", "min", "max"), tg):
        assert abs(exact[k] - t) < 1e-6, (k, exact[k], t)
    for k, t_obs in (("mean", y.mean()), ("min", y.min()), ("max", y.max())):
        _p_value(out, k, n, exact[k], t_obs, what)


# ---- sv: Student-t at df = 10 ------------------------------------------------------------------------------------------
def test_sv_student_t_at_df_10(hip):
    N, S, Cn, df = 100, 250, 200, 10.0
    rng = np.random.default_rng(620)
    s = rng.uniform(-3.0, 1.0, size=N)
    q = np.concatenate([s, [math.log(0.15), math.log(df)]])
    s2, df2 = PD.sv_params(models.SV, q[None])
    assert np.array_equal(s2[:, 0], s) and math.isclose(df2[0], df, rel_tol=1e-14)
    scale = np.exp(s)
    cdf_i = lambda t: E.t_cdf(t / scale, df)   # noqa: E731
    # returns at scattered quantiles of their own laws; the largest and the smallest put at p-values 0.05 and 0.95
    r = scale * E.t_ppf(rng.uniform(0.02, 0.98, size=N), df)
    hi = optimize.brentq(lambda t: 1.0 - np.prod(cdf_i(t)) - 0.05, 0.0, 1e3, xtol=1e-13)
    lo = optimize.brentq(lambda t: np.prod(1.0 - cdf_i(t)) - 0.95, -1e3, 0.0, xtol=1e-13)
    r = np.clip(r, 0.9 * lo, 0.9 * hi)
    r[int(np.argmax(scale))], r[int(np.argsort(scale)[-2])] = hi, lo
    assert r.max() == hi and r.min() == lo
    spec = models.sv(list(r))
    n = S * Cn
    out = _ppc(spec, q, S, Cn, seed=96)
    _shares(out, n, N, cdf_i(r), np.zeros(N), "sv")
    zm = np.abs(out["mean"]) / (scale * math.sqrt(E.t_var(df) / n))
    zv = np.abs(out["var"] / (scale ** 2 * E.t_var(df)) - 1.0) / math.sqrt((2.0 + E.t_excess_kurtosis(df)) / n)
    zb = E.normal_bound(A / N)
    print("sv: max |mean_i| %.2f, max |var_i / exact - 1| %.2f <= %.2f standard errors" % (zm.max(), zv.max(), zb))
    assert zm.max() <= zb
    assert zv.max() <= zb
    p_max, p_min = _max_min_exact(r, cdf_i)
    assert abs(p_max - 0.05) < 1e-6 and abs(p_min - 0.95) < 1e-6
    _p_value(out, "max", n, p_max, r.max(), "sv")
    _p_value(out, "min", n, p_min, r.min(), "sv")


# ---- radon: 919 normal datums, the committed observations ---------------------------------------------------------------
def test_radon_per_datum_and_whole_data_set(hip):
    S, Cn = 30, 1090
    spec = models.radon()
    N = 919
    y = spec.data[2 * 85 + 1 + N:]
    q0 = np.asarray(spec.to_unconstrained(spec.default_init))
    q = q0 + 0.2 * np.random.default_rng(630).normal(size=spec.d)
    q[85], q[86], q[87], q[88], q[89] = 1.4, 0.7, math.log(0.4), math.log(0.75), -0.7
    loc, scale = PD.radon_params(spec.data, q[None])
    loc, scale = loc[:, 0], np.full(N, scale[0])
    n = S * Cn
    out = _ppc(spec, q, S, Cn, seed=97)
    _shares(out, n, N, E.normal_cdf(y, loc, scale), np.zeros(N), "radon")
    _normal_moments(out, n, N, loc, scale, "radon")
    p_max, p_min = _max_min_exact(y, lambda t: E.normal_cdf(t, loc, scale))
    p_mean = float(E.normal_sf(y.mean(), loc.mean(), scale[0] / math.sqrt(N)))
    assert 1e-3 < p_mean < 1.0 - 1e-3 and 1e-3 < p_max < 1.0 - 1e-3 and 1e-3 < p_min < 1.0 - 1e-3, (p_mean, p_max, p_min)
    _p_value(out, "mean", n, p_mean, y.mean(), "radon")
    _p_value(out, "max", n, p_max, y.max(), "radon")
    _p_value(out, "min", n, p_min, y.min(), "radon")


# ---- logistic: the shares of a discrete law ---------------------------------------------------------------------------------
def test_logistic_shares(hip):
    S, Cn = 60, 1090
    spec = models.logistic()
    N = 500
    y = spec.data[N * 20:]
    assert set(np.unique(y)) == {0.0, 1.0}
    q = np.concatenate([[0.3], 0.3 * np.random.default_rng(640).normal(size=20)])
    p = PD.logistic_p(spec.data, q)
    n = S * Cn
    out = _ppc(spec, q, S, Cn, seed=98)
    # p_eq_i = P(yrep = y_i); p_lt_i = P(yrep = 0) where y_i = 1, else nothing lies below
    _shares(out, n, N, np.where(y == 1.0, 1.0 - p, 0.0), np.where(y == 1.0, p, 1.0 - p), "logistic")
