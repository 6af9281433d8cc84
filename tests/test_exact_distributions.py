"""The exact laws and acceptance functions of tests/exact_distributions.py, on the CPU: the scipy CDFs against
mpmath at 50 digits; the plain numpy samplers inside every bound at the sizes and levels the GPU tests use
(tests/test_gpu_predictive_distributions.py); and teeth: at those sizes and levels every acceptance function
rejects the wrong samplers listed below. Bounds come from n and the level alone.

Level: the acceptance runs here use E.PRED_ALPHA = 1e-6 / 80, the level of one assertion of the GPU file, so
that what passes and what is rejected here is what passes and is rejected there. The assertions of this file
that a correct sampler passes number 45 (normal 6, t 6 x 3 + 3, gamma 5 x 3, Bernoulli 3), fewer than 80: its own
family-wise level is below 1e-6 as well. Seeds are fixed: the outcome is deterministic.

Not claimed (measured, outside the bound by too little or inside it): d = a - 1/4 at df >= 10 (KS distance
2.5e-3 at df = 10 against a radius of 2.4e-3; 7e-4 at df = 200, inside it); u <= p at p = 0 on a generator's own
uniforms (u = 0 has probability 2^-53: no sample shows it; the teeth test hands the sampler a stream that
holds a 0.0 and the limits [0, 0] at p = 0 reject the one replicate of 1.0)."""
import math

import mpmath as mp
import numpy as np
import pytest

import exact_distributions as E

A = E.PRED_ALPHA
CDF_BOUND = 1.0e-9          # the smallest DKW radius used anywhere is 9.6e-4 (n = 1.03e7); three orders below is 1e-6


def _points():
    """200 probabilities from 1e-12 to 1 - 1e-12, evenly spaced in the logit"""
    t = np.linspace(math.log(1e-12), -math.log(1e-12), 200)
    return 1.0 / (1.0 + np.exp(-t))


def _worst(pairs):
    return max(abs(float(a) - float(b)) for a, b in pairs)


def test_normal_cdf_equals_mpmath():
    """measured maximum |scipy - mpmath|: cdf and sf 1.1e-16"""
    mp.mp.dps = 50
    x = E.normal_ppf(_points())
    assert x[0] < -7.0 and x[-1] > 7.0
    ref = [mp.ncdf(mp.mpf(float(v))) for v in x]
    worst = max(_worst(zip(E.normal_cdf(x), ref)), _worst(zip(E.normal_sf(x), [1 - r for r in ref])))
    print("normal: max |scipy - mpmath| = %.3g" % worst)
    assert worst <= CDF_BOUND
    assert _worst(zip(E.normal_cdf(E.normal_ppf(_points())), _points())) <= CDF_BOUND
    assert abs(float(E.abs_normal_sf(E.ZIG_R)) - float(2 * mp.ncdf(-mp.mpf(E.ZIG_R)))) <= 1e-18


def _t_cdf_mp(x, df):
    """regularised incomplete beta: P(T <= x) = 1 - I_w(df / 2, 1 / 2) / 2 for x > 0, w = df / (df + x^2)"""
    x, df = mp.mpf(x), mp.mpf(df)
    tail = mp.betainc(df / 2, mp.mpf(0.5), 0, df / (df + x * x), regularized=True) / 2
    return tail if x < 0 else 1 - tail


@pytest.mark.parametrize("df", E.T_DF, ids=lambda v: "%.3g" % v)
def test_t_cdf_equals_mpmath(df):
    """measured maximum |scipy - mpmath| over cdf and sf: 1.7e-16 at df 0.3, 1, 2, 10, 200; 2.7e-15 at e^200.
    The working precision is 150 digits, 50 to spare: at df = e^200, df / (df + x^2) differs from 1 in the 87th
    digit (at 50 digits mpmath's betainc returns values outside [0, 1] there)."""
    mp.mp.dps = 150
    try:
        p = _points()
        x = E.t_ppf(p, df)
        assert np.all(np.diff(x) > 0)
        ref = [_t_cdf_mp(float(v), df) for v in x]
        worst = max(_worst(zip(E.t_cdf(x, df), ref)), _worst(zip(E.t_sf(x, df), [1 - r for r in ref])))
        print("t(%g): max |scipy - mpmath| = %.3g" % (df, worst))
        assert worst <= CDF_BOUND
        assert _worst(zip(ref, p)) <= CDF_BOUND          # the quantiles
        if df > 1e80:                                    # the clamp of log nu: the normal law to 1 / (4 df)
            assert _worst(zip(ref, [mp.ncdf(mp.mpf(float(v))) for v in x])) <= 1e-80
    finally:
        mp.mp.dps = 50


@pytest.mark.parametrize("shape", [0.15, 0.4, 1.0, 3.0, 100.0])
def test_gamma_cdf_equals_mpmath(shape):
    """measured maximum |scipy - mpmath| over cdf and sf: 4.4e-16 (shape 0.15)"""
    mp.mp.dps = 50
    p = _points()
    x = E.gamma_ppf(p, shape, 0.5)
    ref = [mp.gammainc(mp.mpf(shape), 0, mp.mpf(float(v)) / 2, regularized=True) for v in x]
    worst = max(_worst(zip(E.gamma_cdf(x, shape, 0.5), ref)), _worst(zip(E.gamma_sf(x, shape, 0.5), [1 - r for r in ref])))
    print("gamma(%g): max |scipy - mpmath| = %.3g" % (shape, worst))
    assert worst <= CDF_BOUND
    assert _worst(zip(ref, p)) <= CDF_BOUND


def test_bounds_follow_from_n_and_the_level():
    assert E.dkw_radius(E.N_RADON, A) == math.sqrt(math.log(2.0 / A) / (2.0 * E.N_RADON))
    assert 9.0e-4 < E.dkw_radius(E.N_RADON, A) < 1.0e-3 and 2.3e-3 < E.dkw_radius(E.t_group_n(1), A) < 2.5e-3
    assert CDF_BOUND * 1e3 <= E.dkw_radius(E.N_RADON, A)
    lo, hi = E.binomial_limits(1000, np.array([0.0, 1.0, 0.5]), 1e-6)
    assert lo[0] == hi[0] == 0 and lo[1] == hi[1] == 1000 and 400 < lo[2] < 500 < hi[2] < 600
    from scipy import stats
    assert stats.binom.cdf(lo[2] - 1, 1000, 0.5) <= 5e-7 < stats.binom.cdf(lo[2], 1000, 0.5)
    assert stats.binom.sf(hi[2], 1000, 0.5) <= 5e-7 < stats.binom.sf(hi[2] - 1, 1000, 0.5)
    assert abs(E.normal_bound(0.05) - 1.959964) < 1e-6


# ---- the normal law at the size of the radon call -------------------------------------------------------------
def _normal_verdicts(z):
    d, r = E.ks(z, E.normal_cdf, A)
    x2, xb = E.chi2_equiprobable(z, E.normal_ppf, E.NORMAL_BINS, A)
    tc, lim = E.tail_count(np.abs(z), E.NORMAL_TAILS, E.abs_normal_sf, A)
    sg, slim = E.sign_count(z, A)
    zm, zb = E.z_mean(z, 0.0, 1.0, A)
    cv, cb = E.chi2_var(z, 1.0, 0.0, A)
    return dict(ks=d <= r, chi2=x2 <= xb, tails=E.within(tc, lim), sign=E.within(sg, slim), mean=zm <= zb,
                var=cv <= cb), (d, r, x2, xb, tc, lim)


def test_normal_reference_passes_and_mutants_do_not():
    rng = np.random.default_rng(101)
    ok, fig = _normal_verdicts(E.np_normal(rng, E.N_RADON))
    print("normal reference:", fig)
    assert all(ok.values()), ok
    # the tail sampler replaced by a clamp at R: only the tail counts see it (nothing lies beyond R)
    bad, fig = _normal_verdicts(E.np_normal(rng, E.N_RADON, clamp_tail=True))
    assert not bad["tails"] and fig[4][1] == 0 and fig[4][2] == 0 and fig[4][0] > 0, fig
    # a fifth of one of the 1024 bins moved into its neighbour: 0.02 % of all mass, a step of 2e-4 in the CDF,
    # inside the DKW radius: chi-square sees it, KS does not. (0.2 % of ALL mass does not fit into one bin of
    # 0.098 %; the statistic grows with the share moved, so a larger share is rejected a fortiori -- below,
    # a whole bin.)
    bad, fig = _normal_verdicts(E.np_normal(rng, E.N_RADON, moved_mass=(E.NORMAL_BINS, 600, 0.2)))
    assert not bad["chi2"] and bad["ks"], fig
    bad, fig = _normal_verdicts(E.np_normal(rng, E.N_RADON // 4, moved_mass=(E.NORMAL_BINS, 300, 1.0)))
    assert not bad["chi2"], fig
    # a scale that is 0.2 % off: 8.9 standard errors of the variance at this n
    bad, _ = _normal_verdicts(1.002 * E.np_normal(rng, E.N_RADON))
    assert not bad["var"]


# ---- Student's t at the sizes of the sv groups ------------------------------------------------------------------
def _t_verdicts(x, df):
    d, r = E.ks(x, lambda v: E.t_cdf(v, df), A)
    q = E.t_ppf(1.0 - E.T_TAIL_P, df)
    up, ulim = E.tail_count(x, [q], lambda v: E.t_sf(v, df), A)
    dn, dlim = E.tail_count(-x, [q], lambda v: E.t_sf(v, df), A)
    out = dict(ks=d <= r, upper=E.within(up, ulim), lower=E.within(dn, dlim))
    if df >= 10.0:
        v, vb = E.chi2_var(x, E.t_var(df) if df < 1e80 else 1.0, E.t_excess_kurtosis(df) if df < 1e80 else 0.0, A)
        out["var"] = v <= vb
    return out, (d, r)


T_MUTANTS = dict(rate=dict(chi2_rate=0.55), d=dict(third=0.25), boost=dict(boost_exponent=lambda a: 1.0 / (a + 1.0)),
                 scale=dict(scale=1.02))


@pytest.mark.parametrize("k", range(len(E.T_DF)), ids=["%.3g" % v for v in E.T_DF])
def test_t_reference_passes_and_mutants_do_not(k):
    df, n = E.T_DF[k], E.t_group_n(k)
    rng = np.random.default_rng(200 + k)
    ok, fig = _t_verdicts(E.np_student_t(rng, df, n), df)
    print("t(%g) n=%d reference: D=%.3g radius=%.3g" % (df, n, fig[0], fig[1]))
    assert all(ok.values()), ok
    seen = {}
    for name, kw in T_MUTANTS.items():
        bad, fig = _t_verdicts(E.np_student_t(rng, df, n, **kw), df)
        seen[name] = not all(bad.values())
        print("t(%g) %s: D=%.3g radius=%.3g %s" % (df, name, fig[0], fig[1], bad))
    assert seen["rate"] and seen["scale"], seen               # at every df
    assert seen["d"] or df > 2.0, seen                         # at df <= 2
    assert seen["boost"] == (df < 2.0), seen                   # alpha = df / 2 < 1 boosts; alpha = 1.0 exactly does not


@pytest.mark.parametrize("shape", [0.15, 0.4, 1.0, 3.0, 100.0])
def test_gamma_reference_passes_and_mutants_do_not(shape):
    n = E.t_group_n(1)
    rng = np.random.default_rng(300 + int(shape * 100))
    cdf = lambda v: E.gamma_cdf(v, shape, 0.5)   # noqa: E731
    x = E.np_gamma(rng, shape, 0.5, n)
    d, r = E.ks(x, cdf, A)
    zm, zb = E.z_mean(x, shape / 0.5, math.sqrt(shape) / 0.5, A)
    cv, cb = E.chi2_var(x, shape / 0.25, 6.0 / shape, A)
    assert d <= r and zm <= zb and cv <= cb, (d, r, zm, zb, cv, cb)
    d, r = E.ks(E.np_gamma(rng, shape, 0.5, n, third=0.25), cdf, A)
    assert d > r, (d, r)
    d, r = E.ks(E.np_gamma(rng, shape, 0.5, n, boost_exponent=lambda a: 1.0 / (a + 1.0)), cdf, A)
    assert (d > r) == (shape < 1.0), (d, r)


# ---- Bernoulli at the size of the logistic case ----------------------------------------------------------------
def _bernoulli_verdicts(k, n, p):
    lo, hi = E.binomial_limits(n, p, A / p.size)
    stat, bound = E.pearson_pooled(k, n, p, A)
    return dict(each=E.within(k, (lo, hi)), pooled=stat <= bound), (stat, bound)


def test_bernoulli_reference_passes_and_mutants_do_not():
    rng = np.random.default_rng(401)
    n = E.BERN_N
    p = 1.0 / (1.0 + np.exp(-rng.normal(0.3, 1.2, size=E.BERN_DATUMS)))
    draw = lambda q, **kw: np.array([E.np_bernoulli(rng, qi, n, **kw).sum() for qi in q])   # noqa: E731
    ok, fig = _bernoulli_verdicts(draw(p), n, p)
    assert all(ok.values()), fig
    bad, fig = _bernoulli_verdicts(draw(np.clip(p + 0.005, 0.0, 1.0)), n, p)      # p off by 0.005
    assert not bad["pooled"], fig
    # p = 0 and p = 1: the limits are [0, 0] and [n, n]
    ends = np.array([0.0, 1.0])
    ok, _ = _bernoulli_verdicts(draw(ends), n, ends)
    assert ok["each"]
    u = rng.random(n)
    u[n // 2] = 0.0
    k = np.array([E.np_bernoulli(rng, 0.0, n, inclusive=True, uniforms=u).sum(), float(n)])
    assert k[0] == 1.0 and not _bernoulli_verdicts(k, n, ends)[0]["each"]
    assert E.np_bernoulli(rng, 0.0, n, uniforms=u).sum() == 0.0


# ---- the kinetic energies and the fit draws at the sizes of their GPU files ---------------------------------------
def test_kinetic_energy_reference_passes_and_a_wrong_scale_does_not():
    """tests/test_gpu_momentum_distribution.py's acceptance at its own sizes and level, on half sums of squares of
    numpy normals; momenta 2 % too long (the kinetic energy 4 % up) are rejected at 1030 chains x 100 draws"""
    from test_gpu_momentum_distribution import hold_to_gamma
    rng = np.random.default_rng(501)
    for chains, draws, d in ((1030, 100, 10), (130, 40, 102)):
        hold_to_gamma(0.5 * np.sum(rng.standard_normal((chains, draws, d)) ** 2, axis=2), d, "numpy d=%d" % d)
    with pytest.raises(AssertionError):
        hold_to_gamma(0.5 * np.sum((1.02 * rng.standard_normal((1030, 100, 10))) ** 2, axis=2), 10, "2 % long")


def test_fit_draw_reference_passes_and_a_reused_variate_does_not():
    """tests/test_gpu_fit_draw_distributions.py's acceptance at its own size and level; a variate that two
    dimensions share in one draw of twenty-five (a correlation of 0.04; the pooled bound is 0.017, so one draw
    of a hundred would pass) is rejected by the pooled correlation"""
    from test_gpu_fit_draw_distributions import DRAWS, FITS, hold_to_standard_normal
    rng = np.random.default_rng(502)
    v = rng.standard_normal((FITS, DRAWS, 10))
    hold_to_standard_normal(v, "numpy")
    v[:, ::25, 3] = v[:, ::25, 4]
    with pytest.raises(AssertionError):
        hold_to_standard_normal(v, "reused")
