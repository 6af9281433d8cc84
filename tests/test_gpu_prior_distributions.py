"""Every prior family the device draws (exmc_amd/csrc/exmc_prior.hpp) in every built-in kind, and the prior
predictive replicates, held to the exact law they name. The draws of a call are i.i.d. across chains and
draws, so a variable standardised with its prior's literals is a sample of a law known in closed form; a
datum's replicate is standardised with parameters computed here in plain numpy from the position q of its
draw and the model's data blob (the kinds restated as tests/test_gpu_predictive_distributions.py restates
them), and the pooled sample goes through the acceptance functions of tests/exact_distributions.py. Nothing
here compares the device with the statement (tests/test_gpu_prior.py does, bit for bit); every bound follows
from n and the level.

Level: the file spends E.FAMILY = 1e-6 over PRIOR_ASSERTIONS = 48 statistical assertions (simple 6,
eight_schools 8, radon 14, logistic 3, sv and sv_ncp 8 each: 47), 2.08e-8 each. Every law takes two: the
Kolmogorov-Smirnov distance within the DKW radius, and the counts beyond the 1e-4 and 1 - 1e-4 quantiles
inside exact binomial limits (the level split over the two) -- for HalfCauchy the upper count is the test
of the tangent's tail, scale * tan((pi/2) u) near u = 1. Seeds are fixed. No draw is excluded; every case
asserts that nothing is NaN and that no two chains start with the same eight variates. Every case runs at
least two wavefronts of chains, the last one partial."""
import math

import numpy as np
import pytest

import exact_distributions as E
import test_gpu_predictive_distributions as PD
from exmc_amd import models, sampler
from test_gpu_prior import device_call

pytestmark = pytest.mark.gpu

PRIOR_ASSERTIONS = 48
A = E.level(PRIOR_ASSERTIONS)
TAIL_P = 1.0e-4
F32_TENTH = float(np.float32(0.1))

NORMAL = (E.normal_cdf, E.normal_ppf)
HALF_CAUCHY = (lambda t: (2.0 / math.pi) * np.arctan(np.asarray(t, dtype=np.float64)),
               lambda p: np.tan(0.5 * math.pi * np.asarray(p, dtype=np.float64)))
EXPONENTIAL = (lambda t: -np.expm1(-np.asarray(t, dtype=np.float64)), lambda p: -np.log1p(-np.asarray(p, dtype=np.float64)))
UNIFORM = (lambda t: np.clip(t, 0.0, 1.0), lambda p: np.asarray(p, dtype=np.float64))


def _draws(spec, S, Cn, seed):
    cm = sampler.compile(spec)
    try:
        x, q, y, _ = device_call(cm, S, Cn, seed, 0, want_state=False)
    finally:
        cm.close()
    assert x.shape == q.shape == (S, spec.d, Cn) and y.shape[0] == S and y.shape[2] == Cn
    assert not np.isnan(x).any() and not np.isnan(q).any() and not np.isnan(y).any()
    # no two chains start with the same eight variates
    first = np.ascontiguousarray(x[0, :8 if spec.d >= 8 else spec.d, :].T)
    if spec.d < 8:
        first = np.concatenate([first, np.ascontiguousarray(y[0, :8 - spec.d, :].T)], axis=1)
    gap = np.abs(first[:, None, :] - first[None, :, :]).max(axis=2) + np.eye(Cn)
    assert gap.min() > 1e-12, np.unravel_index(np.argmin(gap), gap.shape)
    return x, q, y


def _rows(a):
    """[S][k][C] -> [k][S C], column s C + c"""
    return np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(a.shape[1], -1)


def hold(label, v, law, tails_of=None):
    """two assertions: KS within the DKW radius; the counts below the 1e-4 and above the 1 - 1e-4 quantile
    inside the exact limits of Binomial(n, 1e-4). tails_of: the part of v whose tails are counted (all of it
    by default)"""
    cdf, ppf = law
    v = np.asarray(v, dtype=np.float64).ravel()
    d, r = E.ks(v, cdf, A)
    t = v if tails_of is None else np.asarray(tails_of, dtype=np.float64).ravel()
    lo_q, hi_q = float(ppf(TAIL_P)), float(ppf(1.0 - TAIL_P))
    counts = np.array([int(np.count_nonzero(t < lo_q)), int(np.count_nonzero(t > hi_q))])
    lim = E.binomial_limits(t.size, np.array([TAIL_P, TAIL_P]), A / 2.0)
    print("%s n=%d: KS %.3g <= %.3g; of %d below the 1e-4 quantile %d, above the 1 - 1e-4 quantile %d, in %d..%d"
          % (label, v.size, d, r, t.size, counts[0], counts[1], lim[0][0], lim[1][0]))
    assert d <= r, label
    assert E.within(counts, lim), label


def test_simple(hip):
    spec = models.simple()
    S, Cn = 800, 130
    x, q, y = _draws(spec, S, Cn, seed=91)
    hold("simple mu / 5", x[:, 0, :] / 5.0, NORMAL)
    hold("simple sigma", x[:, 1, :], EXPONENTIAL)
    qr = _rows(q).T
    loc, scale = PD.simple_params(spec.data, qr)
    hold("simple replicates", (_rows(y) - loc[None]) / scale[None], NORMAL)


def test_eight_schools(hip):
    spec = models.eight_schools()
    S, Cn = 1000, 130
    x, q, y = _draws(spec, S, Cn, seed=92)
    hold("eight_schools mu / 5", x[:, 0, :] / 5.0, NORMAL)
    hold("eight_schools tau / 5", x[:, 1, :] / 5.0, HALF_CAUCHY)
    hold("eight_schools theta_trans", x[:, 2:, :], NORMAL)
    loc, scale = PD.eight_schools_params(spec.data, _rows(q).T)
    hold("eight_schools replicates", (_rows(y) - loc) / scale[:, None], NORMAL)


def test_radon(hip):
    spec = models.radon()
    S, Cn = PD.RADON_S, PD.RADON_C
    x, q, y = _draws(spec, S, Cn, seed=93)
    J = 85
    hold("radon alpha_raw", x[:, :J, :], NORMAL)
    hold("radon mu_alpha / 10", x[:, J, :] / 10.0, NORMAL)
    hold("radon gamma_u / 5", x[:, J + 1, :] / 5.0, NORMAL)
    hold("radon sigma_alpha / 2.5", x[:, J + 2, :] / 2.5, HALF_CAUCHY)
    hold("radon sigma_y / 2.5", x[:, J + 3, :] / 2.5, HALF_CAUCHY)
    hold("radon beta / 5", x[:, J + 4, :] / 5.0, NORMAL)
    loc, scale = PD.radon_params(spec.data, _rows(q).T)
    hold("radon replicates", (_rows(y) - loc) / scale[None], NORMAL)


def test_logistic(hip):
    spec = models.logistic()
    S, Cn = 160, 194
    x, q, y = _draws(spec, S, Cn, seed=94)
    hold("logistic alpha, beta / 10", x / 10.0, NORMAL)
    assert np.all((y == 0.0) | (y == 1.0))
    # the replicates: y_i ~ Bernoulli(p_i(q)) with p of the draw; the sum of y - p over all of them, standardised
    # with the exact variance sum p (1 - p), against the normal quantile (1.5e7 independent terms)
    N = spec.n_obs
    X = spec.data[:N * 20].reshape(N, 20)
    qr = _rows(q)                                              # [21][S C]
    p = 1.0 / (1.0 + np.exp(-(qr[0][None] + X @ qr[1:])))      # [N][S C]
    yr = _rows(y)
    z = abs(float(np.sum(yr - p))) / math.sqrt(float(np.sum(p * (1.0 - p))))
    print("logistic replicates n=%d: |sum(y - p)| = %.2f <= %.2f standard deviations; share of ones %.4f, mean p %.4f"
          % (yr.size, z, E.normal_bound(A), yr.mean(), p.mean()))
    assert z <= E.normal_bound(A)


@pytest.mark.parametrize("kind", [models.SV, models.SV_NCP], ids=["sv", "sv_ncp"])
def test_sv(kind, hip):
    from scipy import stats
    spec = (models.sv if kind == models.SV else models.sv_ncp)(models.sv_returns())
    S, Cn = 250, 194
    x, q, y = _draws(spec, S, Cn, seed=95 + kind)
    hold("%s nu * f32(0.1)" % spec.name, x[:, 101, :] * F32_TENTH, EXPONENTIAL)
    hold("%s sigma * 50" % spec.name, x[:, 100, :] * 50.0, EXPONENTIAL)
    # the increments s_1, s_t - s_{t-1}, standardised by the sampled sigma
    s = x[:, :100, :]
    inc = np.concatenate([s[:, :1, :], np.diff(s, axis=1)], axis=1) / x[:, 100:101, :]
    hold("%s increments / sigma" % spec.name, inc, NORMAL)
    # the replicates: r_t exp(-s_t) is Student-t with the draw's nu; through its CDF a uniform. The tails are
    # counted over the draws with nu >= 1 (nu is drawn before the replicates, so given nu they are still
    # i.i.d. uniform). Below that the law has no tail to count in a double: nu ~ Exponential(0.1) reaches
    # 0.01 and less, where the t's 1 - 1e-4 quantile, 1e4^(1 / nu) and more, lies past the largest double,
    # and where chi2 = gamma(nu / 2 + 1) u^(2 / nu) underflows to 0 with probability exp(-354 nu), so the
    # replicate is +-inf with CDF 1 or 0: 0.1 / 354 = 2.8e-4 of all replicates, three times what the two
    # tails hold (measured on the first run: 1224 and 1238 against 364..616 of 4 850 000).
    sw, df = PD.sv_params(kind, _rows(q).T)                    # [100][S C], [S C]
    u = stats.t.cdf(_rows(y) * np.exp(-sw), df[None])
    keep = df >= 1.0
    assert 0.85 < keep.mean() < 0.95                           # exp(-0.1) = 0.905
    hold("%s replicates, t CDF" % spec.name, u, UNIFORM, tails_of=u[:, keep])
