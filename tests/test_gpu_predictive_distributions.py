"""Every family of posterior predictive replicates the device draws (exmc_amd/csrc/exmc_predictive.hpp), held
to the exact law it names. The trace of a call is constant within a chain, so the replicates of a chain are
i.i.d. from a law known in closed form; they are standardised with parameters computed here in plain numpy
from the model's data blob (the kinds restated as tests/test_ic_host.py restates them), and the pooled sample
goes through the acceptance functions of tests/exact_distributions.py. Nothing here compares the device with
the statement (tests/test_gpu_predictive.py does, bit for bit); every bound follows from n and the level.

Level: the file spends 1e-6 over at most E.PRED_ASSERTIONS = 80 statistical assertions, E.PRED_ALPHA = 1.25e-8
each (radon 5, eight_schools 2, simple 2, sv and sv_ncp 22 each, logistic 3, independence 5: 61). Where one
assertion covers several cells (datums, thresholds, chain pairs) its level is split again over the cells.
tests/test_exact_distributions.py shows on the CPU that at these sizes and this level a correct sampler passes
and the wrong ones listed there do not. Seeds are fixed. No replicate is excluded; every case asserts that
none is NaN. Every case runs at least two wavefronts of chains, the last one partial."""
import math

import numpy as np
import pytest

import exact_distributions as E
from exmc_amd import models, sampler
from test_gpu_predictive import device_call

pytestmark = pytest.mark.gpu

A = E.PRED_ALPHA
TINY32 = float(np.float32(1.0e-30))
_cache = {}


def _exp200(v):
    return np.exp(np.clip(v, -200.0, 200.0))


def _trace(q, S):
    """q [C][d], one point per chain -> the device trace [S][d][C], constant within a chain"""
    return np.ascontiguousarray(np.broadcast_to(q.T[None], (S,) + q.T.shape))


def _replicates(spec, q, S, seed, chain_lo=0):
    cm = sampler.compile(spec)
    try:
        y, _ = device_call(cm, _trace(q, S), seed, chain_lo, want_state=False)
    finally:
        cm.close()
    assert y.shape[0] == S and y.shape[2] == q.shape[0]
    assert np.count_nonzero(np.isnan(y)) == 0          # the share of NaN replicates is 0
    return y


# ---- the kinds' parameters, in plain numpy from the blob ---------------------------------------------------------
def radon_params(blob, q):
    """q [C][90] -> loc [N][C], scale [C]"""
    J = 85
    N = (blob.size - 171) // 2
    u, cs, fl = blob[:J], blob[J:2 * J + 1].astype(int), blob[2 * J + 1:2 * J + 1 + N]
    county = np.repeat(np.arange(J), np.diff(cs))
    alpha = q[:, J, None] + q[:, J + 1, None] * u[None] + _exp200(q[:, J + 2, None]) * q[:, :J]     # [C][J]
    loc = alpha[:, county] + q[:, J + 4, None] * fl[None]
    return loc.T, np.maximum(_exp200(q[:, J + 3]), TINY32)


def eight_schools_params(blob, q):
    return (q[:, 0, None] + _exp200(q[:, 1, None]) * q[:, 2:10]).T, blob[8:16]       # loc [8][C], scale [8]


def simple_params(blob, q):
    return q[:, 0], np.maximum(_exp200(q[:, 1]), TINY32)                             # loc [C], scale [C]


def sv_params(kind, q):
    """q [C][102] -> s [100][C] (the scale of return t is exp(s_t)), df [C]"""
    if kind == models.SV_NCP:
        s = np.cumsum(np.concatenate([q[:, :1], _exp200(q[:, 100, None]) * q[:, 1:100]], axis=1), axis=1)
    else:
        s = q[:, :100]
    return s.T, np.maximum(_exp200(q[:, 101]), TINY32)


def logistic_p(blob, q):
    """q [21] -> p [N] in long double"""
    N = blob.size // 21
    X = blob[:N * 20].reshape(N, 20).astype(np.longdouble)
    eta = np.longdouble(q[0]) + X @ q[1:].astype(np.longdouble)
    return np.asarray(1.0 / (1.0 + np.exp(-eta)), dtype=np.float64)


# ---- normal, through radon: 919 datums x 280 chains x 40 draws ---------------------------------------------------
RADON_C, RADON_S = 280, 40


def _radon_z():
    if "radon" not in _cache:
        spec = models.radon()
        q0 = np.asarray(spec.to_unconstrained(spec.default_init))
        q = q0[None] + 0.5 * np.random.default_rng(501).normal(size=(RADON_C, spec.d))
        y = _replicates(spec, q, RADON_S, seed=77)
        loc, scale = radon_params(spec.data, q)
        assert y.shape == (RADON_S, 919, RADON_C) and y.size == E.N_RADON
        _cache["radon"] = (y - loc[None]) / scale[None, None]
    return _cache["radon"]


def test_radon_replicates_are_standard_normal(hip):
    z = _radon_z()
    d, r = E.ks(z, E.normal_cdf, A)
    x2, xb = E.chi2_equiprobable(z, E.normal_ppf, E.NORMAL_BINS, A)
    tc, lim = E.tail_count(np.abs(z), E.NORMAL_TAILS, E.abs_normal_sf, A)
    sg, slim = E.sign_count(z, A)
    # each datum's loc: the mean of its 11200 standardised replicates is N(0, 1 / 11200) exactly
    per = z.shape[0] * z.shape[2]
    zm = np.abs(z.mean(axis=(0, 2))) * math.sqrt(per)
    zb = E.normal_bound(A / z.shape[1])
    print("radon n=%d: KS %.3g <= %.3g; chi2(1023) %.1f <= %.1f; |z| > 3, R, 4.5: %s in %s..%s; positive %d in %s; "
          "max datum mean %.2f <= %.2f sigma" % (z.size, d, r, x2, xb, tc, lim[0], lim[1], sg, slim, zm.max(), zb))
    assert d <= r
    assert x2 <= xb
    assert E.within(tc, lim)
    assert E.within(sg, slim)
    assert zm.max() <= zb, int(np.argmax(zm))


def test_chains_draw_independently(hip):
    """chain c draws with seed + 7919 c: the standardised radon replicates of two chains, as series over (draw,
    datum), must not correlate, at lag 0 for the neighbours at distance 1, 32 and 64 (a wavefront apart) and
    at lags 1 and 2 for distance 1; and no two chains may start with the same variates."""
    z = _radon_z()
    C = z.shape[2]
    series = np.ascontiguousarray(z.reshape(-1, C).T)                  # [C][S * N]
    n = series.shape[1]
    cases = [(1, 0), (32, 0), (64, 0), (1, 1), (1, 2)]
    for dist, lag in cases:
        a, b = series[:C - dist, lag:], series[dist:, :n - lag]
        r = np.abs(E.correlation(a, b))
        bound = E.correlation_bound(n - lag, A / r.size)
        print("chains c, c+%d at lag %d: max |r| %.3g <= %.3g over %d pairs" % (dist, lag, r.max(), bound, r.size))
        assert r.max() <= bound, (dist, lag, int(np.argmax(r)))
    first = series[:, :8]
    gap = np.abs(first[:, None, :] - first[None, :, :]).max(axis=2) + np.eye(C)
    assert gap.min() > 1e-9, np.unravel_index(np.argmin(gap), gap.shape)


# ---- normal, through eight_schools and simple, at hostile parameter values ----------------------------------------
def test_eight_schools_replicates_at_the_clamp_and_at_extreme_scales(hip):
    """130 chains x 1000 draws x 8 schools. The schools' scales are data: two at 1e-150, two at 1e150 (their
    loc is exactly 0: mu = 0 and theta = 0, so that loc + scale z keeps z). A third of the chains each at
    log tau = 250 and -250, past the clamp at +-200 (tau = e^+-200, theta of the order 1 / tau), and at 0.3."""
    sigma = np.array([1e-150, 1e150, 16.0, 11.0, 9.0, 11.0, 1e-150, 1e150])
    spec = models.eight_schools(y=models.EIGHT_SCHOOLS_Y, sigma=list(sigma))
    C, S = 130, 1000
    rng = np.random.default_rng(502)
    q = np.zeros((C, 10))
    mid = np.arange(2, 6)
    q[:44, 1], q[44:88, 1], q[88:, 1] = 250.0, -250.0, 0.3
    q[:44, 2 + mid] = np.arange(1, 5) * 1e-87
    q[44:88, 2 + mid] = -np.arange(1, 5) * 1e87
    q[88:, 2 + mid] = rng.normal(size=(C - 88, 4))
    y = _replicates(spec, q, S, seed=78)
    loc, scale = eight_schools_params(spec.data, q)
    assert np.all(loc[[0, 1, 6, 7]] == 0.0) and 0.5 < abs(loc[2, 0]) < 2.0 and 0.5 < abs(loc[2, 50]) < 2.0
    z = (y - loc[None]) / scale[None, :, None]
    d, r = E.ks(z, E.normal_cdf, A)
    de, re_ = E.ks(z[:, [0, 1, 6, 7], :], E.normal_cdf, A)
    print("eight_schools n=%d: KS %.3g <= %.3g; extreme scales n=%d: KS %.3g <= %.3g" % (z.size, d, r, z.size // 2, de, re_))
    assert d <= r
    assert de <= re_


def test_simple_replicates_at_the_floor_and_the_clamp(hip):
    """130 chains x 800 draws x 10 datums: a third of the chains each with log sigma = -250 (the scale is the
    float32 floor 1e-30, loc 0), 250 (e^200 after the clamp, loc 2) and log 1.3 (loc 2)."""
    spec = models.simple()
    C, S = 130, 800
    q = np.zeros((C, 2))
    q[:44] = (0.0, -250.0)
    q[44:88] = (2.0, 250.0)
    q[88:] = (2.0, math.log(1.3))
    y = _replicates(spec, q, S, seed=79)
    loc, scale = simple_params(spec.data, q)
    assert scale[0] == TINY32 and scale[50] == math.exp(200.0)
    z = (y - loc[None, None]) / scale[None, None]
    d, r = E.ks(z, E.normal_cdf, A)
    df_, rf = E.ks(z[:, :, :44], E.normal_cdf, A)
    print("simple n=%d: KS %.3g <= %.3g; at the floor n=%d: KS %.3g <= %.3g" % (z.size, d, r, z[:, :, :44].size, df_, rf))
    assert d <= r
    assert df_ <= rf


# ---- Student-t, through sv and sv_ncp ----------------------------------------------------------------------------
def _log_nu_of_two(oracle_lib):
    """a log nu at which the device's exp gives nu = 2.0 exactly (alpha = 1.0 must not boost), searched among
    the neighbours of log 2 with the checker's deterministic exp; log 2 itself if there is none"""
    v = math.log(2.0)
    cands = [v]
    for _ in range(4):
        cands = [math.nextafter(cands[0], -1.0)] + cands + [math.nextafter(cands[-1], 1.0)]
    for c in sorted(cands, key=lambda c: abs(c - v)):
        if oracle_lib.exo_det_exp(c) == 2.0:
            return c
    return v


@pytest.mark.parametrize("kind", [models.SV, models.SV_NCP], ids=["sv", "sv_ncp"])
def test_sv_replicates_are_student_t(kind, hip, oracle_lib):
    """Groups of chains at nu = 0.3 (264 chains), 1, 2, 10, 200 and e^200 (log nu = 200, the clamp; 66 chains
    each), 250 draws x 100 returns. The log volatilities s_t differ per return and span -8 .. 3 in unequal
    steps; for sv_ncp q holds s_1 and the innovations that walk there."""
    spec = (models.sv if kind == models.SV else models.sv_ncp)(models.sv_returns())
    C, S = sum(E.T_CHAINS), E.T_DRAWS
    assert C % 64 != 0 and C > 128
    rng = np.random.default_rng(503)
    steps = rng.gamma(2.0, size=99)
    s_want = -8.0 + 11.0 * np.concatenate([[0.0], np.cumsum(steps) / steps.sum()])
    log_sigma = math.log(0.15)
    q = np.zeros((C, 102))
    q[:, 100] = log_sigma
    if kind == models.SV:
        q[:, :100] = s_want
    else:
        q[:, 0] = s_want[0]
        q[:, 1:100] = np.diff(s_want) / math.exp(log_sigma)
    log_nu = [math.log(0.3), 0.0, _log_nu_of_two(oracle_lib), math.log(10.0), math.log(200.0), 200.0]
    lo = np.concatenate([[0], np.cumsum(E.T_CHAINS)])
    for k in range(len(E.T_DF)):
        q[lo[k]:lo[k + 1], 101] = log_nu[k]
    s, df = sv_params(kind, q)
    # the walk against np.cumsum, to within rounding
    assert np.max(np.abs(s - s_want[:, None])) <= 256 * np.finfo(float).eps * 8.0
    assert s.min() == -8.0 and abs(s.max() - 3.0) < 1e-12
    y = _replicates(spec, q, S, seed=80 + kind)
    z = y * np.exp(-s)[None]
    for k, nu in enumerate(E.T_DF):
        assert np.allclose(df[lo[k]:lo[k + 1]], nu, rtol=1e-14, atol=0.0)
        x = z[:, :, lo[k]:lo[k + 1]]
        assert x.size == E.t_group_n(k)
        sf = lambda v: E.t_sf(v, nu)   # noqa: E731
        d, r = E.ks(x, lambda v: E.t_cdf(v, nu), A)
        qt = E.t_ppf(1.0 - E.T_TAIL_P, nu)
        up, ulim = E.tail_count(x, [qt], sf, A)
        dn, dlim = E.tail_count(-x, [qt], sf, A)
        print("%s nu=%.3g n=%d: KS %.3g <= %.3g; above the 1 - 1e-4 quantile %d, below the 1e-4 quantile %d, in %d..%d"
              % (spec.name, nu, x.size, d, r, up[0], dn[0], ulim[0][0], ulim[1][0]))
        assert d <= r, nu
        assert E.within(up, ulim), nu
        assert E.within(dn, dlim), nu
        if nu >= 10.0:
            big = nu > 1e80
            v, vb = E.chi2_var(x, 1.0 if big else E.t_var(nu), 0.0 if big else E.t_excess_kurtosis(nu), A)
            print("    variance: %.2f <= %.2f standard errors" % (v, vb))
            assert v <= vb, nu
        if nu > 1e80:     # at the clamp the t is the normal
            dn_, rn = E.ks(x, E.normal_cdf, A)
            print("    against the normal law: KS %.3g <= %.3g" % (dn_, rn))
            assert dn_ <= rn


# ---- Bernoulli, through logistic ----------------------------------------------------------------------------------
def test_logistic_replicates_are_bernoulli(hip):
    """500 datums, 160 draws. Chains 0..129 share one coefficient vector (20800 replicates per datum, eta_i
    from about -4 to 4); chains 130..145 have eta = 40 for every datum (p rounds to 1), 146..161 eta = -40
    (p = 4e-18, below the uniform's grid of 2^-53); chains 162..193 have a NaN intercept: a NaN p draws 0.0."""
    spec = models.logistic()
    N, C, S = E.BERN_DATUMS, 194, 160
    rng = np.random.default_rng(504)
    main = np.concatenate([[0.3], 0.3 * rng.normal(size=20)])
    q = np.zeros((C, 21))
    q[:130] = main
    q[130:146, 0], q[146:162, 0], q[162:, 0] = 40.0, -40.0, np.nan
    y = _replicates(spec, q, S, seed=81)
    assert y.shape == (S, N, C) and np.all((y == 0.0) | (y == 1.0))
    p = logistic_p(spec.data, main)
    assert 0.005 < p.min() < 0.1 and 0.9 < p.max() < 0.995
    n = E.BERN_N
    k = y[:, :, :130].sum(axis=(0, 2))
    lo, hi = E.binomial_limits(n, p, A / N)
    zdev = np.abs(k - n * p) / np.sqrt(n * p * (1.0 - p))
    zb = E.normal_bound(A / N)
    stat, bound = E.pearson_pooled(k, n, p, A)
    print("logistic n=%d per datum: max deviation %.2f <= %.2f sigma; pooled Pearson(%d) %.1f <= %.1f"
          % (n, zdev.max(), zb, N, stat, bound))
    assert zdev.max() <= zb, int(np.argmax(zdev))
    assert E.within(k, (lo, hi))
    assert stat <= bound
    # eta = +-40 and the NaN intercept: the exact limits leave one value each
    m = 16 * S
    p_hi, p_lo = logistic_p(spec.data, q[130]), logistic_p(spec.data, q[146])
    assert np.all(p_hi == 1.0) and np.all((p_lo > 0.0) & (p_lo < 1e-17))
    assert E.within(y[:, :, 130:146].sum(axis=(0, 2)), E.binomial_limits(m, p_hi, A / N)) and np.all(y[:, :, 130:146] == 1.0)
    assert E.within(y[:, :, 146:162].sum(axis=(0, 2)), E.binomial_limits(m, p_lo, A / N)) and np.all(y[:, :, 146:162] == 0.0)
    assert np.all(y[:, :, 162:] == 0.0)
