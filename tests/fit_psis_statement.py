"""The importance diagnostics of a variational fit written from the papers in plain numpy / libm: the
Pareto-smoothed importance ratios p(x) / q(x) of the fit's draws (Vehtari, Simpson, Gelman, Yao, Gabry,
"Pareto smoothed importance sampling"; Yao, Vehtari, Simpson, Gelman 2018 for their use on variational
fits), and systematic resampling from the smoothed weights (the scheme of the reference's smc.ex:180-195;
pooled over the fits it is the importance resampling of multi-path Pathfinder, Zhang et al. 2022).
TEST INFRASTRUCTURE beside the device kernels and tests/host/fit_psis_host_checker.c: it shares no code
with either, knows nothing of chunks, blocks or exmc_detmath.h, and takes the generalised-Pareto fit from
tests/psis_statement.py, the statement of the same fit.

Differences from PSIS-LOO that DESIGN.md "Importance diagnostics of the fits" states: a ratio of -inf is a
sample of weight zero (it counts in n and never enters the tail); a group with a NaN or +inf ratio, or
without a finite one, is NaN throughout and resamples to index -1."""
import ctypes as C
import math

import numpy as np

import oracle as O
import psis_statement as PS
from pathfinder_statement import lane_sum

SIGMA, LOG_SIGMA = 0, 1


def group(lr, total=PS.lsum):
    """One group's ratios in sample order -> dict(khat, log_mean_ratio, ess, n_zero, tail, lw)"""
    lr = np.asarray(lr, dtype=np.float64)
    n = lr.size
    nan = dict(khat=math.nan, log_mean_ratio=math.nan, ess=math.nan, n_zero=math.nan, tail=math.nan,
               lw=np.full(n, np.nan))
    if np.any(np.isnan(lr)) or np.any(lr == np.inf) or not np.any(np.isfinite(lr)):
        return nan
    mx = float(lr.max())
    x = lr - mx
    M = PS.tail_len(n)
    cutoff = max(float(np.sort(x)[n - 1 - M]) if M < n else -math.inf, PS.LOG_DBL_MIN)
    members = np.nonzero(x > cutoff)[0]
    T = members.size
    k = math.inf
    if T > 4:
        order = members[np.argsort(x[members], kind="stable")]   # by (x, k)
        ec = math.exp(cutoff)
        t = [math.exp(float(x[j])) - ec for j in order]
        try:
            k, sigma = PS.gpd_fit(t, total)
        except (ValueError, ZeroDivisionError, OverflowError):
            k = math.nan
        if math.isfinite(k):
            x = x.copy()
            for j, kk in enumerate(order, start=1):
                x[kk] = math.log(PS.gpd_quantile((j - 0.5) / T, k, sigma) + ec)
    x = np.minimum(x, 0.0)
    w = [math.exp(float(a)) for a in x]          # exp(-inf) = 0
    s1, s2 = total(w), total([a * a for a in w])
    l1 = math.log(s1)
    return dict(khat=k, log_mean_ratio=mx + l1 - math.log(n), ess=s1 * s1 / s2, n_zero=float(np.sum(lr == -np.inf)),
                tail=float(T), lw=x - l1)


def first_uniform(seed):
    """The first :rand.uniform_s of the generator seeded with `seed`, from the oracle's generator"""
    L = O.lib()
    r = O.Rng()
    L.exo_rng_seed(C.byref(r), seed)
    return L.exo_rng_uniform(C.byref(r))


def resample(lw, R, u):
    """Systematic resampling: index j is the first k whose cumulative weight reaches (u + j) / R"""
    lw = np.asarray(lw, dtype=np.float64)
    if R < 1:
        return np.zeros(0, dtype=np.int64)
    if np.any(np.isnan(lw)):
        return np.full(R, -1, dtype=np.int64)
    cum = np.cumsum(np.exp(lw))
    pos = (u + np.arange(R)) / R
    return np.minimum(np.searchsorted(cum, pos, side="left"), lw.size - 1)


def groups(lr, pooled, n_resample=0, seed=0, total=PS.lsum):
    """lr [S][n_fits] -> out [5][G], lw [S][n_fits], idx [R][G]: per fit the columns are the groups, pooled
    the one group holds the samples k = s n_fits + c"""
    lr = np.asarray(lr, dtype=np.float64)
    S, F = lr.shape
    cols = [lr.reshape(-1)] if pooled else [lr[:, c] for c in range(F)]
    out = np.empty((5, len(cols)))
    lw = np.empty((S, F))
    idx = np.zeros((n_resample, len(cols)), dtype=np.int64)
    for g, col in enumerate(cols):
        r = group(col, total)
        out[:, g] = [r[k] for k in ("khat", "log_mean_ratio", "ess", "n_zero", "tail")]
        if pooled:
            lw[:] = r["lw"].reshape(S, F)
        else:
            lw[:, g] = r["lw"]
        idx[:, g] = resample(r["lw"], n_resample, first_uniform((seed + 7919 * g) & (2 ** 64 - 1)))
    return out, lw, idx


# ---- the log ratio in the device's arithmetic: the checker's model in the lane layout -------------
def log_ratio_lane(model, lanes, draws, mu, scale, scale_kind):
    """draws [S][d] of one fit (mu, scale [d]) -> (lr [S], logp [S]) as fit_log_ratio_kernel forms them:
    the oracle model in lane mode, exo_det_log / exo_det_exp, the lane layout's sum over the dimensions"""
    L = O.lib()
    cfg = O.Cfg(1, lanes)
    d = model.d
    vsum = lane_sum(lanes, d)
    draws = np.asarray(draws, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    scale = np.asarray(scale, dtype=np.float64)
    c = 0.5 * d * math.log(2.0 * math.pi)
    with np.errstate(all="ignore"):
        if scale_kind == LOG_SIGMA:
            ls = scale.copy()
            sigma = np.array([_det(L.exo_det_exp, float(v)) for v in scale])
        else:
            sigma = scale.copy()
            ls = np.array([_det(L.exo_det_log, float(v)) for v in scale])
        fit_bad = not (np.all(np.isfinite(mu)) and np.all(np.isfinite(scale)))
        lr = np.empty(draws.shape[0])
        logp = np.empty(draws.shape[0])
        for s, x in enumerate(draws):
            lp, _ = model.logp_grad(x, cfg)
            lp = float(lp)
            z = (x - mu) / sigma
            t = 0.5 * (z * z) + ls
            logq = -vsum(t) - c
            logp[s] = lp
            if fit_bad or not np.all(np.isfinite(x)) or math.isnan(lp) or lp == -math.inf:
                lr[s] = -math.inf
            elif lp == math.inf:
                lr[s] = math.nan
            else:
                lr[s] = lp - logq
    return lr, logp


def _det(f, v):
    """exmc_log / exmc_exp at the arguments a hostile fit brings"""
    if math.isnan(v):
        return math.nan
    return f(v)
