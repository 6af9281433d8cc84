"""PSIS-LOO-PIT written from the definition in plain numpy / libm (Vehtari, Gelman, Gabry 2017, "Practical
Bayesian model evaluation using leave-one-out cross-validation and WAIC", section 2; Gabry et al. 2019,
"Visualization in Bayesian workflow", section 5; the smoothing of Vehtari, Simpson, Gelman, Yao, Gabry,
"Pareto smoothed importance sampling", as DESIGN.md "PSIS-LOO" states it with r_eff = 1). TEST
INFRASTRUCTURE: the product never imports it.

Per datum, over the pooled samples k: the importance ratios exp(-ll_k) have their largest T <= M replaced
by the quantiles of the generalised Pareto distribution fitted to them and are truncated at their largest
raw value; with the normalised weights w_k,

    p_lt = sum_k w_k [yrep_k < y]     p_eq = sum_k w_k [yrep_k == y]     pit = p_lt + p_eq / 2

It reuses tests/psis_statement.py's tail_len, gpd_fit and gpd_quantile and normalises the weights directly
(exp of every log weight, one division): it knows nothing of blocks, running maxima or exmc_detmath.h.
Every sum goes through `total`, the left-to-right sum or math.fsum; the difference between the two
evaluations is the estimator's own sensitivity to rounding (tests/test_loo_pit_host.py)."""
import math

import numpy as np

import psis_statement as PSIS
from psis_statement import lsum


def log_weights(ll, total=lsum):
    """(lw [n] unnormalised smoothed log weights, all <= 0; Pareto k; T) of one datum's finite terms"""
    ll = np.asarray(ll, dtype=np.float64)
    n = ll.size
    lr = -ll
    x = lr - lr.max()
    M = PSIS.tail_len(n)
    cutoff = max(float(np.sort(x)[n - 1 - M]), PSIS.LOG_DBL_MIN)
    members = np.nonzero(x > cutoff)[0]                          # ascending k
    T = members.size
    k = math.inf
    if T > 4:
        order = members[np.argsort(x[members], kind="stable")]   # by (x, k)
        ec = math.exp(cutoff)
        t = [math.exp(float(x[j])) - ec for j in order]
        try:
            k, sigma = PSIS.gpd_fit(t, total)
        except (ValueError, ZeroDivisionError, OverflowError):
            k = math.nan
        if math.isfinite(k):
            x = x.copy()
            for j, kk in enumerate(order, start=1):
                x[kk] = math.log(PSIS.gpd_quantile((j - 0.5) / T, k, sigma) + ec)
    return np.minimum(x, 0.0), k, T


def datum(ll, yrep, y, total=lsum):
    """(p_lt, p_eq, pit, k, T) of one datum: terms and replicates in sample order, the observation"""
    ll = np.asarray(ll, dtype=np.float64)
    yrep = np.asarray(yrep, dtype=np.float64)
    if not np.all(np.isfinite(ll)):
        return math.nan, math.nan, math.nan, math.nan, 0
    lw, k, T = log_weights(ll, total)
    w = [math.exp(float(a)) for a in lw]
    W = total(w)
    with np.errstate(invalid="ignore"):
        lt, eq = yrep < y, yrep == y                              # a NaN replicate is in neither set
    p_lt = total([a for a, f in zip(w, lt) if f]) / W
    p_eq = total([a for a, f in zip(w, eq) if f]) / W
    return p_lt, p_eq, p_lt + 0.5 * p_eq, k, T


def run(ll, yrep, y, total=lsum):
    """out [4][N] (p_lt, p_eq, pit, k) and the tail sizes, of ll, yrep [S][N][C] pooled k = s C + c and y [N]"""
    ll = np.asarray(ll, dtype=np.float64)
    yrep = np.asarray(yrep, dtype=np.float64)
    S, N, C = ll.shape
    assert yrep.shape == ll.shape and len(y) == N
    out = np.empty((4, N))
    tails = np.empty(N, dtype=np.int64)
    for i in range(N):
        r = datum(ll[:, i, :].reshape(-1), yrep[:, i, :].reshape(-1), float(y[i]), total)
        out[:, i] = r[:4]
        tails[i] = r[4]
    return out, tails
