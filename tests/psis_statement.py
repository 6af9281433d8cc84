"""PSIS-LOO written from the published algorithm in plain numpy / libm (Vehtari, Simpson, Gelman, Yao,
Gabry, "Pareto smoothed importance sampling"; Zhang & Stephens 2009 for the generalised-Pareto fit), as
DESIGN.md "PSIS-LOO" states it with r_eff = 1. A third statement beside the device kernels and
tests/host/psis_host_checker.c: it shares no code with either, knows nothing of chunks, lanes or
exmc_detmath.h, and sorts the tail with numpy's stable sort on x (ties keep the sample order k).

Every sum goes through `total`, which is either the left-to-right Python sum or math.fsum: the
difference between the two evaluations is the estimator's own sensitivity to rounding, from which
tests/test_psis_host.py derives its bound."""
import math
import sys

import numpy as np

LOG_DBL_MIN = math.log(sys.float_info.min)


def lsum(v):
    acc = 0.0
    for x in v:
        acc += x
    return acc


def exp(x):
    """math.exp, overflowing to +inf as C's does"""
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def tail_len(n):
    return int(math.ceil(min(n / 5, 3 * math.sqrt(n))))


def gpd_fit(t, total=lsum):
    """(k, sigma) of the ascending sample t: the posterior-mean estimator with PSIS' weak prior on k"""
    T = len(t)
    m = 30 + int(math.floor(math.sqrt(T)))
    t_last, t_q = t[T - 1], t[int(math.floor(T / 4 + 0.5)) - 1]
    with np.errstate(all="ignore"):
        b = [1 / t_last + (1 - math.sqrt(m / (j - 0.5))) / (3 * t_q) for j in range(1, m + 1)]

        def kappa(bv):
            return total([math.log1p(-bv * v) for v in t]) / T

        kap = [kappa(bv) for bv in b]
        L = [T * (math.log(-bv / kv) - kv - 1) for bv, kv in zip(b, kap)]
        w = [1 / total([exp(Li - Lj) for Li in L]) for Lj in L]
        w = [0.0 if wj < 10 * sys.float_info.epsilon else wj for wj in w]
        W = total(w)
        w = [wj / W for wj in w]
        bh = total([wj * bv for wj, bv in zip(w, b)])
        kh = kappa(bh)
    return (T * kh + 10 * 0.5) / (T + 10), -kh / bh


def gpd_quantile(p, k, sigma):
    if k == 0:
        return -sigma * math.log1p(-p)
    return sigma * math.expm1(-k * math.log1p(-p)) / k


def lse(v, total=lsum):
    m = max(v)
    return m + math.log(total([math.exp(x - m) for x in v]))


def datum(ll, total=lsum):
    """(elpd_loo, p_loo, k, T) of one datum's terms in sample order"""
    ll = np.asarray(ll, dtype=np.float64)
    n = ll.size
    if not np.all(np.isfinite(ll)):
        return math.nan, math.nan, math.nan, 0
    lr = -ll
    x = lr - lr.max()
    M = tail_len(n)
    cutoff = max(float(np.sort(x)[n - 1 - M]), LOG_DBL_MIN)
    members = np.nonzero(x > cutoff)[0]                       # ascending k
    T = members.size
    k = math.inf
    if T > 4:
        order = members[np.argsort(x[members], kind="stable")]   # by (x, k)
        ec = math.exp(cutoff)
        t = [math.exp(float(x[j])) - ec for j in order]
        try:
            k, sigma = gpd_fit(t, total)
        except (ValueError, ZeroDivisionError, OverflowError):
            k = math.nan
        if math.isfinite(k):
            x = x.copy()
            for j, kk in enumerate(order, start=1):
                x[kk] = math.log(gpd_quantile((j - 0.5) / T, k, sigma) + ec)
    x = np.minimum(x, 0.0)
    lw = [float(a) for a in x]
    v = [float(a) for a in ll]
    elpd = lse([a + b for a, b in zip(lw, v)], total) - lse(lw, total)
    lppd = lse(v, total) - math.log(n)
    return elpd, lppd - elpd, k, T


def stats(ll, total=lsum):
    """[3][N] (elpd_loo, p_loo, k) and the tail sizes of ll [S][N][C], samples pooled k = s C + c"""
    ll = np.asarray(ll, dtype=np.float64)
    S, N, C = ll.shape
    out = np.empty((3, N))
    tails = np.empty(N, dtype=np.int64)
    for i in range(N):
        e, p, k, T = datum(ll[:, i, :].reshape(-1), total)
        out[:, i] = (e, p, k)
        tails[i] = T
    return out, tails
