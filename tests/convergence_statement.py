"""A plain-numpy statement of the convergence diagnostics across chains (include/exmc_hip_convergence.h,
DESIGN.md "Convergence diagnostics across chains"): what exmc_hip_convergence computes per dimension of a
trace x [S][d][C], written from the contract. TEST INFRASTRUCTURE: the product never imports it.

Every running sum is a real loop over the draws (or the split chains), vectorised over the other index
only; numpy's elementwise + - * / on float64 round once each, so the loops are the contract's arithmetic.
log is the checker's exo_det_log (= exmc_log), sqrt is IEEE. The pooled order is the statement's own
stable sort of the values; ranks are integers (or halves), so they do not depend on how it is made.

  convergence(x) -> [6][d]: rhat_bulk, rhat_tail, ess_bulk, ess_tail, ess_mean, mcse_mean
  CUTS collects, per ESS taken, the smallest |P| among the Geyer pairs it compared with zero (the pair
  at the cut included): how far the sequence was from stopping elsewhere."""
import math

import numpy as np

import oracle as O

ROWS = ("rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean")
LAGS = 16
CUTS = []


def _log(v):
    return float(O.lib().exo_det_log(float(v)))


def _probit_inner(p):
    t = math.sqrt(-2.0 * _log(p))
    return t - (2.515517 + 0.802853 * t + 0.010328 * t * t) / (1.0 + 1.432788 * t + 0.189269 * t * t
                                                                + 0.001308 * t * t * t)


def _probit(p):
    return -_probit_inner(p) if p < 0.5 else _probit_inner(1.0 - p)


def split(xd):
    """one dimension's draws xd [S][C] -> y [n][M], column k = 2 c + half"""
    S, C = xd.shape
    n = S // 2
    y = np.empty((n, 2 * C))
    y[:, 0::2] = xd[:n]
    y[:, 1::2] = xd[n:2 * n]
    return y


def sorted_pool(y):
    v = y.reshape(-1)
    order = np.argsort(v, kind="stable")
    return v[order], order


def scores(y):
    """the normal scores of the average ranks over the pool, in y's shape"""
    sv, order = sorted_pool(y)
    N = sv.size
    heads = np.flatnonzero(np.concatenate(([True], sv[1:] != sv[:-1])))
    ends = np.concatenate((heads[1:], [N]))
    z = np.empty(N)
    for a, b in zip(heads, ends):
        r = float(a + 1) + float(b - a - 1) / 2.0
        z[order[a:b]] = _probit((r - 0.375) / (float(N) + 0.25))
    return z.reshape(y.shape)


def quantile(sv, p):
    """Diagnostics.quantile (diagnostics.ex:170-180)"""
    h = float(sv.size - 1) * p
    lo, hi = math.floor(h), math.ceil(h)
    frac = h - lo
    with np.errstate(invalid="ignore"):
        return sv[lo] + np.float64(frac) * (sv[hi] - sv[lo])


def moments(y):
    """mean_k, var_k [M]"""
    n = y.shape[0]
    s = np.zeros(y.shape[1])
    for i in range(n):
        s = s + y[i]
    mean = s / np.float64(n)
    ss = np.zeros(y.shape[1])
    for i in range(n):
        dv = y[i] - mean
        ss = ss + dv * dv
    return mean, ss / np.float64(n - 1)


def _lsum(v):
    s = np.float64(0.0)
    for a in v:
        s = s + a
    return s


def rhat(y):
    """rhat_kernel phase 1's expressions over the M split chains, len = n, m = M"""
    n, M = y.shape
    means, vars_ = moments(y)
    gm = _lsum(means) / np.float64(M)
    b = _lsum([(mk - gm) * (mk - gm) for mk in means])
    w = _lsum(vars_)
    b = np.float64(n) / np.float64(M - 1) * b
    w = w / np.float64(M)
    var_hat = np.float64(n - 1) / np.float64(n) * w + b / np.float64(n)
    return float(np.sqrt(var_hat / w))


def _acov_block(c, l0):
    """acov_k(l0 .. l0 + 15) [16][M] of the centred series c [n][M], each sum left to right over i"""
    n, M = c.shape
    acc = np.zeros((LAGS, M))
    lag = l0 + np.arange(LAGS)
    pad = np.concatenate((c, np.zeros((l0 + LAGS, M))))
    for i in range(n - l0):
        valid = (i + lag < n)[:, None]
        prod = c[i][None, :] * pad[i + lag]
        acc = np.where(valid, acc + prod, acc)
    return acc / np.float64(n)


def ess(y):
    """(ESS, var_plus) of a derived series y [n][M]"""
    n, M = y.shape
    N = n * M
    nn, Mm = np.float64(n), np.float64(M)
    mean, _ = moments(y)
    c = y - mean[None, :]
    block = _acov_block(c, 0)
    W = _lsum(block[0] * nn / np.float64(n - 1)) / Mm
    gm = _lsum(mean) / Mm
    Bn = _lsum([(mk - gm) * (mk - gm) for mk in mean]) / np.float64(M - 1)
    var_plus = W * np.float64(n - 1) / nn + Bn
    if not var_plus > 0:
        return float("nan"), float(var_plus)
    tau, prev = np.float64(-1.0), np.float64(np.inf)
    l0, A, closest = 0, None, float("inf")
    j = 0
    while 2 * j + 1 <= n - 1:
        if 2 * j >= l0 + LAGS or A is None:
            if A is not None:
                l0 += LAGS
                block = _acov_block(c, l0)
            A = np.array([_lsum(block[t]) / Mm for t in range(LAGS)])
        r0 = np.float64(1.0) if j == 0 else np.float64(1.0) - (W - A[2 * j - l0]) / var_plus
        r1 = np.float64(1.0) - (W - A[2 * j + 1 - l0]) / var_plus
        P = r0 + r1
        closest = min(closest, abs(float(P)))
        if not P > 0:
            break
        P = P if P < prev else prev
        tau = tau + np.float64(2.0) * P
        prev = P
        j += 1
    CUTS.append(closest)
    cap = np.float64(_log(10.0)) / np.float64(_log(float(N)))
    tau = tau if tau > cap else cap
    return float(np.float64(N) / tau), float(var_plus)


def dimension(xd):
    """the six outputs of one dimension's draws xd [S][C]"""
    y = split(np.asarray(xd, dtype=np.float64))
    if np.isnan(y).any():
        return [float("nan")] * 6
    with np.errstate(all="ignore"):
        sv, _ = sorted_pool(y)
        med, q05, q95 = quantile(sv, 0.5), quantile(sv, 0.05), quantile(sv, 0.95)
        z = scores(y)
        zf = scores(np.fabs(y - med))
        i05 = np.where(y <= q05, 1.0, 0.0)
        i95 = np.where(y <= q95, 1.0, 0.0)
        ess_bulk, _ = ess(z)
        e05, _ = ess(i05)
        e95, _ = ess(i95)
        ess_tail = float("nan") if (math.isnan(e05) or math.isnan(e95)) else min(e05, e95)
        ess_mean, vp = ess(y)
        mcse = float(np.sqrt(np.float64(vp) / np.float64(ess_mean)))
        return [rhat(z), rhat(zf), ess_bulk, ess_tail, ess_mean, mcse]


def convergence(x):
    """x [S][d][C] -> [6][d]"""
    x = np.asarray(x, dtype=np.float64)
    return np.array([dimension(x[:, j, :]) for j in range(x.shape[1])]).T
