"""The statement of the convergence diagnostics across chains (tests/convergence_statement.py, the contract
of include/exmc_hip_convergence.h) against a second formulation that shares no code with it, its behaviour
on the cases the diagnostics exist for, and its properties. CPU only; the device is held to the statement
byte for byte in tests/test_gpu_convergence.py."""
import math
import os
import re

import numpy as np
import pytest

import convergence_statement as CS
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ar1(rng, S, C, phi, d=1):
    e = rng.normal(size=(S, d, C))
    x = np.zeros((S, d, C))
    x[0] = e[0] / math.sqrt(1.0 - phi * phi)
    for i in range(1, S):
        x[i] = phi * x[i - 1] + e[i]
    return x


def exo_rhat(x, dim=0):
    chains = np.ascontiguousarray(x[:, dim, :].T)
    return O.lib().exo_rhat(O.dptr(chains), chains.shape[0], chains.shape[1])


# ---- 1. a second formulation: scipy's ranks, vectorised moments, FFT autocovariances ----------------

def _alt_scores(v):
    from scipy.stats import rankdata
    N = v.size
    p = (rankdata(v.reshape(-1), method="average") - 0.375) / (N + 0.25)
    q = np.where(p < 0.5, p, 1.0 - p)
    t = np.sqrt(-2.0 * np.log(q))
    num = np.polyval([0.010328, 0.802853, 2.515517], t)
    den = np.polyval([0.001308, 0.189269, 1.432788, 1.0], t)
    return (np.where(p < 0.5, -1.0, 1.0) * (t - num / den)).reshape(v.shape)


def _alt_rhat(y):   # y [M][n]
    n = y.shape[1]
    w = y.var(axis=1, ddof=1).mean()
    b = n * y.mean(axis=1).var(ddof=1)
    return math.sqrt(((n - 1) / n * w + b / n) / w)


def _alt_ess(y):    # y [M][n]
    M, n = y.shape
    c = y - y.mean(axis=1, keepdims=True)
    f = np.fft.rfft(c, 2 * n, axis=1)
    A = (np.fft.irfft(f * np.conj(f), 2 * n, axis=1)[:, :n] / n).mean(axis=0)
    W = A[0] * n / (n - 1)
    var_plus = W * (n - 1) / n + y.mean(axis=1).var(ddof=1)
    rho = 1.0 - (W - A) / var_plus
    rho[0] = 1.0
    pairs = rho[0:2 * (n // 2):2] + rho[1:2 * (n // 2):2]
    stop = np.flatnonzero(~(pairs > 0))
    pairs = np.minimum.accumulate(pairs[:stop[0] if stop.size else pairs.size])
    tau = max(-1.0 + 2.0 * pairs.sum(), math.log(10.0) / math.log(M * n))
    return M * n / tau, var_plus


def alt_dimension(xd):   # xd [S][C]
    S, C = xd.shape
    n = S // 2
    y = np.concatenate((xd[:n].T, xd[n:2 * n].T))   # [M][n], the halves stacked: another chain order
    pool = np.sort(y.reshape(-1))
    med, q05, q95 = (np.quantile(pool, p) for p in (0.5, 0.05, 0.95))
    z, zf = _alt_scores(y), _alt_scores(np.abs(y - med))
    ess_mean, vp = _alt_ess(y)
    return [_alt_rhat(z), _alt_rhat(zf), _alt_ess(z)[0],
            min(_alt_ess((y <= q05) * 1.0)[0], _alt_ess((y <= q95) * 1.0)[0]), ess_mean, math.sqrt(vp / ess_mean)]


@pytest.mark.parametrize("S,C,phi,seed", [(200, 8, 0.0, 1), (600, 4, 0.6, 2), (81, 30, 0.3, 3), (1000, 2, 0.9, 4)])
def test_statement_agrees_with_a_second_formulation(S, C, phi, seed):
    """1e-9 relative: the reordering bound N u is about 1e-11 at these sizes, the margin is for the chained
    divisions. No Geyer pair the statement compared with zero lies within 1e-6 of it, so a flipped
    comparison could not hide behind the tolerance."""
    pytest.importorskip("scipy.stats")
    x = ar1(np.random.default_rng(seed), S, C, phi) + 0.5
    del CS.CUTS[:]
    got = CS.convergence(x)[:, 0]
    assert len(CS.CUTS) == 4 and min(CS.CUTS) > 1e-6, CS.CUTS
    want = alt_dimension(x[:, 0, :])
    for name, g, w in zip(CS.ROWS, got, want):
        assert abs(g - w) <= 1e-9 * abs(w), (name, g, w)


# ---- 2. behaviour ------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,S", [(8, 200), (4, 1000), (70, 80)])
def test_iid_normal_chains_pass(C, S):
    x = np.random.default_rng(10 + C).normal(size=(S, 1, C))
    r = dict(zip(CS.ROWS, CS.convergence(x)[:, 0]))
    N = 2 * C * (S // 2)
    assert r["rhat_bulk"] < 1.01 and r["rhat_tail"] < 1.01, r
    assert 0.8 * N <= r["ess_bulk"] <= N * math.log10(N), r


@pytest.mark.parametrize("phi", [0.5, 0.7])
def test_ar1_bulk_ess_is_near_theory(phi):
    C, S = 8, 2000
    x = ar1(np.random.default_rng(20), S, C, phi)
    r = dict(zip(CS.ROWS, CS.convergence(x)[:, 0]))
    want = C * S * (1.0 - phi) / (1.0 + phi)
    assert abs(r["ess_bulk"] - want) <= 0.2 * want, (r, want)


def test_a_chain_of_another_scale_is_seen_by_the_folded_rhat_only():
    x = np.random.default_rng(30).normal(size=(400, 1, 4))
    x[:, 0, 2] *= 3.0
    r = dict(zip(CS.ROWS, CS.convergence(x)[:, 0]))
    assert exo_rhat(x) < 1.01
    assert r["rhat_tail"] > 1.1 and r["ess_tail"] < 1600 / 10, r


def test_a_shifted_cauchy_chain_is_seen_by_the_rank_normalised_rhat_only():
    """The band is 1.05, not the 1.1 a single prototype run suggested: with 200 000 draws per chain the
    rank-normalised R-hat of this case is 1.1105, and over 30 seeds of 4 x 400 draws it spreads from 1.087
    to 1.144 (sd 0.014), so 1.1 fails one seed in four by chance. 1.05 is that value less four deviations,
    and still far above what converged chains give (< 1.01 above)."""
    x = np.random.default_rng(40).standard_cauchy(size=(400, 1, 4))
    x[:, 0, 1] += 3.0
    r = dict(zip(CS.ROWS, CS.convergence(x)[:, 0]))
    assert exo_rhat(x) < 1.01
    assert r["rhat_bulk"] > 1.05, r


# ---- 3. properties -----------------------------------------------------------------------------------

def test_bulk_rows_are_invariant_under_a_strictly_increasing_map():
    x = ar1(np.random.default_rng(50), 120, 6, 0.4)
    y = np.exp(x)
    assert np.unique(y).size == y.size
    a, b = CS.convergence(x)[:, 0], CS.convergence(y)[:, 0]
    assert a[0] == b[0] and a[2] == b[2]          # ranks only: equal bits
    assert a[4] != b[4]


def test_constant_and_nan_dimensions_are_nan():
    x = np.random.default_rng(60).normal(size=(64, 4, 5))
    x[:, 1, :] = 7.0
    x[17, 2, 3] = np.nan
    x[:, 3, :] = np.arange(5.0)[None, :]           # constant within chains, different between them
    out = CS.convergence(x)
    assert np.all(np.isfinite(out[:, 0]))
    assert np.all(np.isnan(out[:, 1])) and np.all(np.isnan(out[:, 2]))
    # no within-chain variance but the rounding of the means: both R-hats are enormous
    assert out[0, 3] > 100 and out[1, 3] > 100


def test_odd_draw_counts_ignore_the_last_draw():
    x = ar1(np.random.default_rng(70), 101, 5, 0.5, d=2)
    a = CS.convergence(x)
    x[100] = 1e6
    assert np.array_equal(CS.convergence(x), a)
    assert np.array_equal(CS.convergence(x[:100]), a)


# ---- the interface ------------------------------------------------------------------------------------

def test_header_and_binding_name_the_two_entry_points():
    from exmc_amd import _lib
    txt = open(os.path.join(ROOT, "include", "exmc_hip_convergence.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(exmc_hip_\w+)\s*\(", txt))) == sorted(_lib.CONVERGENCE_EXPORTS)
    assert not set(_lib.CONVERGENCE_EXPORTS) & set(_lib.EXPORTS)
    L = _lib.load()
    for name in _lib.CONVERGENCE_EXPORTS:
        assert hasattr(L, name), name
