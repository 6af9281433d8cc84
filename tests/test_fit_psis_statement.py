"""The importance diagnostics of the fits on the CPU: the host checker of the device's orders
(tests/host/fit_psis_host_checker.c) against the statement from the papers (tests/fit_psis_statement.py),
the statement against the closed form of a normal pair, and the properties of the contract (DESIGN.md
"Importance diagnostics of the fits"): p = q, systematic resampling, weight-zero samples, NaN groups."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import fit_psis_checker as FC
import fit_psis_statement as FS
import oracle as O
from exmc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ratios(S, F, seed, scale=1.5):
    """log ratios with a heavy right tail and no ties: every tail holds its M samples (no T > 4 edge)"""
    rng = np.random.default_rng(seed)
    return scale * rng.standard_t(4, size=(S, F)) + rng.normal(size=(1, F))


# (S, n_fits, pooled): 200 samples take the n / 5 branch of the tail length, 1000 the 3 sqrt n branch,
# 9100 pooled samples more than two blocks of the cumulative sum and more than one chunk of 64
CASES = [(40, 3, False), (200, 2, False), (1000, 2, False), (30, 70, True), (130, 70, True)]


@pytest.mark.parametrize("S,F,pooled", CASES)
def test_checker_equals_statement(S, F, pooled):
    lr = ratios(S, F, 3 + S)
    R = 257
    want, lw_s, idx_s = FS.groups(lr, pooled, R, seed=11)
    got, lw_c, idx_c = FC.groups(lr, pooled, R, seed=11)
    n = S * F if pooled else S
    assert np.all(want[4] == FS.PS.tail_len(n)) and np.all(want[4] > 4)
    np.testing.assert_array_equal(got[3:], want[3:])                 # n_zero, T
    np.testing.assert_allclose(got[:3], want[:3], rtol=1e-9, atol=0)
    np.testing.assert_allclose(lw_c, lw_s, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(idx_c, idx_s)
    assert np.all(np.isfinite(got[0])) and np.all(got[2] > 1) and np.all(got[2] <= n)


def _normal_pair(s, seed, n=100000):
    """lr of q = N(0, s^2) against p = N(0, 1) at n draws of q"""
    x = np.random.default_rng(seed).normal(0.0, s, size=n)
    return x * x * (1.0 / (s * s) - 1.0) / 2.0 + math.log(s)


@pytest.mark.parametrize("s,tol", [(0.8, 0.172), (0.5, 0.245)])
def test_statement_against_the_closed_form(s, tol):
    """For q = N(0, s^2) and p = N(0, 1) the ratio is s exp(x^2 (1 / s^2 - 1) / 2) with x ~ q, whose
    survival function is t^(-1 / (1 - s^2)) up to a slowly varying factor: the tail index is 1 - s^2.

    The tolerance is twice the largest deviation of the statement's khat from 1 - s^2 over the 20 seeds
    1000 .. 1019 at n = 10^5, measured on the CPU (the Zhang-Stephens estimate is biased at finite n, the
    slowly varying factor pulls it down):
        s = 0.8: mean -0.0119, sd 0.0334, range -0.0859 .. +0.0552, largest 0.0859 -> 0.172
        s = 0.5: mean -0.0516, sd 0.0402, range -0.1223 .. +0.0098, largest 0.1223 -> 0.245
    The test takes seeds of its own."""
    for seed in range(2000, 2005):
        khat = FS.group(_normal_pair(s, seed))["khat"]
        print("s=%g seed=%d khat=%.4f closed form %.4f" % (s, seed, khat, 1 - s * s))
        assert abs(khat - (1 - s * s)) <= tol


@pytest.mark.parametrize("pooled", [False, True])
def test_p_equals_q(pooled):
    S, F = 300, 3
    lr = np.zeros((S, F))
    n = S * F if pooled else S
    for mod in (FC, FS):
        out, lw, _ = mod.groups(lr, pooled)
        assert np.all(out[1] == 0.0)                                   # log_mean_ratio, exactly
        np.testing.assert_allclose(out[2], n, rtol=1e-12, atol=0)      # exp(log n): a few ulps of n
        assert np.all(out[3] == 0.0) and np.all(out[4] == 0.0) and np.all(np.isposinf(out[0]))
    out, lw, _ = FC.groups(lr, pooled)
    assert np.all(lw == -O.lib().exo_det_log(float(n)))
    _, lw, _ = FS.groups(lr, pooled)
    assert np.all(lw == -math.log(n))


@pytest.mark.parametrize("pooled,R", [(False, 64), (False, 1000), (True, 5000), (True, 1)])
def test_resampling(pooled, R):
    S, F = 400, 6
    lr = ratios(S, F, 17)
    seed = 2 ** 40 + 5
    out, lw, idx = FC.groups(lr, pooled, R, seed)
    G = 1 if pooled else F
    n = S * F if pooled else S
    assert idx.shape == (R, G) and idx.min() >= 0 and idx.max() < n
    assert np.all(np.diff(idx, axis=0) >= 0)
    L = O.lib()
    for g in range(G):
        r = O.Rng()
        L.exo_rng_seed(C.byref(r), seed + 7919 * g)
        u = L.exo_rng_uniform(C.byref(r))
        assert FC.first_uniform(seed + 7919 * g) == u == FS.first_uniform(seed + 7919 * g)
        w = np.exp(lw.reshape(-1) if pooled else lw[:, g])
        count = np.bincount(idx[:, g], minlength=n)
        # a sample's count is floor(R w) or ceil(R w); the cumulative sum's rounding may move one
        # position across either end of its interval: at most one off
        assert np.all(count >= np.floor(R * w) - 1) and np.all(count <= np.ceil(R * w) + 1)
        # the positions themselves: index j is the first k whose cumulative weight reaches (u + j) / R
        cum = np.cumsum(w)
        pos = (u + np.arange(R)) / R
        near = np.abs(cum[idx[:, g]] - pos) < 1e-9                        # too close to a boundary to call
        ok = (cum[idx[:, g]] >= pos) & ((idx[:, g] == 0) | (cum[np.maximum(idx[:, g] - 1, 0)] < pos))
        assert np.all(ok | near)


def test_equal_weights_resample_to_the_identity():
    n = 1000
    for pooled, lr in ((False, np.full((n, 2), -3.25)), (True, np.full((n // 4, 4), 7.5))):
        _, _, idx = FC.groups(lr, pooled, n, seed=5)
        assert 1e-3 < FC.first_uniform(5) < 1 - 1e-3
        for g in range(idx.shape[1]):
            np.testing.assert_array_equal(idx[:, g], np.arange(n))


@pytest.mark.parametrize("pooled", [False, True])
def test_weight_zero_samples(pooled):
    """-inf ratios count in n, never enter the tail and are never picked: the group equals the one whose
    zero-weight samples have the ratio -1e300"""
    S, F = 500, 4
    lr = ratios(S, F, 23)
    zero = np.random.default_rng(5).random((S, F)) < 0.3
    a = np.where(zero, -np.inf, lr)
    b = np.where(zero, -1e300, lr)
    R = 2000
    for mod in (FC, FS):
        oa, lwa, ia = mod.groups(a, pooled, R, seed=9)
        ob, lwb, ib = mod.groups(b, pooled, R, seed=9)
        np.testing.assert_array_equal(oa[[0, 1, 2, 4]], ob[[0, 1, 2, 4]])
        np.testing.assert_array_equal(ia, ib)
        assert np.all(np.isneginf(lwa[zero])) and np.all(np.isfinite(lwa[~zero]))
        want_zero = zero.sum() if pooled else zero.sum(axis=0)
        np.testing.assert_array_equal(oa[3], want_zero)
        assert np.all(ob[3] == 0)
        picked = zero.reshape(-1)[ia[:, 0]] if pooled else np.stack([zero[ia[:, g], g] for g in range(F)])
        assert not picked.any()


def test_nan_groups():
    """all weights zero, a NaN, a +inf: the group is NaN and resamples to -1; its neighbours do not change"""
    S, F = 60, 5
    lr = ratios(S, F, 31)
    bad = lr.copy()
    bad[:, 1] = -np.inf
    bad[7, 2] = np.nan
    bad[9, 4] = np.inf
    for mod in (FC, FS):
        out, lw, idx = mod.groups(bad, False, 33, seed=1)
        ref, lwr, idr = mod.groups(lr, False, 33, seed=1)
        for g in (1, 2, 4):
            assert np.all(np.isnan(out[:, g])) and np.all(np.isnan(lw[:, g])) and np.all(idx[:, g] == -1)
        for g in (0, 3):
            np.testing.assert_array_equal(out[:, g], ref[:, g])
            np.testing.assert_array_equal(lw[:, g], lwr[:, g])
            np.testing.assert_array_equal(idx[:, g], idr[:, g])
        out, lw, idx = mod.groups(bad, True, 33, seed=1)
        assert np.all(np.isnan(out)) and np.all(np.isnan(lw)) and np.all(idx == -1)
    d = np.arange(S * 2 * F, dtype=np.float64).reshape(S, 2, F)
    g = FC.gather(d, np.array([[-1, 3, 0, 0, 59]], dtype=np.int32), False)
    assert np.all(np.isnan(g[0, :, 0])) and np.all(g[0, :, 1] == d[3, :, 1]) and np.all(g[0, :, 4] == d[59, :, 4])


def test_tiny_groups_are_not_smoothed():
    lr = ratios(8, 1, 2)
    for pooled in (False, True):
        out, lw, idx = FC.groups(lr, pooled, 8, seed=0)
        want, lws, ids = FS.groups(lr, pooled, 8, seed=0)
        assert np.isposinf(out[0, 0]) and out[4, 0] <= 4
        np.testing.assert_allclose(out[1:3], want[1:3], rtol=1e-9)
        np.testing.assert_array_equal(idx, ids)
    out, lw, idx = FC.groups(np.array([[0.5]]), False, 3, seed=0)      # one sample: all the weight
    assert out[1, 0] == 0.5 and out[2, 0] == 1.0 and lw[0, 0] == 0.0 and np.all(idx == 0)


def test_header_declares_what_the_binding_names():
    txt = open(os.path.join(ROOT, "include", "exmc_hip_fit_psis.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(exmc_hip_\w+)\s*\(", code))) == sorted(_lib.FIT_PSIS_EXPORTS)
    others = (_lib.EXPORTS + _lib.COMPARE_EXPORTS + _lib.PSIS_EXPORTS + _lib.PATHFINDER_EXPORTS + _lib.ADVI_EXPORTS)
    assert not set(_lib.FIT_PSIS_EXPORTS) & set(others)
    assert "__cplusplus" in txt and (_lib.FIT_SIGMA, _lib.FIT_LOG_SIGMA) == (FS.SIGMA, FS.LOG_SIGMA) == (0, 1)
    assert tuple(FC.ROWS) == tuple(_lib.FIT_PSIS_ROWS)
