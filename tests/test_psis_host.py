"""PSIS-LOO on the host: tests/host/psis_host_checker.c (the device's contract, exmc_detmath.h functions and
the stated orders) against tests/psis_statement.py (the published algorithm in numpy / libm), known
answers, and the input matrices the GPU tests share (tests/test_gpu_psis.py)."""
import math

import numpy as np
import pytest

import ic_checker as IC
import psis_checker as PC
import psis_statement as ST

LOG_DBL_MIN = ST.LOG_DBL_MIN


def matrix(S, C, N, seed):
    """ll [S][N][C]: datum i's terms are -|z| scale_i with scales from 0.3 to 6, so that the importance
    ratios exp(-ll) run from thin to very heavy tails (k from below 0 to above 1)"""
    rng = np.random.default_rng(seed)
    scale = np.geomspace(0.3, 6.0, N) if N > 1 else np.array([2.0])
    return np.ascontiguousarray(-np.abs(rng.normal(size=(S, N, C))) * scale[None, :, None] - 0.5)


def ties():
    """64 x 64 samples (M = 192) whose largest 300 lr take three distinct values, in scattered positions.
    Datum 0: 100 of each, so the (M + 1)-th largest is the middle value and the tail is the top 100
    alone, all equal: the fit's grid point b_3 is exactly 0 there (m = 40, sqrt(m / 2.5) = 4), its kappa
    0, and k comes out NaN: nothing is smoothed. Datum 1: 60, 70 and 170 of them, a tail of 130 with two
    distinct values. Datum 2 has every tail value distinct, for comparison."""
    rng = np.random.default_rng(5)
    ll = -np.abs(rng.normal(size=(64, 3, 64)))
    for i, (a, b) in enumerate(((100, 200), (60, 130))):
        flat = ll[:, i, :].reshape(-1)
        pos = rng.permutation(4096)[:300]
        flat[pos[:a]] = -9.0
        flat[pos[a:b]] = -8.5
        flat[pos[b:]] = -8.0
        ll[:, i, :] = flat.reshape(64, 64)
    return np.ascontiguousarray(ll)


def hostile():
    """25 x 8 samples, 7 datums: 0 and 4 ordinary; 2 and 6 have a few terms near -760 / -720 and the
    rest some 700 above, so that all but 13 (datum 2) or 3 (datum 6) of their x lie below log DBL_MIN
    and the cutoff is the floor; 1 holds a NaN, 3 a +inf, 5 a -inf"""
    rng = np.random.default_rng(9)
    ll = -np.abs(rng.normal(size=(25, 7, 8))) * 3.0
    ll[:, 2, :] = rng.uniform(-30.0, 0.0, size=(25, 8))
    ll[::2, 2, 3] = -760.0 + rng.uniform(0.0, 3.0, size=13)
    ll[:, 6, :] = -5.0 + rng.normal(size=(25, 8)) * 0.01
    ll[::9, 6, 1] = -720.0 + rng.uniform(0.0, 1.0, size=3)
    ll[3, 1, 2] = np.nan
    ll[7, 3, 0] = np.inf
    ll[11, 5, 5] = -np.inf
    return np.ascontiguousarray(ll)


CASES = {"n200": lambda: matrix(25, 8, 6, 1), "n4096": lambda: matrix(64, 64, 6, 2),
         "n2590": lambda: matrix(37, 70, 5, 3), "n20": lambda: matrix(5, 4, 3, 4), "ties": ties}


def test_tail_length_and_branches():
    assert [PC.tail_len(n) for n in (20, 200, 4096, 2590, 70000)] == [4, 40, 192, 153, 794]
    assert [ST.tail_len(n) for n in (20, 200, 4096, 2590, 70000)] == [4, 40, 192, 153, 794]


def test_checker_agrees_with_the_statement():
    """The bound is not chosen: the statement is evaluated twice, with left-to-right sums and with
    math.fsum; the largest difference between the two, per output row over all cases, is the estimator's
    own sensitivity to rounding, and the checker must agree with the statement within 16 times that
    (the factor covers the few-ulp differences of exmc_log / exmc_exp from libm over T terms).
    Measured here: sensitivity (elpd_loo, p_loo, k) = (8.6e-14, 8.9e-14, 8.9e-15), so the bounds are
    (1.4e-12, 1.4e-12, 1.4e-13); the checker's largest differences from the statement are
    (8.3e-14, 8.6e-14, 1.0e-14)."""
    sens, diff = np.zeros(3), np.zeros(3)
    for name, make in CASES.items():
        ll = make()
        a, ta = ST.stats(ll, ST.lsum)
        b, tb = ST.stats(ll, math.fsum)
        c, tc = PC.stats_from_ll(ll, tails=True)
        assert list(ta) == list(tb) == list(tc), name
        for v in (b, c):   # k = +inf (T <= 4) and k = NaN (a degenerate fit) in the same places
            assert np.array_equal(np.isinf(a[2]), np.isinf(v[2])), name
            assert np.array_equal(np.isnan(a[2]), np.isnan(v[2])), name
        special = ~np.isfinite(a[2])
        a[2, special] = b[2, special] = c[2, special] = 0.0
        sens = np.maximum(sens, np.abs(a - b).max(axis=1))
        diff = np.maximum(diff, np.abs(c - a).max(axis=1))
    print("sensitivity", sens, "bound", 16 * sens, "checker - statement", diff)
    assert np.all(sens > 0)
    assert np.all(diff <= 16 * sens), (diff, 16 * sens)


def test_ties_leave_a_short_tail_and_small_n_is_not_smoothed():
    out, T = PC.stats_from_ll(ties(), tails=True)
    assert list(T) == [100, 130, 192]
    assert np.all(np.isfinite(out[:2])) and np.isnan(out[2, 0]) and np.all(np.isfinite(out[2, 1:]))
    out, T = PC.stats_from_ll(CASES["n20"](), tails=True)
    assert np.all(T <= 4) and np.all(np.isposinf(out[2]))


def _gpd_tail(k, T=2000, sigma=1.0):
    u = np.random.default_rng(0).uniform(size=T)
    return np.sort(sigma * np.expm1(-k * np.log1p(-u)) / k)


@pytest.mark.parametrize("k", [0.3, 0.9])
def test_known_pareto_tails_fall_on_the_right_side_of_0p7(k):
    t = _gpd_tail(k)
    kc, sc = PC.fit(t)
    ks, ss = ST.gpd_fit([float(v) for v in t])
    for got in (kc, ks):
        assert (got < 0.7) == (k < 0.7), (k, got)
        assert abs(got - k) < 0.1, (k, got)
    assert abs(kc - ks) < 1e-9 and abs(sc - ss) < 1e-9 * ss


def test_all_terms_equal():
    """x = 0 everywhere: no sample lies above the cutoff, T = 0, k = +inf, and every weight is equal, so
    elpd_loo is plain IS-LOO's, -log_mean_exp(-ll) = a. Both form it as (+-a + log n) - log n in
    floating point: each is within half an ulp of |a| + log n of a, hence the bound."""
    a, S, C = -1.37, 16, 8
    ll = np.full((S, 3, C), a)
    out, T = PC.stats_from_ll(ll, tails=True)
    assert list(T) == [0, 0, 0] and np.all(np.isposinf(out[2]))
    plain = IC.stats_from_ll(ll)
    bound = 2.0 ** -52 * (abs(a) + math.log(S * C))
    assert np.all(np.abs(out[0] - plain[2]) <= bound)
    assert np.all(np.abs(out[0] - a) <= bound)
    assert np.all(np.abs(out[1]) <= 2 * bound)
    st, Ts = ST.stats(ll)
    assert list(Ts) == [0, 0, 0] and np.all(np.isposinf(st[2])) and np.all(np.abs(st[0] - a) <= bound)


def test_non_finite_terms_void_their_datum_alone():
    ll = hostile()
    out, T = PC.stats_from_ll(ll, tails=True)
    for i in (1, 3, 5):
        assert np.all(np.isnan(out[:, i]))
    ok = [0, 2, 4, 6]
    assert np.all(np.isfinite(out[:2, ok]))
    clean = PC.stats_from_ll(ll[:, ok, :])
    assert clean.tobytes() == np.ascontiguousarray(out[:, ok]).tobytes()
    st, _ = ST.stats(ll)
    assert np.all(np.isnan(st[:, [1, 3, 5]]))
    # the floor: the cutoff of datums 2 and 6 is log DBL_MIN, not the (M + 1)-th largest x
    for i, want in ((2, 13), (6, 3)):
        v = ll[:, i, :].reshape(-1)
        x = np.sort(v.min() - v)[::-1]
        assert x[PC.tail_len(200)] < LOG_DBL_MIN
        assert T[i] == int(np.sum(x > LOG_DBL_MIN)) == want
    assert np.isfinite(out[2, 2]) and np.isposinf(out[2, 6])
