"""PSIS-LOO-PIT on the host: tests/host/loo_pit_host_checker.c (the device's contract, exmc_detmath.h
functions and the stated orders) against tests/loo_pit_statement.py (the definition in numpy / libm), and the
edge cases of the contract (include/exmc_hip_loo_pit.h): constant terms, non-finite terms, NaN replicates,
too few samples to smooth."""
import math

import numpy as np

import loo_pit_checker as LC
import loo_pit_statement as LS
import ppc_statement as PPC
import psis_checker as PC


def case(S, C, N, seed):
    """ll, yrep [S][N][C] and y [N]. Datum i's terms are -|z| scale_i - 0.5 with scales from 0.3 to 6, so that
    the importance ratios run from thin to very heavy tails (k from below 0 to above 1). Even datums are
    continuous (normal replicates, the observation at a quantile that moves with i); odd datums are counts
    (round(2 z)), whose observation ties with many replicates, so that p_eq > 0. The replicates lean on
    the terms (a low term comes with a replicate far out), as a model's would: the weights matter."""
    rng = np.random.default_rng(seed)
    scale = np.geomspace(0.3, 6.0, N) if N > 1 else np.array([2.0])
    z = rng.normal(size=(S, N, C))
    ll = np.ascontiguousarray(-np.abs(z) * scale[None, :, None] - 0.5)
    yrep = z + 0.3 * rng.normal(size=(S, N, C))
    yrep[:, 1::2, :] = np.round(2.0 * yrep[:, 1::2, :])
    y = np.linspace(-1.2, 1.2, N) if N > 1 else np.array([0.4])
    y[1::2] = np.round(2.0 * y[1::2])
    return ll, np.ascontiguousarray(yrep), np.ascontiguousarray(y)


# n = 200: one block; 4096: one full block; 37 x 70: two blocks, the second of 6 chains; 7 x 130: three blocks
CASES = {"n200": (25, 8, 6, 1), "n4096": (64, 64, 6, 2), "n2590": (37, 70, 5, 3), "n910": (7, 130, 6, 4)}
ROWS = ("p_lt", "p_eq", "pit", "k")


def test_checker_agrees_with_the_statement():
    """The bound is not chosen: the statement is evaluated twice, with left-to-right sums and with
    math.fsum; the largest difference between the two, per output row over all cases, is the estimator's own
    sensitivity to rounding, and the checker must agree with the statement within 16 times that (the rule
    of tests/test_psis_host.py: the factor covers the few-ulp differences of exmc_log / exmc_exp from libm
    over the terms of a sum).
    Measured here: sensitivity (p_lt, p_eq, pit, k) = (1.7e-15, 2.5e-16, 1.7e-15, 8.9e-15), so the bounds are
    (2.8e-14, 4.0e-15, 2.8e-14, 1.4e-13); the checker's largest differences from the statement are
    (2.3e-15, 2.2e-16, 2.3e-15, 1.0e-14)."""
    sens, diff = np.zeros(4), np.zeros(4)
    for name, shape in CASES.items():
        ll, yrep, y = case(*shape)
        a, ta = LS.run(ll, yrep, y, LS.lsum)
        b, tb = LS.run(ll, yrep, y, math.fsum)
        c, tc = LC.run(ll, yrep, y, tails=True)
        assert list(ta) == list(tb) == list(tc), name
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(np.isfinite(c)), name
        assert np.all(a[1, 1::2] > 0) and np.all(a[1, 0::2] == 0), name       # ties where the data are counts
        # k is PSIS-LOO's, bit for bit
        assert c[3].tobytes() == PC.stats_from_ll(ll)[2].tobytes(), name
        sens = np.maximum(sens, np.abs(a - b).max(axis=1))
        diff = np.maximum(diff, np.abs(c - a).max(axis=1))
    print("sensitivity", dict(zip(ROWS, sens)), "bound", dict(zip(ROWS, 16 * sens)), "checker - statement",
          dict(zip(ROWS, diff)))
    assert np.all(sens > 0)
    assert np.all(diff <= 16 * sens), (diff, 16 * sens)


def test_the_weights_matter():
    """on these cases LOO-PIT is not the plain PIT: the smoothed weights move every datum"""
    ll, yrep, y = case(*CASES["n2590"])
    out = LC.run(ll, yrep, y)
    plain = PPC.run(yrep, y)
    assert np.all(np.abs(out[2] - plain["pit"]) > 1e-3)


def test_constant_terms_give_the_plain_pit():
    """ll constant per datum: x = 0 for every sample, no sample lies above the cutoff (T = 0, k = +inf),
    and every weight is exp(0) = 1 exactly. sA, sL and sQ are then sums of at most n ones, exact integers
    below 2^53 in any order and across the merge (m == m2 adds), so p_lt = n_lt / n and p_eq = n_eq / n
    are the very divisions the plain PIT makes: the difference is 0. The bound n 2^-53 is what a statement
    that rounded each of its n additions by half an ulp of a sum below 1 could differ by; both stay
    inside it."""
    S, C, N = 9, 70, 6
    _, yrep, y = case(S, C, N, 11)
    ll = np.broadcast_to(np.linspace(-3.0, -0.1, N)[None, :, None], (S, N, C)).copy()
    n = S * C
    bound = n * 2.0 ** -53
    plain = PPC.run(yrep, y)
    out, T = LC.run(ll, yrep, y, tails=True)
    st, Ts = LS.run(ll, yrep, y)
    assert list(T) == list(Ts) == [0] * N
    for got in (out, st):
        assert np.all(np.isposinf(got[3]))
        assert np.all(np.abs(got[0] - plain["p_lt"]) <= bound)
        assert np.all(np.abs(got[1] - plain["p_eq"]) <= bound)
        assert np.all(np.abs(got[2] - plain["pit"]) <= bound)
    assert np.any(plain["p_eq"] > 0)


def test_non_finite_terms_void_their_datum_alone():
    ll, yrep, y = case(25, 70, 7, 5)
    ll[3, 1, 2] = np.nan
    ll[7, 3, 0] = np.inf
    ll[11, 5, 69] = -np.inf
    out = LC.run(ll, yrep, y)
    st, _ = LS.run(ll, yrep, y)
    for i in (1, 3, 5):
        assert np.all(np.isnan(out[:, i])) and np.all(np.isnan(st[:, i]))
    ok = [0, 2, 4, 6]
    assert np.all(np.isfinite(out[:, ok]))
    clean = LC.run(ll[:, ok, :], yrep[:, ok, :], y[ok])
    assert clean.tobytes() == np.ascontiguousarray(out[:, ok]).tobytes()


def test_a_nan_replicate_counts_in_neither_set():
    """... but its weight stays in the denominator: the same numbers as with a replicate above the
    observation in its place, and p_lt + p_eq < 1"""
    ll, yrep, y = case(25, 70, 4, 6)
    holes = np.zeros(yrep.shape, bool)
    holes[::3, :, 5] = True
    holes[4, 1, :] = True
    a = LC.run(ll, np.where(holes, np.nan, yrep), y)
    b = LC.run(ll, np.where(holes, np.inf, yrep), y)
    assert a.tobytes() == b.tobytes() and np.all(np.isfinite(a))
    assert a.tobytes() != LC.run(ll, yrep, y).tobytes()
    everywhere = LC.run(ll, np.full(yrep.shape, np.nan), y)
    assert np.all(everywhere[:3] == 0.0) and everywhere[3].tobytes() == a[3].tobytes()
    st, _ = LS.run(ll, np.where(holes, np.nan, yrep), y)
    assert np.all(np.abs(st[:3] - a[:3]) < 1e-12)


def test_small_n_is_not_smoothed():
    """n = 20: M = 4, T <= 4, nothing is smoothed: k = +inf and the PIT is that of the raw weights"""
    ll, yrep, y = case(5, 4, 3, 7)
    out, T = LC.run(ll, yrep, y, tails=True)
    assert np.all(T <= 4) and np.all(np.isposinf(out[3])) and np.all(np.isfinite(out[:3]))
    st, _ = LS.run(ll, yrep, y)
    assert np.all(np.isposinf(st[3])) and np.all(np.abs(st[:3] - out[:3]) < 1e-14)
    for i in range(3):
        w = np.exp(-(ll[:, i, :].reshape(-1)))
        v = yrep[:, i, :].reshape(-1)
        assert abs(out[0, i] - w[v < y[i]].sum() / w.sum()) < 1e-14
