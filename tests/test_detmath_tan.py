"""exmc_tan_halfpi (include/exmc_detmath.h): tan((pi/2) u) on [0, 1], the tangent inside HalfCauchy.sample
(lib/exmc/dist/half_cauchy.ex:34-40) as the prior walk draws it (DESIGN.md "Prior predictive"). Host build of
the shared header through tests/host/prior_host_shim.c; tests/test_gpu_prior.py holds the device evaluation to
these bits on tan_inputs().

Accuracy is measured against mpmath at 50 digits, in units of the last place of the correctly rounded result.
Measured worst error over tan_inputs(): 1.509 ulp (at u = 0.70211541434789790, in the reciprocal half); the
bound asserted is that figure rounded up to the next half ulp."""
import ctypes as C
import math

import numpy as np
import pytest

import prior_statement as PR

TAN_ULP_BOUND = 2.0
DENORMALS = (5e-324, 1e-320, 3e-315, 1e-310, 2.2250738585072009e-308)


def tan_inputs():
    """every k / 4096, 2e5 random doubles in (0, 1), the 2000 doubles nearest each of 0, 0.5 and 1 (inside
    [0, 1]), denormals"""
    rng = np.random.default_rng(11)
    parts = [np.arange(0, 4097) / 4096.0, rng.random(200_000)]
    for c in (0.0, 0.5, 1.0):
        near, a, b = [c], c, c
        for _ in range(2000):
            a, b = np.nextafter(a, -1.0), np.nextafter(b, 2.0)
            near += [a, b]
        parts.append(np.array([v for v in near if 0.0 <= v <= 1.0]))
    parts.append(np.array(DENORMALS))
    return np.ascontiguousarray(np.concatenate(parts))


def tan_many(L, u):
    u = np.ascontiguousarray(u, dtype=np.float64)
    out = np.empty_like(u)
    dp = C.POINTER(C.c_double)
    L.h_tan_halfpi_n(u.ctypes.data_as(dp), u.size, out.ctypes.data_as(dp))
    return out


@pytest.fixture(scope="module")
def lib():
    return PR.shim()


def test_accuracy_against_fifty_digits(lib):
    import mpmath as mp
    u = tan_inputs()
    got = tan_many(lib, u)
    worst, at = 0.0, None
    with mp.workdps(50):
        halfpi = mp.pi / 2
        for ui, gi in zip(u.tolist(), got.tolist()):
            if ui == 0.0 or ui == 1.0:
                continue            # exact values: the test below
            true = mp.tan(halfpi * mp.mpf(ui))
            err = float(abs(mp.mpf(gi) - true) / mp.mpf(float(np.spacing(abs(float(true))))))
            if err > worst:
                worst, at = err, ui
    print("exmc_tan_halfpi: worst error %.4f ulp at u = %r over %d inputs" % (worst, at, u.size))
    assert worst <= TAN_ULP_BOUND, (worst, at)


def test_exact_values(lib):
    f = lib.h_tan_halfpi
    assert f(0.0) == 0.0 and math.copysign(1.0, f(0.0)) == 1.0
    assert math.copysign(1.0, f(-0.0)) == 1.0 and f(-0.0) == 0.0
    assert f(1.0) == math.inf
    assert f(0.5) == 1.0
    assert math.isnan(f(math.nan))
    for bad in (-5e-324, -1.0, np.nextafter(1.0, 2.0), 2.0, math.inf, -math.inf):
        assert math.isnan(f(bad)), bad
    got = tan_many(lib, tan_inputs())
    assert not np.isnan(got).any() and (got >= 0.0).all()
    assert not np.signbit(got).any()
    # the pole is approached from below: the largest double under 1 gives (2 / pi) 2^53, not a negative number
    assert f(np.nextafter(1.0, 0.0)) == pytest.approx(2.0 ** 53 * 2.0 / math.pi, rel=1e-15)
    # ... and the tangent is monotone across the two hand-overs of the evaluation
    for c in (0.375, 0.5, 0.625):
        x = np.array([np.nextafter(c, 0.0), c, np.nextafter(c, 1.0)])
        y = tan_many(lib, x)
        assert y[0] <= y[1] <= y[2]


def test_symmetry_about_one_half(lib):
    """tan((pi/2) u) tan((pi/2) (1 - u)) = 1: wherever 1 - u is exact the product of the two evaluations is
    within the asserted bound of 1, in units of the last place of 1"""
    u = tan_inputs()
    u = u[(u > 0.0) & (u < 1.0)]
    u = u[(1.0 - (1.0 - u)) == u]
    assert u.size > 8000
    prod = tan_many(lib, u) * tan_many(lib, 1.0 - u)
    dev = np.abs(prod - 1.0) / 2.0 ** -52
    print("symmetry: worst |f(u) f(1 - u) - 1| = %.3f ulp of 1 over %d inputs" % (dev.max(), u.size))
    assert dev.max() <= TAN_ULP_BOUND
