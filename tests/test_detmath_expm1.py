"""exmc_expm1 (include/exmc_detmath.h), the expm1 of PSIS-LOO's generalised-Pareto quantile: host build of
the shared header (through tests/host/psis_host_checker.c) against libm's expm1 over the arguments the
quantile produces, -k log1p(-p) within +-40."""
import math

import numpy as np

import psis_checker as PC


def _ulps(x):
    got = PC.expm1(x)
    want = np.array([math.expm1(v) for v in x])
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_within_two_ulp_of_libm_over_pm40():
    """Stated accuracy: <= 2 ulp against math.expm1 (measured: 2.0, reached only next to the reduction
    boundaries +-ln2/2 where 2 expm1(r) + 1 doubles the error of expm1(r); <= 1 ulp for |x| >= 1.04)."""
    rng = np.random.default_rng(11)
    ln2 = math.log(2.0)
    parts = [rng.uniform(-40, 40, 400_000), rng.uniform(-1.5, 1.5, 400_000), rng.uniform(-1, 1, 100_000) * 1e-3,
             np.sign(rng.uniform(-1, 1, 100_000)) * np.exp(rng.uniform(-700, 0, 100_000))]
    parts += [(k + 0.5) * ln2 + rng.uniform(-1, 1, 1000) * 1e-6 for k in range(-58, 59)]
    x = np.concatenate(parts)
    x = x[np.abs(x) <= 40]
    e = _ulps(x)
    assert e.max() <= 2.0, (e.max(), x[e.argmax()])
    far = np.abs(x) >= 1.04
    assert e[far].max() <= 1.0, e[far].max()


def test_special_values():
    got = PC.expm1(np.array([0.0, -0.0, np.inf, -np.inf, -41.0, -800.0, 5e-324, 1e-300]))
    assert got[0] == 0.0 and not np.signbit(got[0])
    assert got[1] == 0.0 and np.signbit(got[1])
    assert got[2] == np.inf and got[3] == -1.0 and got[4] == -1.0 and got[5] == -1.0
    assert got[6] == 5e-324 and got[7] == 1e-300
    assert np.isnan(PC.expm1(np.array([np.nan]))[0])
    assert abs(PC.expm1(np.array([41.0]))[0] - math.expm1(41.0)) <= np.spacing(math.expm1(41.0))
    assert PC.expm1(np.array([800.0]))[0] == np.inf
