"""The inputs of the posterior predictive tests, shared by tests/test_predictive_statement.py (which shows
on the CPU that they take every branch of the samplers) and tests/test_gpu_predictive.py (which holds the
device to the statement on them). TEST INFRASTRUCTURE.

Synthetic traces: 0.5 * normal around each kind's default initial point in the unconstrained space, at
the kinds' own data; for the sv kinds the first ten chains sit around nu = 0.3, below 2, where
sample_gamma's alpha = nu / 2 is below 1 and takes the boost. The statement's replicates of a trace are
computed once per process and shared."""
import numpy as np

import predictive_statement as PS
from exmc_amd import models

KINDS = [models.SIMPLE, models.EIGHT_SCHOOLS, models.SV, models.SV_NCP, models.LOGISTIC, models.RADON]
C_PAR, S_PAR, SEED, CHAIN_LO = 70, 3, 19, 2     # two wavefronts, the second partial
LOW_NU_CHAINS = 10

_specs, _expected = {}, {}


def spec(kind):
    if kind not in _specs:
        _specs[kind] = {models.SIMPLE: models.simple, models.EIGHT_SCHOOLS: models.eight_schools,
                        models.SV: lambda: models.sv(models.sv_returns()),
                        models.SV_NCP: lambda: models.sv_ncp(models.sv_returns()),
                        models.LOGISTIC: models.logistic, models.RADON: models.radon}[kind]()
    return _specs[kind]


def draws(kind, S=S_PAR, Cn=C_PAR):
    """a host trace in the device layout [S][d][C]"""
    sp = spec(kind)
    q0 = np.asarray(sp.to_unconstrained(sp.default_init), dtype=np.float64)
    rng = np.random.default_rng(1000 + kind)
    x = q0[None, :, None] + 0.5 * rng.normal(size=(S, sp.d, Cn))
    if kind in (models.SV, models.SV_NCP):
        x[:, 101, :LOW_NU_CHAINS] += np.log(0.3) - q0[101]
    return np.ascontiguousarray(x)


def hostile(kind, S=2, Cn=70):
    """draws(kind) with rows no sampler would write: NaN, +inf, -inf, 1e308, -1e308 and denormals, each
    in all dimensions of one chain and in single dimensions of others (both wavefronts have some)"""
    x = draws(kind, S, Cn)
    d = x.shape[1]
    bad = [np.nan, np.inf, -np.inf, 1e308, -1e308, 5e-324, -2.5e-310]
    for k, v in enumerate(bad):
        x[:, :, 3 + k] = v                               # a whole row
        x[:, (5 * k + 1) % d, 20 + k] = v                # one dimension
        x[:, d - 1 - (k % min(d, 5)), 64 + (k % 6)] = v  # the scale parameters, second wavefront
        x[0, k % d, 40 + k] = v                          # one draw only
    return x


def expected(kind, which="parity"):
    """(draws, yrep, states, counters) of the statement on the parity or the hostile trace"""
    key = (kind, which)
    if key not in _expected:
        x = draws(kind) if which == "parity" else hostile(kind)
        _expected[key] = (x,) + PS.run(kind, spec(kind).data, x, seed=SEED, chain_lo=CHAIN_LO)
    return _expected[key]
