"""The statement of prior sampling (tests/prior_statement.py) on the CPU: the Kahn order of every kind, sv and
sv_ncp pinned literally; HalfCauchy and Exponential draw from the laws they name, and the sv walk's increments
are standard normal; a generator that holds 0.0 gives the stated values and goes on; the inputs of the GPU
parity tests never reach the gamma cap. (The BEAM side as source files: tests/test_beam_boundary_sources.py.)"""
import math

import numpy as np
import pytest

import predictive_inputs as PI
import predictive_statement as PS
import prior_statement as PR
from exmc_amd import models

N_DRAWS = 20000


def _order(kind):
    sp = PI.spec(kind)
    return PR.kahn_order(PR.prior_table(kind, sp.var_names))


@pytest.mark.parametrize("kind", [models.SIMPLE, models.EIGHT_SCHOOLS, models.LOGISTIC, models.RADON])
def test_kinds_without_parents_walk_in_string_order(kind):
    sp = PI.spec(kind)
    assert _order(kind) == sorted(sp.var_names)
    # ... which is the handle's flat order (point_map.ex:37)
    assert _order(kind) == [sp.var_names[i] for i in sp.flat_order()]


def test_sv_order_is_pinned():
    assert _order(models.SV) == ["nu", "sigma"] + ["s_%d" % t for t in range(1, 101)]


def test_sv_ncp_order_is_pinned():
    """the rewritten s_2 .. s_100 have no parents: string order, before sigma; s_1 waits for sigma"""
    free = sorted("s_%d" % t for t in range(2, 101))
    assert free[:4] == ["s_10", "s_100", "s_11", "s_12"] and free[-1] == "s_99"
    assert _order(models.SV_NCP) == ["nu"] + free + ["sigma", "s_1"]


def test_kahn_takes_the_smallest_ready_id():
    t = {"b": ("normal", (0.0, "z"), None), "z": ("exponential", (1.0,), "log"), "a": ("normal", ("b", 1.0), None),
         "c": ("normal", (0.0, 1.0), None)}
    assert PR.kahn_order(t) == ["c", "z", "b", "a"]


def _cdf_check(v, cdf, points):
    v = np.asarray(v)
    for t in points:
        F = cdf(t)
        assert abs(float(np.mean(v <= t)) - F) <= 5 * math.sqrt(F * (1 - F) / v.size), t


def test_half_cauchy_draws_from_its_law():
    g = PS.Gen(seed=21)
    scale = 2.5
    v = [PR.sample_half_cauchy(scale, g) for _ in range(N_DRAWS)]
    assert min(v) >= 0.0
    _cdf_check(v, lambda t: (2.0 / math.pi) * math.atan(t / scale), [0.05, 0.5, 1.0, 2.5, 6.0, 25.0, 250.0, 2500.0])


def test_exponential_draws_from_its_law():
    g = PS.Gen(seed=22)
    lam = PR.F32_TENTH
    v = [PR.sample_exponential(lam, g) for _ in range(N_DRAWS)]
    assert min(v) > 0.0
    _cdf_check(v, lambda t: 1.0 - math.exp(-lam * t), [0.1, 1.0, 5.0, 10.0, 30.0, 60.0])
    mean = float(np.mean(v))
    assert abs(mean - 1.0 / lam) <= 5 * (1.0 / lam) / math.sqrt(N_DRAWS)


@pytest.mark.parametrize("kind", [models.SV, models.SV_NCP])
def test_sv_increments_are_standard_normal(kind):
    sp = PI.spec(kind)
    S = N_DRAWS // 100
    x, q, _, _ = PR.prior_samples(sp, S, seed=23, replicates=False)
    sigma = x[:, 100]
    if kind == models.SV_NCP:       # the walk is rebuilt from q: its sigma is exp(clamp200(log sigma))
        sigma = np.array([PS._exp(PS.clamp200(float(v))) for v in q[:, 100]])
    s = x[:, :100]
    z = np.concatenate([s[:, :1], np.diff(s, axis=1)], axis=1) / sigma[:, None]
    z = z.ravel()
    assert z.size == N_DRAWS
    assert abs(float(z.mean())) <= 5 / math.sqrt(z.size)
    assert abs(float(z.var(ddof=1)) - 1.0) <= 5 * math.sqrt(2.0 / (z.size - 1))
    # q is the unconstrained position of x
    assert np.allclose(np.exp(q[:, 100:]), x[:, 100:], rtol=1e-14)
    if kind == models.SV:
        assert np.array_equal(q[:, :100], x[:, :100])
    else:
        assert np.array_equal(q[:, 0], x[:, 0]) and not np.array_equal(q[:, 1:100], x[:, 1:100])


class _Forced(PS.Gen):
    """a generator whose next uniforms are given"""

    def __init__(self, forced, seed):
        super().__init__(seed=seed)
        self.forced = list(forced)

    def uniform(self):
        return self.forced.pop(0) if self.forced else super().uniform()


def test_a_zero_uniform_gives_the_stated_values_and_the_walk_goes_on():
    g = _Forced([0.0, 0.0], seed=5)
    assert PR.sample_exponential(50.0, g) == math.inf
    assert PR.sample_half_cauchy(2.5, g) == 0.0
    assert 0.0 < PR.sample_exponential(50.0, g) < math.inf
    # a whole draw of simple: sigma = +inf, its position +inf, and the datums' scale exp(200)
    sp = PI.spec(models.SIMPLE)
    g = _Forced([0.0], seed=6)
    x, q, yrep, _ = PR.prior_samples(sp, 2, gen=g)
    assert x[0, 1] == math.inf and q[0, 1] == math.inf and np.isfinite(x[0, 0])
    assert np.isfinite(yrep[0]).all() and np.abs(yrep[0]).max() > 1e80
    assert np.isfinite(x[1]).all() and np.isfinite(q[1]).all() and np.isfinite(yrep[1]).all()
    # eight_schools: tau = 0.0, log tau = -inf, the datums collapse onto mu
    sp = PI.spec(models.EIGHT_SCHOOLS)
    g = _Forced([0.0], seed=7)
    x, q, yrep, _ = PR.prior_samples(sp, 1, gen=g)
    assert x[0, 1] == 0.0 and q[0, 1] == -math.inf and np.isfinite(yrep).all()


def test_parity_inputs_never_reach_the_gamma_cap():
    total = PS.new_counters()
    for kind in PI.KINDS:
        for Cn in (PR.C_PAR, 1):
            x, q, yrep, states, n = PR.expected(kind, Cn)
            sp = PI.spec(kind)
            assert x.shape == q.shape == (PR.S_PAR, sp.d, Cn)
            assert yrep.shape == (PR.S_PAR, PS.n_data(kind, sp.data), Cn)
            assert n["cap"] == 0, kind
            assert np.isfinite(x).all() and np.isfinite(q).all(), kind
            assert not np.isnan(yrep).any(), kind
            for k in total:
                total[k] += n[k]
    assert total["boost"] > 0 and total["zig_wedge"] > 0 and total["gamma_log_reject"] > 0


def test_continuation_and_no_replicates():
    sp = PI.spec(models.EIGHT_SCHOOLS)
    whole = PR.run(sp, 5, 3, seed=5, chain_lo=1)
    a = PR.run(sp, 2, 3, seed=5, chain_lo=1)
    b = PR.run(sp, 3, 3, states=a[3])
    for k in range(3):
        assert np.concatenate([a[k], b[k]]).tobytes() == whole[k].tobytes()
    assert b[3].tobytes() == whole[3].tobytes()
    bare = PR.run(sp, 2, 3, seed=5, chain_lo=1, replicates=False)
    assert bare[2] is None and bare[0][0].tobytes() == a[0][0].tobytes()
    assert bare[0][1].tobytes() != a[0][1].tobytes()          # the generator did not advance for the datums
