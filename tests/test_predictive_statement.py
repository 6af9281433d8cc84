"""The statement of posterior predictive sampling (tests/predictive_statement.py) on the CPU: its samplers
draw from the distributions they name; the inputs of the GPU parity test take every branch of the
samplers and never reach the gamma cap; hostile traces terminate. (The NIF table against the Elixir
stub: tests/test_beam_boundary_sources.py.)"""
import math

import numpy as np
import pytest

import predictive_inputs as PI
import predictive_statement as PS
from exmc_amd import models

N_MOMENTS = 20000


def _moments(v):
    v = np.asarray(v)
    return float(v.mean()), float(v.var(ddof=1))


def test_normal_replicates_have_the_mean_and_variance():
    g = PS.Gen(seed=11)
    loc, scale = 1.5, 2.0
    v = [PS.sample_normal(loc, scale, g) for _ in range(N_MOMENTS)]
    mean, var = _moments(v)
    assert abs(mean - loc) <= 5 * scale / math.sqrt(N_MOMENTS)
    # the variance of a normal sample's variance is 2 sigma^4 / (n - 1)
    assert abs(var - scale ** 2) <= 5 * scale ** 2 * math.sqrt(2.0 / (N_MOMENTS - 1))


def test_bernoulli_replicates_have_the_mean_and_variance():
    g = PS.Gen(seed=12)
    p = 0.3
    v = [PS.sample_bernoulli(p, g) for _ in range(N_MOMENTS)]
    assert set(v) == {0.0, 1.0}
    mean, var = _moments(v)
    assert abs(mean - p) <= 5 * math.sqrt(p * (1 - p) / N_MOMENTS)
    # Var(s^2) ~ (mu4 - sigma^4) / n with mu4 = p q (1 - 3 p q)
    pq = p * (1 - p)
    assert abs(var - pq) <= 5 * math.sqrt((pq * (1 - 3 * pq) - pq ** 2) / N_MOMENTS)
    assert PS.sample_bernoulli(math.nan, g) == 0.0


def test_student_t_replicates_have_the_mean():
    g = PS.Gen(seed=13)
    df, loc, scale = 10.0, 0.5, 1.5
    v = [PS.sample_student_t(df, loc, scale, g) for _ in range(N_MOMENTS)]
    mean, _ = _moments(v)
    sd = scale * math.sqrt(df / (df - 2.0))
    assert abs(mean - loc) <= 5 * sd / math.sqrt(N_MOMENTS)
    assert g.n["cap"] == 0 and g.n["boost"] == 0 and g.n["gamma_log_reject"] > 0


def test_gamma_has_the_mean_on_both_sides_of_the_boost():
    for alpha, seed in ((0.4, 14), (3.0, 15)):
        g = PS.Gen(seed=seed)
        v = [PS.sample_gamma(alpha, 0.5, g) for _ in range(N_MOMENTS)]
        mean, _ = _moments(v)
        assert abs(mean - alpha / 0.5) <= 5 * math.sqrt(alpha / 0.25 / N_MOMENTS), alpha
        assert (g.n["boost"] == N_MOMENTS) == (alpha < 1.0)


def test_student_t_replicates_have_the_variance():
    """a wrong rate in the chi-square, or a wrong df under the root, changes the scale and leaves the mean"""
    g = PS.Gen(seed=13)
    df, loc, scale = 10.0, 0.5, 1.5
    v = [PS.sample_student_t(df, loc, scale, g) for _ in range(N_MOMENTS)]
    _, var = _moments(v)
    want = scale ** 2 * df / (df - 2.0)
    # Var(s^2) ~ sigma^4 (2 + excess kurtosis) / n, the t's excess kurtosis 6 / (df - 4)
    assert abs(var - want) <= 5 * want * math.sqrt((2.0 + 6.0 / (df - 4.0)) / N_MOMENTS)


def test_gamma_has_the_variance_on_both_sides_of_the_boost():
    for alpha, seed in ((0.4, 14), (3.0, 15)):
        g = PS.Gen(seed=seed)
        v = [PS.sample_gamma(alpha, 0.5, g) for _ in range(N_MOMENTS)]
        _, var = _moments(v)
        want = alpha / 0.25
        # the gamma's excess kurtosis is 6 / alpha
        assert abs(var - want) <= 5 * want * math.sqrt((2.0 + 6.0 / alpha) / N_MOMENTS), alpha


def test_the_cap_ends_a_loop_that_never_accepts():
    g = PS.Gen(seed=16)
    before = g.state()
    assert math.isnan(PS.sample_gamma(math.nan, 0.5, g))       # every log test compares with NaN
    assert g.n["cap"] == 1 and g.n["gamma_log_reject"] == PS.GAMMA_CAP and g.n["boost"] == 1
    assert g.state() != before                                   # ... and the generator has moved on
    assert 0.0 <= g.uniform() < 1.0


def test_scan_restates_the_walk_of_sv_ncp():
    import sv_ncp_checker as NC
    q = np.random.default_rng(5).normal(size=102)
    sigma = PS._exp(PS.clamp200(float(q[100])))
    s = PS.scan_fwd64([float(q[0]) if i == 0 else (sigma * float(q[i]) if i < 100 else 0.0) for i in range(128)])
    assert np.array(s[:100]).tobytes() == NC.walk(q, dev=True).tobytes()


def test_parity_inputs_take_every_branch_and_never_the_cap():
    total = PS.new_counters()
    for kind in PI.KINDS:
        x, yrep, states, n = PI.expected(kind)
        assert x.shape == (PI.S_PAR, PI.spec(kind).d, PI.C_PAR)
        assert yrep.shape == (PI.S_PAR, PS.n_data(kind, PI.spec(kind).data), PI.C_PAR)
        assert np.isfinite(yrep).all(), kind
        assert n["cap"] == 0, kind
        for k in total:
            total[k] += n[k]
        if kind in (models.SV, models.SV_NCP):
            # the chains around nu = 0.3 boost, the others (nu around 10) do not
            nu = np.exp(x[:, 101, :])
            assert (nu[:, :PI.LOW_NU_CHAINS] < 2.0).all() and (nu[:, PI.LOW_NU_CHAINS:] >= 2.0).all()
            assert n["boost"] == PI.S_PAR * 100 * PI.LOW_NU_CHAINS
            for k in ("zig_wedge", "gamma_v_reject", "gamma_log_reject"):
                assert n[k] > 0, (kind, k)
        if kind == models.LOGISTIC:
            assert set(np.unique(yrep)) == {0.0, 1.0}
    for k in PS.COUNTERS:
        assert (total[k] > 0) == (k != "cap"), (k, total)


@pytest.mark.parametrize("kind", PI.KINDS)
def test_hostile_traces_terminate(kind):
    x, yrep, states, n = PI.expected(kind, "hostile")
    assert not np.isfinite(x).all()
    assert yrep.shape[2] == x.shape[2]
    if kind != models.LOGISTIC:          # a Bernoulli replicate of a NaN p is 0.0
        assert not np.isfinite(yrep).all()
    # chains whose rows were left alone equal the same chains of a clean run
    clean = PS.run(kind, PI.spec(kind).data, PI.draws(kind, 2, 70)[:, :, :3], seed=PI.SEED, chain_lo=PI.CHAIN_LO)[0]
    assert clean.tobytes() == np.ascontiguousarray(yrep[:, :, :3]).tobytes()


def test_continuation_of_the_statement():
    kind = models.SV
    x = PI.draws(kind, 3, 4)
    blob = PI.spec(kind).data
    whole, st, _ = PS.run(kind, blob, x, seed=5, chain_lo=1)
    a, sa, _ = PS.run(kind, blob, x[:1], seed=5, chain_lo=1)
    b, sb, _ = PS.run(kind, blob, x[1:], states=sa)
    assert np.concatenate([a, b]).tobytes() == whole.tobytes() and sb.tobytes() == st.tobytes()
