"""The non-centred sv kind (EXMC_MODEL_SV_NCP) on the host: its checker in the kernel's order
against the reference's order, the generator's resolution of the same IR, a plain-numpy statement
and central differences; its ModelSpec (flat order, init inversion, walk reconstruction)."""
import numpy as np
import pytest

import gen_checker as GC
import sv_ncp_checker as S
from exmc_amd import codegen, models

T = 100
R = np.asarray(models.sv_returns())


def _points(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, T + 2))
    q[:, 0] *= 0.3
    q[:, T] = rng.uniform(np.log(0.02), np.log(1.0), size=n)    # log sigma
    q[:, T + 1] = rng.uniform(np.log(2.0), np.log(60.0), size=n)  # log nu
    return q


def _close(lp_a, g_a, lp_b, g_b):
    assert abs(lp_a - lp_b) <= 1e-12 * max(1.0, abs(lp_b)), (lp_a, lp_b)
    np.testing.assert_allclose(g_a, g_b, rtol=1e-11, atol=1e-12)


def _numpy_statement(r, q):
    """The posterior written again with numpy only: forward walk, autodiff by hand."""
    z, ls, ln = q[:T], q[T], q[T + 1]
    sigma, nu = np.exp(np.clip(ls, -200, 200)), np.exp(np.clip(ln, -200, 200))
    f = np.float32
    s = np.cumsum(np.concatenate([[z[0]], sigma * z[1:]]))
    l2p = float(f(np.log(float(f(2 * np.pi)))))

    def lgam(x):   # math.ex:27-52 (f32 Lanczos coefficients) and its derivative
        c = [float(f(v)) for v in (0.99999999999980993, 676.5203681218851, -1259.1392167224028,
                                   771.32342877765313, -176.61502916214059, 12.507343278686905,
                                   -0.13857109526572012, 9.9843695780195716e-6, 1.5056327351493116e-7)]
        den = x + np.arange(8)
        ag = c[0] + np.sum(np.array(c[1:]) / den)
        dag = -np.sum(np.array(c[1:]) / den ** 2)
        t = x + 6.5
        return (float(f(0.5 * np.log(2 * np.pi))) + (x - 0.5) * np.log(t) - t + np.log(ag),
                np.log(t) + (x - 0.5) / t - 1.0 + dag / ag)

    a1, da1 = lgam((nu + 1) / 2)
    a0, da0 = lgam(nu / 2)
    zz = (np.asarray(r) * np.exp(-s)) ** 2
    w = zz / nu
    lik = np.sum(a1 - a0 - 0.5 * np.log(nu * float(f(np.pi))) - s - (nu + 1) / 2 * np.log1p(w))
    e1 = z[0] / sigma
    prior = (-0.5 * (e1 ** 2 + l2p + 2 * np.log(sigma))) + np.sum(-0.5 * (z[1:] ** 2 + l2p))
    hyp = (float(f(np.log(50.0))) - 50.0 * sigma + ls) + (float(f(np.log(float(f(0.1))))) - float(f(0.1)) * nu + ln)
    gs = -1.0 + (nu + 1) * w / (1 + w)
    A = np.cumsum(gs[::-1])[::-1]
    g = np.zeros(T + 2)
    g[0] = A[0] - e1 / sigma
    g[1:T] = -z[1:] + sigma * A[1:]
    g[T] = (e1 ** 2 - 1) + np.sum(sigma * z[1:] * A[1:]) - 50.0 * sigma + 1.0
    dn = np.sum(0.5 * da1 - 0.5 * da0 - 0.5 / nu - 0.5 * np.log1p(w) + (nu + 1) / 2 * w / (1 + w) / nu)
    g[T + 1] = dn * nu - float(f(0.1)) * nu + 1.0
    return hyp + prior + lik, g


def test_device_order_agrees_with_the_reference_order():
    qs = np.vstack([_points(40, 1), models.sv_ncp(R).to_unconstrained(models.sv_ncp(R).default_init)])
    for q in qs:
        lp_d, g_d = S.logp_grad(R, q, dev=True)
        lp_r, g_r = S.logp_grad(R, q, dev=False)
        _close(lp_d, g_d, lp_r, g_r)


def test_device_scans_are_not_the_sequential_order():
    """The kernel's walk is a scan, not the sequence: some bits differ (else the checker's two modes
    would test nothing), and all agree to rounding."""
    q = _points(1, 2)[0]
    a, b = S.walk(q, dev=True), S.walk(q, dev=False)
    assert not np.array_equal(a, b)
    np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-13)
    assert a[0] == q[0]


def test_checker_agrees_with_the_generated_ncp_text():
    """codegen.generate(sv_ir, ncp=True, lanes=64) resolves s_t = s_{t-1} + sigma z_t the reference's
    way (compiler.ex:444-463); its flat order is the string sort of the names."""
    gen = codegen.generate(codegen.sv_ir(R), ncp=True, lanes=64)
    assert set(gen.ncp_info) == {"s_%d" % t for t in range(2, T + 1)}
    spec = models.sv_ncp(R)
    perm = [spec.var_names.index(n) for n in gen.var_names]
    for q in _points(12, 3):
        lp_g, g_g = GC.logp_grad(gen, q[perm], lanes=64)
        lp_c, g_c = S.logp_grad(R, q, dev=False)
        _close(lp_c, g_c[perm], lp_g, g_g)
        lp_d, g_d = S.logp_grad(R, q, dev=True)
        _close(lp_d, g_d[perm], lp_g, g_g)


def test_checker_agrees_with_a_numpy_statement():
    for q in _points(12, 4):
        lp_n, g_n = _numpy_statement(R, q)
        lp_c, g_c = S.logp_grad(R, q, dev=False)
        assert abs(lp_c - lp_n) <= 1e-11 * max(1.0, abs(lp_n))
        np.testing.assert_allclose(g_c, g_n, rtol=1e-9, atol=1e-10)


def test_gradient_against_central_differences():
    h = 1e-6
    for q in _points(3, 5):
        _, g = S.logp_grad(R, q, dev=False)
        fd = np.zeros_like(q)
        for i in range(q.size):
            a, b = q.copy(), q.copy()
            a[i] += h
            b[i] -= h
            fd[i] = (S.logp_grad(R, a, dev=False)[0] - S.logp_grad(R, b, dev=False)[0]) / (2 * h)
        np.testing.assert_allclose(g, fd, rtol=1e-5, atol=1e-5)


def test_spec_flat_order_names_and_init_are_svs():
    sv, nc = models.sv(R), models.sv_ncp(R)
    assert nc.kind == models.SV_NCP == 7
    assert nc.var_names == sv.var_names and nc.flat_order() == sv.flat_order()
    assert nc.flat_order() == S.sv_flat_order()
    assert nc.default_init == sv.default_init and nc.transforms == sv.transforms
    assert nc.ncp_info["s_2"] == {"mu": "s_1", "sigma": "sigma"} and "s_1" not in nc.ncp_info
    assert np.array_equal(nc.data, sv.data)


def test_spec_init_round_trip_and_reconstruction():
    spec = models.sv_ncp(R)
    rng = np.random.default_rng(6)
    walk = np.cumsum(rng.normal(0, 0.15, T))
    init = {"s_%d" % (t + 1): float(walk[t]) for t in range(T)}
    init.update(sigma=0.15, nu=8.0)
    q = spec.to_unconstrained(init)
    assert q[0] == walk[0]
    np.testing.assert_allclose(q[1:T], np.diff(walk) / 0.15, rtol=1e-12)
    x = spec.constrain(q)
    np.testing.assert_allclose(x[:T], walk, rtol=1e-12, atol=1e-14)
    assert x[T] == np.exp(np.log(0.15)) and x[T + 1] == np.exp(np.log(8.0))
    # the default init (all s_t = 0) maps to all z = 0 and back
    q0 = spec.to_unconstrained(spec.default_init)
    assert np.array_equal(q0, models.sv(R).to_unconstrained(spec.default_init))
    x0 = spec.constrain(q0)
    assert np.array_equal(x0, models.sv(R).constrain(q0))


def test_spec_reconstruction_is_the_sequential_walk_bit_for_bit():
    spec = models.sv_ncp(R)
    draws = _points(7, 8).reshape(7, T + 2)
    x = spec.constrain(draws)
    sigma = np.exp(np.clip(draws[:, T], -200.0, 200.0))
    s = draws[:, 0].copy()
    assert np.array_equal(x[:, 0], s)
    for t in range(1, T):
        s = s + sigma * draws[:, t]
        assert np.array_equal(x[:, t], s), t
    # ... which is the checker's left-to-right walk
    for c in range(7):
        assert np.array_equal(x[c, :T], S.walk(draws[c], dev=False))


def test_generated_spec_ncp_round_trip_unchanged():
    """GeneratedSpec shares the inversion and the reconstruction; what it returns is unchanged."""
    spec = codegen.GeneratedSpec(codegen.generate(codegen.sv_ir(R), ncp=True), "unused", default_init=None)
    nc = models.sv_ncp(R)
    init = {n: 0.0 for n in nc.var_names}
    init.update({"s_1": 0.1, "s_2": -0.2, "s_3": 0.05, "sigma": 0.2, "nu": 5.0})
    q = spec.to_unconstrained(init)
    assert q[spec.var_names.index("s_2")] == (-0.2 - 0.1) / 0.2
    x = spec.constrain(q)
    for n in ("s_1", "s_2", "s_3", "sigma", "nu"):
        assert abs(x[spec.var_names.index(n)] - init[n]) < 1e-12
    with pytest.raises(codegen.CodegenError):
        bad = codegen.GeneratedSpec(codegen.generate(codegen.sv_ir(R), ncp=True), "unused")
        bad.gen.ncp_info = {"s_2": {"mu": "s_3", "sigma": "sigma"}, "s_3": {"mu": "s_2", "sigma": "sigma"}}
        bad.constrain(q)
