"""Generator coverage added in round 2: vector free RVs with a scalar-valued
distribution (GaussianRandomWalk dist/gaussian_random_walk.ex:21-57, MvNormal
dist/mv_normal.ex:20-47), Custom-distribution closures over a declarative op set (dist/custom.ex;
validate_posteriordb.exs:279-295), meas_obs (compiler.ex:258-266, 342-369). Checked on the CPU: the
generated text compiled for the host against an independent numpy/scipy evaluation of the same
densities, the gradient against central differences, the flat layout against PointMap's rule."""
import math

import numpy as np
import pytest
from scipy import stats

import gen_checker as GC
import gen_models as GM
import oracle as O
from exmc_amd import codegen as cg

DET = O.Cfg(1, 1)


def _split(q):
    # ids sorted as strings: c, m, sigma, tau, w  (point_map.ex:37)
    return dict(c=q[0], m=q[1:4], lsig=q[4], ltau=q[5], w=q[6:12])


def scipy_logp(q, ir):
    v = _split(q)
    sigma, tau = math.exp(v["lsig"]), math.exp(v["ltau"])
    n = ir.nodes
    lp = stats.expon.logpdf(sigma, scale=1 / 2.0) + v["lsig"]                      # sigma + log-Jacobian
    w = v["w"]
    lp += stats.norm.logpdf(w[0], 0.0, sigma) + np.sum(stats.norm.logpdf(np.diff(w), 0.0, sigma))   # GRW
    lp += stats.multivariate_normal.logpdf(v["m"], n["m"]["params"]["mu"], n["m"]["params"]["cov"])
    lp += stats.halfcauchy.logpdf(tau, scale=2.0) + v["ltau"]
    lp += stats.norm.logpdf(v["c"], 0.0, 3.0)
    lp += np.sum(stats.norm.logpdf(n["y"]["value"], w, 0.5))                         # vector obs, mean = w
    s = np.array([1.0, 2.0, 0.7])
    z = (n["z"]["value"] - (v["c"] + tau * v["m"])) / s
    lp += np.sum(-0.5 * z * z - np.log(s))                                           # the Custom closure
    lp += stats.norm.logpdf((3.0 - 1.0) / 2.0, 1.0, 2.0) - math.log(2.0)             # affine meas_obs
    a = np.array([[2.0, 1.0], [0.0, 3.0]])
    x = np.linalg.solve(a, n["v"]["value"])
    lp += np.sum(stats.norm.logpdf(x, 0.0, 1.0) - math.log(abs(np.linalg.det(a))))  # matmul meas_obs
    return lp


def test_layout_follows_point_map():
    gen = cg.generate(GM.walk_ir())
    assert gen.d == 12
    assert gen.var_names == ["c", "m[0]", "m[1]", "m[2]", "sigma", "tau"] + ["w[%d]" % i for i in range(6)]
    assert gen.vector_entries == {"m": (1, 3), "w": (6, 6)}
    assert gen.transforms == {"sigma": "log", "tau": "log"}
    assert gen.lanes == 1                                     # no plate layout for these node kinds


def test_value_against_scipy_and_gradient_against_central_differences():
    ir = GM.walk_ir()
    gen = cg.generate(ir)
    rng = np.random.default_rng(0)
    for _ in range(12):
        q = rng.normal(size=gen.d) * 0.6
        lp, g = GC.logp_grad(gen, q)
        want = scipy_logp(q, ir)
        assert abs(lp - want) <= 2e-6 * (1 + abs(want)), (lp, want)
        for i in range(gen.d):
            h = 1e-6
            e = np.zeros(gen.d); e[i] = h
            fd = (GC.logp_grad(gen, q + e)[0] - GC.logp_grad(gen, q - e)[0]) / (2 * h)
            assert abs(fd - g[i]) <= 2e-5 * (1 + abs(g[i])), (i, fd, g[i])


def test_meas_obs_is_a_constant_of_the_data():
    """compiler.ex:258-266: eager -- dropping the meas_obs nodes shifts logp by a constant and leaves
    the gradient untouched."""
    ir = GM.walk_ir()
    ir2 = cg.IR()
    for id_, n in ir.nodes.items():
        if n["op"] != "meas_obs" and id_ not in ("k_rv", "v_rv"):
            ir2.nodes[id_] = n
    ga, gb = cg.generate(ir), cg.generate(ir2)
    rng = np.random.default_rng(1)
    shifts = []
    for _ in range(5):
        q = rng.normal(size=ga.d) * 0.5
        la, gra = GC.logp_grad(ga, q)
        lb, grb = GC.logp_grad(gb, q)
        shifts.append(la - lb)
        np.testing.assert_allclose(gra, grb, rtol=1e-13, atol=1e-13)
    assert np.ptp(shifts) < 1e-12 and abs(shifts[0]) > 0.1


def test_doctest_literals_of_the_vector_distributions():
    # mv_normal.ex:13-14: logpdf([0, 0]; mu 0, cov I) = -1.8379
    ir = cg.IR()
    ir.rv("x", "mv_normal", dict(mu=[0.0, 0.0], cov=[[1.0, 0.0], [0.0, 1.0]]))
    gen = cg.generate(ir)
    assert round(GC.logp_grad(gen, np.zeros(2))[0], 4) == -1.8379
    # gaussian_random_walk.ex:12-15 (no expected value printed there): x = [0.1, 0.2, 0.15], sigma 1
    ir = cg.IR()
    ir.rv("s", "exponential", {"lambda": 1.0}, transform="log")
    ir.rv("x", "gaussian_random_walk", dict(sigma="s", steps=3))
    gen = cg.generate(ir)
    lp = GC.logp_grad(gen, np.array([0.0, 0.1, 0.2, 0.15]))[0]        # s = exp(0) = 1 (+ Exponential(1) term -1)
    want = sum(stats.norm.logpdf(d, 0.0, 1.0) for d in (0.1, 0.1, -0.05)) - 1.0
    assert abs(lp - want) < 1e-6


def test_refusals():
    with pytest.raises(cg.CodegenError):
        cg.generate(GM.walk_only_ir(3, transform="log"))
    ir = GM.walk_only_ir(25)                                            # 25 flat dimensions > 20:
    gen = cg.generate(ir)                                               # the lane layout since round 3
    assert gen.lanes == 16 and gen.lane_layout["family_sizes"] == [24]
    x = np.cumsum(np.random.default_rng(0).normal(size=25))
    want = sum(stats.norm.logpdf(d, 0.0, 1.0) for d in np.diff(np.concatenate([[0.0], x])))
    assert abs(GC.logp_grad(gen, x, lanes=16)[0] - want) < 1e-6
    with pytest.raises(cg.CodegenError):
        cg.generate(GM.meas_ref_param_ir())
    with pytest.raises(cg.CodegenError):
        cg.IR().meas_obs("k", "x", 1.0, ("exp",))


def test_sampling_through_the_checker_and_trace_grouping():
    """The whole sampler path on the generated model (CPU checker running the generated text)."""
    gen = cg.generate(GM.walk_ir())
    m = GC.model(gen, 1)

    spec = cg.GeneratedSpec(gen, "/nonexistent.so", default_init=GM.WALK_INIT)
    q0 = spec.to_unconstrained(GM.WALK_INIT)
    assert q0.shape == (12,) and q0[4] == math.log(0.5) and list(q0[6:12]) == GM.WALK_INIT["w"]
    assert spec.flat_order() == list(range(12))
    t, st = O.sample(m, q0, num_warmup=150, num_samples=150, seed=2, cfg=DET)
    # (a centred random walk under a free scale is a funnel: divergences are the sampler reporting
    # it, as the reference would; value and gradient are checked above)
    assert 0.001 < st.step_size < 2.0 and np.all(np.isfinite(t["draws"])) and t["n_steps"].min() >= 1
    from exmc_amd import sampler
    tr = sampler._build_trace(spec, t["draws"])
    assert tr["w"].shape == (150, 6) and tr["m"].shape == (150, 3)
    assert np.array_equal(tr["w"][:, 2], tr["w[2]"]) and np.all(tr["sigma"] > 0)
