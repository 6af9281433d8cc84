"""Builder-IR test models for the generator (exmc_amd/codegen.py), shared by CPU and GPU tests."""
import numpy as np

from exmc_amd import codegen as cg


simple_ir = cg.simple_ir
eight_schools_ir = cg.eight_schools_ir


def zoo_ir(seed=5):
    """Every covered distribution and transform at least once; d = 9."""
    rng = np.random.default_rng(seed)
    ir = cg.IR()
    ir.rv("a_loc", "cauchy", dict(loc=0.5, scale=2.0))
    ir.rv("b_scale", "half_normal", dict(sigma=2.0), transform="softplus")
    ir.rv("c_df", "exponential", {"lambda": 0.2}, transform="log")
    ir.rv("d_p", "normal", dict(mu=0.0, sigma=1.5), transform="logit")
    ir.rv("e_lap", "laplace", dict(mu="a_loc", b="b_scale"))
    ir.rv("f_ln", "lognormal", dict(mu=0.1, sigma=0.7), transform="log")
    ir.rv("g_t", "student_t", dict(df="c_df", loc="a_loc", scale="f_ln"))
    ir.rv("h_hc", "half_cauchy", dict(scale="b_scale"), transform="log")
    ir.rv("i_centered", "normal", dict(mu="a_loc", sigma=1.0))   # one ref only: no NCP
    ir.rv("t_obs_rv", "student_t", dict(df=4.0, loc="e_lap", scale="h_hc"))
    ir.obs("t_obs", "t_obs_rv", rng.normal(size=7) * 2.0)
    ir.rv("n_obs_rv", "normal", dict(mu="i_centered", sigma=np.abs(rng.normal(size=5)) + 0.5))
    ir.obs("n_obs", "n_obs_rv", rng.normal(size=5))
    ir.rv("bern_rv", "bernoulli", dict(p="d_p"))
    ir.obs("bern", "bern_rv", (rng.uniform(size=9) < 0.4).astype(float))
    ir.rv("l_obs_rv", "laplace", dict(mu="g_t", b=1.3))
    ir.obs("l_obs", "l_obs_rv", 0.25)
    return ir


ZOO_INIT = dict(a_loc=0.3, b_scale=1.2, c_df=5.0, d_p=0.4, e_lap=-0.2, f_ln=0.9, g_t=0.1, h_hc=1.5,
                i_centered=0.0)


def walk_ir(seed=3):
    """Round-2 generator coverage in one model (d = 12): a GaussianRandomWalk latent path driven by a
    log-scale rv, an MvNormal block with a constant covariance, a Custom-distribution likelihood
    written as a closure over the declarative op set (the shape of validate_posteriordb.exs:279-295),
    a vector obs whose mean is the random walk, and two meas_obs terms (affine, matmul)."""
    rng = np.random.default_rng(seed)
    ir = cg.IR()
    ir.rv("sigma", "exponential", {"lambda": 2.0}, transform="log")
    ir.rv("w", "gaussian_random_walk", dict(sigma="sigma", steps=6))
    cov = np.array([[1.0, 0.3, 0.1], [0.3, 2.0, 0.2], [0.1, 0.2, 1.5]])
    ir.rv("m", "mv_normal", dict(mu=[0.1, -0.2, 0.3], cov=cov))
    ir.rv("tau", "half_cauchy", dict(scale=2.0), transform="log")
    ir.rv("c", "normal", dict(mu=0.0, sigma=3.0))
    ir.rv("y_rv", "normal", dict(mu="w", sigma=0.5))
    ir.obs("y", "y_rv", rng.normal(size=6) * 0.4)

    def lik(o, x, p):
        # sum_j Normal(x_j; c + tau * m_j, s_j) up to the constant the posteriordb script drops
        terms = []
        for xj, mj, sj in zip(x, p["m"], p["s"]):
            z = o.div(o.sub(xj, o.add(p["c"], o.mul(p["tau"], mj))), sj)
            terms.append(o.sub(o.mul(o.lit(-0.5), o.mul(z, z)), o.log(sj)))
        return o.sum(terms)
    ir.rv("z_rv", "custom", dict(logpdf=lik, m="m", c="c", tau="tau", s=[1.0, 2.0, 0.7]))
    ir.obs("z", "z_rv", [0.4, -1.1, 2.0])
    ir.rv("k_rv", "normal", dict(mu=1.0, sigma=2.0))
    ir.meas_obs("k", "k_rv", 3.0, ("affine", 2.0, 1.0))
    ir.rv("v_rv", "normal", dict(mu=0.0, sigma=1.0))
    ir.meas_obs("v", "v_rv", [0.5, -0.25], ("matmul", [[2.0, 1.0], [0.0, 3.0]]))
    return ir


WALK_INIT = dict(sigma=0.5, w=[0.0, 0.1, 0.0, -0.1, 0.05, 0.0], m=[0.0, 0.0, 0.0], tau=1.0, c=0.2)


def simplex_ir(seed=7):
    """The distributions added at the end of round 2 (d = 8): a Dirichlet rv on the 4-simplex behind
    the stick-breaking transform, Gamma / Beta / Weibull / Uniform01 free rvs with their default
    transforms, a Poisson likelihood whose rate is the Gamma rv, Gamma- and Weibull-distributed
    observations, and a Dirichlet-distributed observation."""
    rng = np.random.default_rng(seed)
    ir = cg.IR()
    ir.rv("theta", "dirichlet", dict(alpha=[2.0, 1.5, 1.0, 3.0]), transform="stick_breaking")
    ir.rv("rate", "gamma", dict(alpha=3.0, beta=2.0), transform="log")
    ir.rv("p", "beta", dict(alpha=2.0, beta=5.0), transform="logit")
    ir.rv("k", "weibull", {"k": 1.5, "lambda": 2.0}, transform="log")
    ir.rv("u", "uniform01", {}, transform="logit")
    ir.rv("cnt_rv", "poisson", dict(mu="rate"))
    ir.obs("cnt", "cnt_rv", rng.poisson(1.5, size=6).astype(float))
    ir.rv("wait_rv", "weibull", {"k": "k", "lambda": 1.3})
    ir.obs("wait", "wait_rv", rng.weibull(1.5, size=5) * 1.3 + 0.05)
    ir.rv("g_rv", "gamma", dict(alpha=2.5, beta="rate"))
    ir.obs("g", "g_rv", rng.gamma(2.5, 0.6, size=4) + 0.05)
    ir.rv("b_rv", "bernoulli", dict(p="p"))
    ir.obs("b", "b_rv", (rng.uniform(size=7) < 0.3).astype(float))
    ir.rv("mix_rv", "dirichlet", dict(alpha=[4.0, 2.0, 1.0, 1.0]))
    ir.obs("mix", "mix_rv", [0.4, 0.3, 0.2, 0.1])
    ir.rv("n_rv", "normal", dict(mu="u", sigma=0.5))
    ir.obs("n", "n_rv", 0.6)
    return ir


SIMPLEX_INIT = dict(theta=[0.25, 0.25, 0.25, 0.25], rate=1.0, p=0.3, k=1.2, u=0.5)


def survival_ir(seed=11):
    """The Builder.obs meta and the remaining distributions (d = 6): right-censored Weibull survival
    times and exact ones, left- / right- / interval-censored Normal measurements, a weighted and
    masked vector obs, reduce :mean and :logsumexp, an observation of a :log-transformed rv, and a
    two-component Normal mixture likelihood whose component means are free, and a TruncatedNormal
    likelihood (exmc_erf)."""
    rng = np.random.default_rng(seed)
    ir = cg.IR()
    ir.rv("k", "gamma", dict(alpha=2.0, beta=1.0), transform="log")
    ir.rv("lam", "lognormal", dict(mu=0.5, sigma=0.8), transform="log")
    ir.rv("m", "normal", dict(mu=0.0, sigma=2.0))
    ir.rv("s", "half_normal", dict(sigma=1.5), transform="log")
    ir.rv("m1", "normal", dict(mu=-1.0, sigma=1.0))
    ir.rv("m2", "normal", dict(mu=2.0, sigma=1.0))
    ir.rv("t_rv", "weibull", {"k": "k", "lambda": "lam"})
    ir.obs("t_exact", "t_rv", rng.weibull(1.5, size=5) * 2.0 + 0.1)
    ir.obs("t_cens", "t_rv", [2.5, 3.0, 3.0], censored="right")
    ir.rv("x_rv", "normal", dict(mu="m", sigma="s"))
    ir.obs("x_left", "x_rv", [-0.5, 0.2], censored="left")
    ir.obs("x_right", "x_rv", 1.7, censored="right")
    ir.obs("x_int", "x_rv", dict(lower=[-1.0, 0.0], upper=[0.5, 2.0]), censored="interval")
    ir.obs("x_w", "x_rv", rng.normal(size=6), weight=[1.0, 0.5, 2.0, 1.0, 0.25, 3.0],
           mask=[True, True, False, True, True, False])
    ir.obs("x_mean", "x_rv", rng.normal(size=4) + 0.3, reduce="mean", weight=2.0)
    ir.obs("x_lse", "x_rv", [0.1, 0.9, -0.4], reduce="logsumexp")
    ir.rv("pos_rv", "lognormal", dict(mu="m", sigma=0.7), transform="log")
    ir.obs("pos", "pos_rv", [0.8, 1.9])
    ir.rv("mix_rv", "mixture", dict(components=["normal", "normal"],
                                    params=[dict(mu="m1", sigma=0.6), dict(mu="m2", sigma=1.1)],
                                    weights=[0.35, 0.65]))
    ir.obs("mix", "mix_rv", rng.normal(size=7) * 1.5 + 0.5)
    ir.rv("tn_rv", "truncated_normal", dict(mu="m", sigma="s", lower=-2.0, upper=3.0))
    ir.obs("tn", "tn_rv", [-1.2, 0.4, 2.6])
    return ir


SURVIVAL_INIT = dict(k=1.2, lam=1.5, m=0.1, s=1.0, m1=-0.8, m2=1.7)


# ---- the three larger BASELINE configs as Builder IR (exmc_amd/codegen.py sv_ir / radon_ir /
# logistic_ir) next to their hand-written kinds: same variable names, so an init map or a point of
# one is a point of the other after a permutation ----
def sv_returns(seed=3):
    return np.random.default_rng(seed).normal(size=100) * 0.02


def baseline_pair(which):
    """(ir, ncp, hand-written ModelSpec, lanes of the generated layout)"""
    from exmc_amd import models
    if which == "sv":
        r = sv_returns()
        return cg.sv_ir(r), False, models.sv(r), 64
    if which == "logistic":
        X, y = models.logistic_data()
        return cg.logistic_ir(X, y), True, models.logistic(X, y), 16
    if which == "radon":
        spec = models.radon()
        J = 85
        d = spec.data
        start = d[J:2 * J + 1].astype(int)
        n = start[-1]
        names = [v for v in spec.var_names if v.startswith("alpha_raw")]
        ir = cg.radon_ir(d[:J], start, d[2 * J + 1:2 * J + 1 + n], d[2 * J + 1 + n:], names=names)
        return ir, False, spec, 64
    raise ValueError(which)


def to_spec_order(gen, spec):
    """idx with q_generated = q_handwritten[idx] (the generated kernel order is the flat order)."""
    return [spec.var_names.index(n) for n in gen.var_names]


# ---- the models of the rewrite-pass tests (tests/test_codegen_rewrite.py) ----
POISSON_DATA = [2.0, 4.0, 3.0, 1.0, 5.0, 3.0, 2.0, 4.0, 3.0, 3.0]


def poisson_ir():
    """test/new_dist_test.exs:270-290: mu ~ Exponential(0.1), y ~ Poisson(mu), written without transforms"""
    ir = cg.IR()
    ir.rv("mu", "exponential", {"lambda": 0.1})
    ir.rv("y", "poisson", dict(mu="mu"))
    ir.obs("y_obs", "y", POISSON_DATA)
    return ir


LIFT_A = [[2.0, 0.5], [0.0, 1.5]]
LIFT_W = [1.0, 0.25, 3.0]


def _lift_base():
    ir = cg.IR()
    ir.rv("m", "normal", dict(mu=0.0, sigma=2.0))
    ir.rv("x", "normal", dict(mu=1.0, sigma=0.5))
    ir.rv("lik_rv", "normal", dict(mu="m", sigma=1.0))
    ir.obs("lik", "lik_rv", [0.3, -0.2])
    ir.rv("v", "normal", dict(mu=0.0, sigma=1.5))
    return ir


def lifted_ir(**opts):
    """obs of det("affine") and det("matmul") nodes: what the lifting passes turn into meas_obs"""
    ir = _lift_base()
    ir.det("ax", "affine", [2.0, -1.0, "x"])
    ir.obs("ax_obs", "ax", [0.5, 1.5, 2.5], weight=LIFT_W, **opts)
    ir.det("mv", "matmul", [LIFT_A, "v"])
    ir.obs("mv_obs", "mv", [0.7, -0.4])
    return ir


def lifted_direct_ir():
    """lifted_ir as the passes leave it, spelled with meas_obs"""
    ir = _lift_base()
    ir.meas_obs("ax_obs", "x", [0.5, 1.5, 2.5], ("affine", 2.0, -1.0), meta=dict(weight=np.asarray(LIFT_W), reduce="sum"))
    ir.meas_obs("mv_obs", "v", [0.7, -0.4], ("matmul", LIFT_A))
    return ir


def meas_transformed_ir(value=(3.0, 5.0)):
    """a meas_obs of a :log-transformed target next to an obs with likelihood: false"""
    ir = cg.IR()
    ir.rv("m", "normal", dict(mu=0.0, sigma=1.0))
    ir.rv("lik_rv", "normal", dict(mu="m", sigma=1.0))
    ir.obs("lik", "lik_rv", 0.2)
    ir.rv("r", "gamma", dict(alpha=2.0, beta=1.5), transform="log")
    ir.meas_obs("r_obs", "r", list(value) if isinstance(value, tuple) else value, ("affine", 2.0, 1.0))
    ir.rv("off_rv", "normal", dict(mu="m", sigma=0.1))
    ir.obs("off", "off_rv", [9.0, 9.0], likelihood=False)
    return ir


def weibull_ir(k_transform=None, **opts):
    """k ~ Gamma, t ~ Weibull(k, 2) observed, the obs options left to the caller"""
    ir = cg.IR()
    ir.rv("k", "gamma", dict(alpha=2.0, beta=1.0), transform=k_transform)
    ir.rv("t_rv", "weibull", {"k": "k", "lambda": 2.0})
    ir.obs("t", "t_rv", [1.0, 2.5], **opts)
    return ir


def dirichlet_obs_ir(transform=None, value=(0.2, 0.5, 0.3), **opts):
    """an observed Dirichlet (its default transform is :stick_breaking) next to a one-dimensional model"""
    ir = cg.IR()
    ir.rv("a", "gamma", dict(alpha=2.0, beta=1.0))
    ir.rv("th", "dirichlet", dict(alpha=[2.0, 3.0, 1.5]), transform=transform)
    ir.obs("th_obs", "th", list(value) if isinstance(value, tuple) else value, **opts)
    ir.rv("y_rv", "normal", dict(mu="a", sigma=1.0))
    ir.obs("y", "y_rv", 1.0)
    return ir


def data_ir(y):
    """Builder.data + a Custom distribution whose params name "__obs_data": sum_i N(y_i | x, sigma) up
    to its constant"""
    def logpdf(o, x, p):
        terms = []
        for yi in p["y"]:
            z = o.div(o.sub(yi, x), p["sigma"])
            terms.append(o.mul(o.lit(-0.5), o.mul(z, z)))
        return o.sub(o.sum(terms), o.mul(o.lit(float(len(p["y"]))), o.log(p["sigma"])))
    ir = cg.IR().data(y)
    ir.rv("sigma", "half_cauchy", dict(scale=2.0), transform="log")
    ir.rv("m", "custom", dict(logpdf=logpdf, y="__obs_data", sigma="sigma"))
    return ir


def data_missing_ir():
    ir = cg.IR()
    ir.rv("m", "custom", dict(logpdf=lambda o, x, p: x, y="__obs_data"))
    return ir


def data_matrix_ir():
    ir = cg.IR().data([[1.0, 2.0], [3.0, 4.0]])
    ir.rv("m", "custom", dict(logpdf=lambda o, x, p: o.mul(o.neg(o.mul(x, x)), p["a"][1][0]), a="__obs_data"))
    return ir


def data_scalar_ir():
    ir = cg.IR().data(1.5)
    ir.rv("m", "custom", dict(logpdf=lambda o, x, p: o.mul(o.neg(o.mul(x, x)), p["a"]), a="__obs_data"))
    return ir


# ---- the models of the refusal tests (test_codegen_obs_meta.py, test_codegen_round2.py, test_codegen_simplex.py) ----
def right_censored_normal_ir():
    ir = cg.IR()
    ir.rv("mu", "normal", dict(mu=0.0, sigma=10.0))
    ir.rv("x_rv", "normal", dict(mu="mu", sigma=2.0))
    ir.obs("x", "x_rv", 1.0, censored="right")
    return ir


def censored_gamma_ir():
    ir = cg.IR()
    ir.rv("a", "gamma", dict(alpha=2.0, beta=1.0), transform="log")
    ir.rv("x_rv", "gamma", dict(alpha="a", beta=1.0))
    ir.obs("x", "x_rv", 1.0, censored="right")                 # censored.ex has no Gamma clause
    return ir


def walk_only_ir(steps, transform=None):
    return cg.IR().rv("x", "gaussian_random_walk", dict(sigma=1.0, steps=steps), transform=transform)


def meas_ref_param_ir():
    ir = cg.IR()
    ir.rv("a", "normal", dict(mu=0.0, sigma=1.0))
    ir.rv("k_rv", "normal", dict(mu="a", sigma=1.0))
    ir.meas_obs("k", "k_rv", 1.0, ("affine", 2.0, 0.0))                  # eager term with a ref param
    return ir


def free_dirichlet_ir(alpha=(1.0, 1.0, 1.0), transform=None):
    return cg.IR().rv("th", "dirichlet", dict(alpha=list(alpha)), transform=transform)


# ---- one small model per branch of the generator that no larger model reaches: the corpus of
# tools/gen_digests.py pins each one's text, or the message of its refusal ----
def _mx(ir=None):
    """m ~ N(0, 2), s ~ HalfNormal(1.5) [:log], x_rv ~ N(m, s) to be observed"""
    ir = cg.IR() if ir is None else ir
    ir.rv("m", "normal", dict(mu=0.0, sigma=2.0))
    ir.rv("s", "half_normal", dict(sigma=1.5), transform="log")
    ir.rv("x_rv", "normal", dict(mu="m", sigma="s"))
    return ir


def obs_ir(value, target="x_rv", **opts):
    """_mx with one obs node of the caller's"""
    return _mx().obs("o", target, value, **opts)


def target_ir(dist, params, transform, value, **opts):
    """m, s and an observed target of the caller's (its params may name m and s)"""
    ir = _mx()
    ir.rv("t_rv", dist, params, transform=transform)
    return ir.obs("o", "t_rv", value, **opts)


def meas_ir(value, info, dist="normal", params=None, transform=None, meta=None):
    ir = _mx().obs("o", "x_rv", 0.4)
    ir.rv("k_rv", dist, dict(mu=1.0, sigma=2.0) if params is None else params, transform=transform)
    return ir.meas_obs("k", "k_rv", value, info, meta=meta)


def free_ir(dist, params, transform=None):
    """_mx, x_rv observed, and one more free rv of the caller's"""
    ir = _mx().obs("o", "x_rv", 0.4)
    return ir.rv("f", dist, params, transform=transform)


def _square(o, x, p):
    return o.mul(o.lit(-0.5), o.mul(x, x))


def literal_custom_ir(observed=False):
    """a Custom rv over literals alone: no datum is read, nothing to fold"""
    ir = cg.IR()
    if not observed:
        return ir.rv("x", "custom", dict(logpdf=_square))
    ir.rv("m", "normal", dict(mu=0.0, sigma=1.0))
    ir.rv("z_rv", "custom", dict(logpdf=lambda o, x, p: o.neg(o.mul(p["m"], p["m"])), m="m"))
    return ir.obs("z", "z_rv", 0.0)


def linear_custom_ir():
    """log-density x * datum: the gradient is the datum itself, an output that is a folded constant"""
    return cg.IR().rv("x", "custom", dict(logpdf=lambda o, x, p: o.mul(x, o.data(2.0))))


def default_transforms_ir():
    """a mixture and two Custom rvs, written without transforms (mixture.ex:34-36, custom.ex:92-95)"""
    ir = cg.IR()
    ir.rv("mix", "mixture", dict(components=["exponential", "exponential"], params=[{"lambda": 1.0}, {"lambda": 3.0}],
                                 weights=[0.5, 0.5]))
    ir.rv("c", "custom", dict(logpdf=_square))
    return ir


def custom_transform_field_ir():
    """a Custom bundle with a transform field: the passes attach it; the field then reaches the closure's
    params, where a string is a reference"""
    return cg.IR().rv("c", "custom", dict(logpdf=_square, transform="log"))


def cyclic_ir():
    ir = cg.IR()
    ir.rv("s", "half_normal", dict(sigma=1.0), transform="log")
    ir.rv("a", "normal", dict(mu="b", sigma="s"))
    ir.rv("b", "normal", dict(mu="a", sigma="s"))
    ir.rv("y_rv", "normal", dict(mu="a", sigma=1.0))
    return ir.obs("y", "y_rv", 0.4)


def ref_to_observed_ir():
    ir = _mx().obs("o", "x_rv", 0.4)
    return ir.rv("f", "normal", dict(mu="x_rv", sigma=1.0))


def unknown_target_ir():
    return _mx().obs("o", "nowhere", 0.4)


def all_observed_ir():
    ir = cg.IR().rv("x", "normal", dict(mu=0.0, sigma=1.0))
    return ir.obs("o", "x", 0.3)


def constant_density_ir():
    return cg.IR().rv("u", "uniform01", {})


def bad_term_order_ir(how):
    ir = obs_ir(0.4)
    ids = sorted(ir.nodes)
    if how == "keys":                             # (IR.order refuses this itself: as a document may carry it)
        ir.term_order = ids[:-1]
        return ir
    return ir.order(list(reversed(ids)))


def corner_cases():
    """[(name, ir thunk, generate's keywords)]"""
    T = lambda fn, *a, **k: (lambda: fn(*a, **k))   # noqa: E731
    rw, pw = dict(rewrite_passes=True), dict(pointwise=True)
    vec3 = [0.3, 1.2, 0.7]
    unit3 = [0.2, 0.5, 0.9]
    mvn = dict(mu=[0.1, -0.2], cov=[[1.0, 0.3], [0.3, 2.0]])
    return [
        # rewrite passes
        ("rewrite/poisson", poisson_ir, rw), ("rewrite/lifted", lifted_ir, rw),
        ("rewrite/lifted_censored", T(lifted_ir, censored="right"), rw),
        ("rewrite/weibull_censored", T(weibull_ir, censored="right"), rw),
        ("rewrite/weibull", weibull_ir, rw), ("rewrite/dirichlet_obs", dirichlet_obs_ir, rw),
        ("rewrite/default_transforms", default_transforms_ir, rw),
        ("rewrite/custom_transform_field", custom_transform_field_ir, rw),
        ("rewrite/simple", cg.simple_ir, rw),
        # "__obs_data"
        ("data/vector", T(data_ir, [0.3, -1.2, 2.2, 0.9]), {}), ("data/matrix", data_matrix_ir, {}),
        ("data/scalar", data_scalar_ir, {}), ("data/missing", data_missing_ir, {}),
        # observation of a transformed target
        ("obs_tr/log", T(target_ir, "lognormal", dict(mu="m", sigma=0.7), "log", 0.8), {}),
        ("obs_tr/log/vector", T(target_ir, "lognormal", dict(mu="m", sigma=0.7), "log", vec3), {}),
        ("obs_tr/softplus", T(target_ir, "half_normal", dict(sigma="s"), "softplus", 0.8), {}),
        ("obs_tr/softplus/vector", T(target_ir, "half_normal", dict(sigma="s"), "softplus", vec3), {}),
        ("obs_tr/logit", T(target_ir, "beta", dict(alpha="s", beta=2.0), "logit", 0.3), {}),
        ("obs_tr/logit/vector", T(target_ir, "beta", dict(alpha="s", beta=2.0), "logit", unit3), {}),
        ("obs_tr/vector_param", T(target_ir, "lognormal", dict(mu="m", sigma=[0.7, 0.9]), "log", 0.8, reduce="sum"), {}),
        ("obs_tr/uncovered", T(target_ir, "normal", dict(mu="m", sigma="s"), "cube", 0.8), {}),
        ("obs_tr/interval", T(target_ir, "normal", dict(mu="m", sigma="s"), "log", dict(lower=0.5, upper=1.5),
                              censored="interval"), {}),
        ("obs_tr/custom", T(target_ir, "custom", dict(logpdf=_square), "log", 0.8), {}),
        # observation metadata
        ("meta/scalar_weight", T(obs_ir, 0.4, weight=2.5), {}),
        ("meta/vector_weight_on_scalar_term", T(target_ir, "mv_normal", mvn, None, [0.3, 0.4], weight=[1.0, 2.0]), {}),
        ("meta/scalar_mask_true", T(obs_ir, 0.4, mask=True), {}), ("meta/scalar_mask_false", T(obs_ir, 0.4, mask=False), {}),
        ("meta/scalar_mask_true/pointwise", T(obs_ir, 0.4, mask=True), pw),
        ("meta/vector_mask_on_scalar_term", T(target_ir, "mv_normal", mvn, None, [0.3, 0.4], mask=[True, False]), {}),
        ("meta/mask_length", T(target_ir, "normal", dict(mu="m", sigma=[1.0, 2.0]), None, 0.4, mask=True, reduce="sum"), {}),
        ("meta/no_reduce", T(target_ir, "normal", dict(mu="m", sigma=[1.0, 2.0]), None, 0.4), {}),
        ("meta/likelihood_false", meas_transformed_ir, {}),
        # meas_obs
        ("meas/affine/vector_a", T(meas_ir, [3.0, 5.0], ("affine", [2.0, -4.0], 1.0)), {}),
        ("meas/affine/vector_b", T(meas_ir, [3.0, 5.0], ("affine", 2.0, [1.0, 0.5])), {}),
        ("meas/matmul", T(meas_ir, [0.5, -0.25], ("matmul", [[2.0, 1.0], [0.0, 3.0]])), {}),
        ("meas/transformed/scalar", T(meas_transformed_ir, 3.0), {}),
        ("meas/transformed/logit", T(meas_ir, [1.5, 1.8], ("affine", 2.0, 1.0), "beta", dict(alpha=2.0, beta=3.0), "logit"), {}),
        ("meas/transformed/softplus", T(meas_ir, 3.0, ("affine", 2.0, 1.0), "half_normal", dict(sigma=1.0), "softplus"), {}),
        ("meas/weighted", T(meas_ir, [3.0, 5.0], ("affine", 2.0, 1.0), meta=dict(weight=np.asarray([1.0, 0.5]), reduce="mean")), {}),
        ("meas/vector_target", T(meas_ir, [0.3, 0.4], ("affine", 2.0, 1.0), "mv_normal", mvn), {}),
        ("meas/ref_param", meas_ref_param_ir, {}),
        # obs
        ("obs/det_target", lifted_ir, {}),
        ("obs/censored/scalar", T(lambda: _mx().obs("a", "x_rv", -0.5, censored="left").obs("b", "x_rv", 1.7, censored="right")
                                  .obs("c", "x_rv", dict(lower=-1.0, upper=0.5), censored="interval")), {}),
        ("obs/censored/vector", T(lambda: _mx().obs("a", "x_rv", [-0.5, 0.2], censored="left")
                                  .obs("b", "x_rv", [1.7, 0.1], censored="right")
                                  .obs("c", "x_rv", dict(lower=[-1.0, 0.0], upper=[0.5, 2.0]), censored="interval")), {}),
        ("obs/censored/right_normal", right_censored_normal_ir, {}), ("obs/censored/gamma", censored_gamma_ir, {}),
        ("obs/censored/weibull", T(weibull_ir, "log", censored="right"), {}),
        ("obs/censored/vector_param", T(target_ir, "normal", dict(mu="m", sigma=[1.0, 2.0]), None, [0.3, 0.4],
                                        censored="left"), {}),
        ("obs/vector_dist/plain", T(dirichlet_obs_ir), {}),
        ("obs/vector_dist/transform", T(dirichlet_obs_ir, "log"), {}),
        ("obs/vector_dist/scalar_value", T(dirichlet_obs_ir, None, 0.5), {}),
        ("obs/vector_dist/censored", T(dirichlet_obs_ir, None, (0.2, 0.5, 0.3), censored="left"), {}),
        ("obs/vector_dist/mv_normal", T(target_ir, "mv_normal", mvn, None, [0.3, 0.4]), {}),
        ("obs/mixture_vector", T(target_ir, "mixture", dict(components=["normal", "normal"],
                                                            params=[dict(mu="m", sigma=0.6), dict(mu=2.0, sigma="s")],
                                                            weights=[0.35, 0.65]), None, vec3), {}),
        ("obs/mixture_scalar", T(target_ir, "mixture", dict(components=["normal", "laplace"],
                                                            params=[dict(mu="m", sigma=0.6), dict(mu=2.0, b="s")],
                                                            weights=[0.35, 0.65]), None, 0.7), {}),
        ("obs/vector_lengths", T(target_ir, "normal", dict(mu="m", sigma=[1.0, 2.0]), None, vec3), {}),
        # free rvs
        ("free/custom", literal_custom_ir, {}), ("free/custom/linear", linear_custom_ir, {}),
        ("free/custom/not_callable", T(free_ir, "custom", dict(logpdf="normal")), {}),
        ("free/custom/list", T(free_ir, "custom", dict(logpdf=lambda o, x, p: [x, x])), {}),
        ("free/vector_param", T(free_ir, "normal", dict(mu=[0.0, 1.0], sigma=1.0)), {}),
        ("free/transformed_vector", T(walk_only_ir, 3, "log"), {}),
        ("free/dirichlet/no_transform", free_dirichlet_ir, {}),
        ("free/dirichlet/short", T(free_dirichlet_ir, (1.0,), "stick_breaking"), {}),
        ("free/dirichlet", T(free_dirichlet_ir, (1.0, 1.0, 1.0), "stick_breaking"), {}),
        ("free/matrix_param", T(free_ir, "normal", dict(mu=[[0.0, 1.0]], sigma=1.0)), {}),
        # the whole model
        ("model/unknown_target", unknown_target_ir, {}), ("model/all_observed", all_observed_ir, {}),
        ("model/too_many_dimensions", T(walk_only_ir, 257), {}), ("model/lanes=8", T(obs_ir, 0.4), dict(lanes=8)),
        ("model/d=25/lanes=auto", T(walk_only_ir, 25), {}), ("model/d=40/lanes=auto", T(walk_only_ir, 40), {}),
        ("model/term_order/keys", T(bad_term_order_ir, "keys"), {}),
        ("model/term_order/unsorted", T(bad_term_order_ir, "unsorted"), {}),
        ("model/constant_density", constant_density_ir, {}), ("model/ref_to_observed", ref_to_observed_ir, {}),
        ("model/cyclic_ncp", cyclic_ir, {}), ("model/cyclic_ncp/ncp=0", cyclic_ir, dict(ncp=False)),
    ]
