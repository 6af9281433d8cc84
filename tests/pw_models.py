"""Models and numpy statements for the per-datum terms of generated models (exmc_amd/codegen.py
generate(pointwise=True)), shared by tests/test_codegen_pointwise.py and its GPU sibling. The numpy
statements share no code with the generator: each restates a distribution module of the reference with
its f32 literals (an untyped Nx.tensor(<float>) is f32)."""
import math

import numpy as np

from exmc_amd import codegen as cg


def f32(x):
    return float(np.float32(x))


LOG_2PI = f32(math.log(f32(2.0 * math.pi)))      # Nx.log(Nx.tensor(2 pi)), normal.ex
TINY = f32(1.0e-30)
LANCZOS = [f32(c) for c in (0.99999999999980993, 676.5203681218851, -1259.1392167224028, 771.32342877765313,
                            -176.61502916214059, 12.507343278686905, -0.13857109526572012,
                            9.9843695780195716e-6, 1.5056327351493116e-7)]      # math.ex:10-20
HALF_LOG_2PI = f32(0.5 * math.log(2.0 * math.pi))
PI32 = f32(math.pi)


def clamp200(z):
    return np.maximum(-200.0, np.minimum(z, 200.0))


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def normal_logpdf(x, mu, sigma):
    """normal.ex:15-24"""
    ss = np.maximum(sigma, TINY)
    z = (x - mu) / ss
    return -0.5 * (z * z + (LOG_2PI + 2.0 * np.log(ss)))


def lgamma(x):
    """math.ex:27-52: Lanczos, g = 7, f32 coefficients"""
    t = x + 6.5
    ag = LANCZOS[0]
    for i, c in enumerate(LANCZOS[1:]):
        ag = ag + c / (x + float(i))
    return ((HALF_LOG_2PI + (x - 0.5) * np.log(t)) - t) + np.log(ag)


def bernoulli_logpdf(x, p):
    """bernoulli.ex:17-27: p clipped to [1e-7, 1 - 1e-7] in f32"""
    lo, hi = f32(1.0e-7), float(np.float32(1.0) - np.float32(1.0e-7))
    pc = np.minimum(np.maximum(p, lo), hi)
    return x * np.log(pc) + (1.0 - x) * np.log(1.0 - pc)


def poisson_logpdf(x, mu):
    """poisson.ex:16-20"""
    return (x * np.log(mu) - mu) - lgamma(x + 1.0)


def student_t_logpdf(x, df, loc, scale):
    """student_t.ex:15-29"""
    ss, sdf = np.maximum(scale, TINY), np.maximum(df, TINY)
    z = (x - loc) / ss
    hp1, h = (sdf + 1.0) / 2.0, sdf / 2.0
    r = lgamma(hp1) - lgamma(h)
    r = r - 0.5 * np.log(sdf * PI32)
    r = r - np.log(ss)
    return r - hp1 * np.log(1.0 + (z * z) / sdf)


# ---- models -------------------------------------------------------------------------------------
def ref_ir(prior_mu, prior_sigma, obs):
    """integration_test.exs 17-19: mu ~ N(prior), x ~ N(mu, 1) observed, one obs node per value"""
    ir = cg.IR()
    ir.rv("mu", "normal", dict(mu=prior_mu, sigma=prior_sigma))
    for name, value in obs:
        ir.rv(name, "normal", dict(mu="mu", sigma=1.0))
        ir.obs(name + "_obs", name, value)
    return ir


LONG_Y = np.round(np.random.default_rng(23).normal(size=37) * 1.5 + 0.7, 3)   # 37 = 2 groups of 16 and 5


def long_ir():
    """the README model with a vector obs longer than one generated function, no multiple of it"""
    return cg.simple_ir(LONG_Y)


COUNTS = dict(cnt=np.array([0.0, 3.0, 1.0, 2.0, 7.0]), b=np.array([1.0, 0.0, 0.0, 1.0]),
              t=np.array([0.3, -1.9, 4.5]))


def counts_ir():
    """Bernoulli, Poisson and StudentT observations (d = 4: df, p, rate, scale in flat order)"""
    ir = cg.IR()
    ir.rv("rate", "gamma", dict(alpha=3.0, beta=2.0), transform="log")
    ir.rv("p", "beta", dict(alpha=2.0, beta=5.0), transform="logit")
    ir.rv("df", "exponential", {"lambda": 0.2}, transform="log")
    ir.rv("scale", "half_normal", dict(sigma=2.0), transform="softplus")
    ir.rv("cnt_rv", "poisson", dict(mu="rate"))
    ir.obs("cnt", "cnt_rv", COUNTS["cnt"])
    ir.rv("b_rv", "bernoulli", dict(p="p"))
    ir.obs("b", "b_rv", COUNTS["b"])
    ir.rv("t_rv", "student_t", dict(df="df", loc=0.25, scale="scale"))
    ir.obs("t", "t_rv", COUNTS["t"])
    return ir


def counts_numpy(q):
    """[..., 12] in datum order b, cnt, t (ids sorted); q = (df, p, rate, scale) unconstrained"""
    df, rate = np.exp(clamp200(q[..., 0:1])), np.exp(clamp200(q[..., 2:3]))
    p = np.exp(-softplus(-q[..., 1:2]))
    scale = softplus(q[..., 3:4])
    return np.concatenate([bernoulli_logpdf(COUNTS["b"], p), poisson_logpdf(COUNTS["cnt"], rate),
                           student_t_logpdf(COUNTS["t"], df, 0.25, scale)], axis=-1)


def walk_y(steps):
    return np.round(np.random.default_rng(100 + steps).normal(size=steps) * 0.4, 3)


def walk_ir(steps):
    """noise, sigma (both :log) and a random walk of `steps` elements observed with noise: d = steps + 2.
    steps = 22 has the lane layout only (d = 24 > 20); steps = 6 is its one-lane sibling."""
    ir = cg.IR()
    ir.rv("noise", "half_normal", dict(sigma=1.0), transform="log")
    ir.rv("sigma", "exponential", {"lambda": 2.0}, transform="log")
    ir.rv("w", "gaussian_random_walk", dict(sigma="sigma", steps=steps))
    ir.rv("y_rv", "normal", dict(mu="w", sigma="noise"))
    ir.obs("y", "y_rv", walk_y(steps))
    return ir


def walk_numpy(q, steps):
    """y_i ~ N(w_i, noise): q = (noise, sigma, w_0 ...)"""
    return normal_logpdf(walk_y(steps), q[..., 2:], np.exp(clamp200(q[..., 0:1])))


def two_obs_ir(with_a=True):
    """one target observed by two vector obs nodes: dropping one leaves the free variables alone"""
    ir = cg.IR()
    ir.rv("mu", "normal", dict(mu=0.0, sigma=5.0))
    ir.rv("sigma", "exponential", {"lambda": 1.0}, transform="log")
    ir.rv("y", "normal", dict(mu="mu", sigma="sigma"))
    if with_a:
        ir.obs("y_a", "y", [0.3, -1.2, 2.2, 0.9, 1.4, -0.1, 0.7], weight=[1.0, 0.5, 2.0, 1.0, 0.25, 3.0, 1.5])
    ir.obs("y_b", "y", [1.1, 0.2, -0.4, 0.6, 1.9])
    return ir


def meta_ir():
    """every kind of obs node next to each other: what counts as a datum"""
    ir = cg.IR()
    ir.rv("m", "normal", dict(mu=0.0, sigma=2.0))
    ir.rv("s", "half_normal", dict(sigma=1.5), transform="log")
    ir.rv("x_rv", "normal", dict(mu="m", sigma="s"))
    ir.obs("a_w", "x_rv", [0.1, 0.2, 0.3], weight=[1.0, 0.5, 2.0])
    ir.obs("b_mask", "x_rv", [0.1, 0.2, 0.3, 0.4, 0.5], mask=[True, False, True, False, True], weight=2.0)
    ir.obs("c_mean", "x_rv", [0.5, 0.6], reduce="mean")
    ir.obs("d_lse", "x_rv", [0.5, 0.6, 0.7], reduce="logsumexp")
    ir.obs("e_off", "x_rv", [0.5, 0.6], likelihood=False)
    ir.rv("k_rv", "normal", dict(mu=1.0, sigma=2.0))
    ir.meas_obs("f_meas", "k_rv", 3.0, ("affine", 2.0, 1.0))
    ir.obs("g_left", "x_rv", [-0.5, 0.2], censored="left")
    ir.obs("h_right", "x_rv", 1.7, censored="right")
    ir.obs("i_int", "x_rv", dict(lower=[-1.0, 0.0], upper=[0.5, 2.0]), censored="interval")
    ir.obs("j_masked_scalar", "x_rv", 0.3, mask=False)

    def lik(o, x, p):
        return o.sum([o.logpdf("normal", xj, dict(mu=p["m"], sigma=o.lit(1.0))) for xj in x])
    ir.rv("z_rv", "custom", dict(logpdf=lik, m="m"))
    ir.obs("k_custom", "z_rv", [0.4, -1.1, 2.0])
    ir.rv("mv_rv", "mv_normal", dict(mu=[0.1, -0.2], cov=[[1.0, 0.3], [0.3, 2.0]]))
    ir.obs("l_mv", "mv_rv", [0.3, 0.4])
    return ir


def no_datum_ir():
    """the only obs node has likelihood: false"""
    ir = cg.IR()
    ir.rv("mu", "normal", dict(mu=0.0, sigma=1.0))
    ir.rv("x", "normal", dict(mu="mu", sigma=1.0))
    ir.obs("x_obs", "x", 0.5, likelihood=False)
    return ir
