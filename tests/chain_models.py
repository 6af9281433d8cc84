"""Random-walk test models for the generator's scan chains (exmc_amd/codegen_lanes.py), shared by
the CPU and GPU tests: chains of Normals whose mu is the previous step and whose sigma is a shared
scale, which the non-centred rewrite turns into s_k = s_{k-1} + sigma z_k."""
import numpy as np

from exmc_amd import codegen as cg


def chain_ir(lengths, seed=0, head="centred", branch=None, sigma_split=None):
    """One walk per entry of `lengths` (the number of increments), named w<j>_1 .. w<j>_<m+1> so that
    the flat order (the string sort) is not the walk's order; each walk's values are observed through
    one Custom closure of Normal terms (the shape of sv's likelihood).

    head: "centred" (w_1 ~ Normal(0.0, 1.0): a plain position entry), "log" (w_1 ~ Exponential(1.0),
    :log -- a transformed value) or "ncp" (w_1 ~ Normal(m0, tau), itself non-centred with another
    scale). branch = k: a second walk of 5 steps starts at step k of walk 0 (step k is the mu of two
    non-centred nodes). sigma_split = k: walk 0 switches to a second scale after step k."""
    rng = np.random.default_rng(seed)
    ir = cg.IR()
    obs = {}
    for j, m in enumerate(lengths):
        p = "w%d_" % j
        ir.rv("sig%d" % j, "exponential", {"lambda": 4.0}, transform="log")
        if head == "centred":
            ir.rv(p + "1", "normal", dict(mu=0.0, sigma=1.0))
        elif head == "log":
            ir.rv(p + "1", "exponential", {"lambda": 1.0}, transform="log")
        elif head == "ncp":
            ir.rv("m%d" % j, "normal", dict(mu=0.0, sigma=2.0))
            ir.rv("tau%d" % j, "exponential", {"lambda": 2.0}, transform="log")
            ir.rv(p + "1", "normal", dict(mu="m%d" % j, sigma="tau%d" % j))
        else:
            raise ValueError(head)
        if sigma_split is not None and j == 0:
            ir.rv("sigb0", "exponential", {"lambda": 4.0}, transform="log")
        for k in range(2, m + 2):
            sig = "sigb0" if (sigma_split is not None and j == 0 and k > sigma_split) else "sig%d" % j
            ir.rv(p + "%d" % k, "normal", dict(mu=p + "%d" % (k - 1), sigma=sig))
        obs.update({p + "%d" % k: float(v) for k, v in zip(range(1, m + 2), np.cumsum(rng.normal(size=m + 1) * 0.3))})
    if branch is not None:
        ir.rv("b_1", "normal", dict(mu="w0_%d" % branch, sigma="sig0"))
        for k in range(2, 6):
            ir.rv("b_%d" % k, "normal", dict(mu="b_%d" % (k - 1), sigma="sig0"))
        obs.update({"b_%d" % k: float(rng.normal()) for k in range(1, 6)})
    names = sorted(obs)

    def lik(o, _x, p):
        return o.sum([o.logpdf("normal", o.data(obs[n]), dict(mu=p[n], sigma=o.lit(0.5))) for n in names])
    params = {n: n for n in names}
    params["logpdf"] = lik
    ir.rv("lik", "custom", params)
    ir.obs("lik_obs", "lik", 0.0)
    return ir
