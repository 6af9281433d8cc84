"""A plain-Python statement of Exmc.ADVI (lib/exmc/advi.ex), written from its text and citing its
lines. TEST INFRASTRUCTURE: the product never imports it.

The statement is parametrised by
  evaluate(z) -> (logp, g)      the model's value and gradient (Compiler.value_and_grad)
  vsum(v) -> float              the sum over a fit's dimensions (Nx.sum's reduction)
  exp(x) -> float               Nx.exp
  normal() -> float             :rand.normal_s of ONE generator seeded with the fit's seed: the loop and
                                the draws walk the same generator (advi.ex:34-37)
and comes in two modes:
  lane mode       the device's arithmetic: the checker's model in the lane layout (oracle Cfg(1, G)),
                  exo_rng_normal, exo_det_exp, and group_sum_slots as pathfinder_statement restates it
  reference mode  the reference's arithmetic as far as Python has it: Cfg(0, 1), math.exp,
                  left-to-right sums
Products and sums round separately, as Nx's element-wise ops do.

Stated deviations from advi.ex (DESIGN.md "ADVI"): max_iters, num_draws, num_mc_samples >= 1 and
window_size >= 2 (below them the reference's behaviour is an accident of 1..0 and a division by zero);
results are in the unconstrained kernel space in kernel order; where sum(log_sigma) is not finite the
reference raises (:126 adds a float to an atom), here the value flows on: a finite logp gives a
non-finite ELBO, which never passes the convergence test."""
import math

import numpy as np

import oracle as O
from pathfinder_statement import Result, _rank_of, lane_sum, rng_factory, seq_sum

MU0 = 0.0             # advi.ex:31
LOG_SIGMA0 = -1.0     # :32
ELBO_NON_FINITE = -1.0e10   # :128
REL_EPS = 1.0e-8      # :83


def entropy_const(d):
    """0.5 * d * (1.0 + :math.log(2.0 * :math.pi())) (:126), libm on the host."""
    return 0.5 * d * (1.0 + math.log(2.0 * math.pi))


def window_converged(elbos_newest_first, window, tol):
    """advi.ex:77-86 on the history, newest first. Enum.sum is 0 + x1 + x2 + ..., left to right."""
    if len(elbos_newest_first) < window:
        return False
    h = window // 2
    recent = elbos_newest_first[:h]           # Enum.take(elbos, div(window, 2))
    old = elbos_newest_first[h:2 * h]         # drop, then take
    mean_recent = seq_sum(recent) / h
    mean_old = seq_sum(old) / h
    # equal means (both -1.0e10 in the non-finite branch) give 0.0 < tol; a NaN mean (a stated deviation:
    # the reference raises where sum(log_sigma) is not a number) compares false
    return abs(mean_recent - mean_old) / (abs(mean_old) + REL_EPS) < tol


def _exp_vec(exp, v):
    return np.array([exp(float(x)) for x in v])


def _exp_guard(exp):
    def f(x):
        try:
            return exp(x)
        except OverflowError:
            return math.inf
    return f


def fit(evaluate, d, normal, vsum=seq_sum, exp=math.exp, num_draws=1000, max_iters=10000, learning_rate=0.01,
        num_mc_samples=1, convergence_tol=1.0e-4, window_size=100, rank=None):
    """ADVI.fit/2 (:21-50). rank[i] = position of kernel dimension i in the flat vector (None:
    identity). Returns mu, log_sigma [d], elbo_history (length num_iters), num_iters, converged, draws
    [num_draws][d] (kernel order, unconstrained), and non_finite: the number of samples that took the
    -1.0e10 branch."""
    assert max_iters >= 1 and num_draws >= 1 and num_mc_samples >= 1 and window_size >= 2
    rank = list(range(d)) if rank is None else [int(r) for r in rank]
    perm = [0] * d                       # perm[r] = kernel dimension of flat entry r
    for i, r in enumerate(rank):
        perm[r] = i
    exp = _exp_guard(exp)
    lr, n = float(learning_rate), int(num_mc_samples)
    cst = entropy_const(d)

    mu = np.full(d, MU0)                 # :31
    log_sigma = np.full(d, LOG_SIGMA0)   # :32
    elbos = []                           # newest first (:75)
    num_iters, converged, non_finite = 0, False, 0

    with np.errstate(all="ignore"):
        for i in range(1, max_iters + 1):            # :62
            sigma = _exp_vec(exp, log_sigma)         # :63
            eps_list = []                            # :105-115: all samples' variates first
            for _ in range(n):
                eps = np.zeros(d)
                for r in range(d):
                    eps[perm[r]] = normal()
                eps_list.append(eps)
            elbo_sum, gm, gl = 0.0, None, None
            for eps in eps_list:                     # :121-139
                z = mu + sigma * eps
                logp, g = evaluate(z)
                logp, g = float(logp), np.array(g, dtype=np.float64)
                entropy = vsum([float(x) for x in log_sigma]) + cst          # :126
                elbo_s = logp + entropy if math.isfinite(logp) else ELBO_NON_FINITE   # :128
                non_finite += 0 if math.isfinite(logp) else 1
                gls = (g * sigma) * eps + 1.0        # :132-136
                elbo_sum = elbo_sum + elbo_s         # :141
                gm = g if gm is None else gm + g     # :143-147, Enum.reduce: the first is the start
                gl = gls if gl is None else gl + gls
            elbo = elbo_sum / n
            gm = gm / (n * 1.0)
            gl = gl / (n * 1.0)
            mu = mu + lr * gm                        # :70
            log_sigma = log_sigma + lr * gl          # :72-73
            elbos.insert(0, elbo)                    # :75
            num_iters = i
            converged = window_converged(elbos, window_size, convergence_tol)   # :77-86
            if converged:                            # :98
                break

        # :158-173, from the generator as the loop left it
        sigma = _exp_vec(exp, log_sigma)
        draws = np.zeros((num_draws, d))
        for s in range(num_draws):
            for r in range(d):
                v = normal()
                draws[s, perm[r]] = mu[perm[r]] + sigma[perm[r]] * v
    return Result(mu=mu, log_sigma=log_sigma, elbo_history=list(reversed(elbos)), num_iters=num_iters,
                  converged=converged, draws=draws, non_finite=non_finite)


# ---- the two modes over the checker's models ------------------------------------------------------
def fit_lane(model, lanes, seed, **kw):
    """The device's statement: `model` an oracle Model (gen_checker.model for a generated one)."""
    cfg = O.Cfg(1, lanes)
    return fit(lambda q: model.logp_grad(q, cfg), model.d, rng_factory(seed, 1)(), vsum=lane_sum(lanes, model.d),
               exp=O.lib().exo_det_exp, rank=_rank_of(model), **kw)


def fit_reference(model, seed, **kw):
    cfg = O.Cfg(0, 1)
    return fit(lambda q: model.logp_grad(q, cfg), model.d, rng_factory(seed, 0)(), vsum=seq_sum, exp=math.exp,
               rank=_rank_of(model), **kw)
