"""A plain-Python statement of Exmc.Pathfinder (lib/exmc/pathfinder.ex), written from its text and
citing its lines. TEST INFRASTRUCTURE: the product never imports it.

The statement is parametrised by
  evaluate(q) -> (logp, g)      the model's value and gradient (Compiler.value_and_grad)
  vsum(v) -> float              the sum over a chain's dimensions (Nx.dot's and Nx.sum's reduction)
  log(x) -> float               Nx.log
  normal() -> float             :rand.normal_s of a generator seeded with the path's seed
and comes in two modes:
  lane mode       the device's arithmetic: the checker's model in the lane layout (oracle Cfg(1, G)),
                  exo_rng_normal, exo_det_log, and group_sum_slots restated below (left to right
                  for a 16-lane group with d <= 12, lane partials then the xor butterfly otherwise)
  reference mode  the reference's arithmetic as far as Python has it: Cfg(0, 1), math.log,
                  left-to-right sums
Products and sums round separately, as Nx's element-wise ops do.

Stated deviations from pathfinder.ex (DESIGN.md "Pathfinder"): a point whose ELBO is not finite is
never selected and a path without a finite ELBO has status 1 and NaN results (the reference raises);
a pair whose dot(y, s) is NaN is not pushed (the reference raises on it)."""
import ctypes as C
import math

import numpy as np

import oracle as O

ALPHA = 0.01          # pathfinder.ex:80
PUSH_MIN = 1.0e-10    # :93
GAMMA_MIN = 1.0e-10   # :140
GRAD_EPS = 1.0e-6     # :162


def entropy_const(d):
    """0.5 * d * (1.0 + :math.log(2.0 * :math.pi())) (:165), libm on the host."""
    return 0.5 * d * (1.0 + math.log(2.0 * math.pi))


def seq_sum(v):
    acc = 0.0
    for x in v:
        acc = acc + float(x)
    return acc


def lane_sum(G, d):
    """group_sum_slots<G, DPL, D>(v, valid, l, 0.0) of exmc_device.hpp: dimension i sits in slot i / G
    of lane i mod G."""
    if G == 16 and d <= 12:      # kSeqSum: 0.0 + v[0] + v[1] + ... in lane order
        return seq_sum

    def f(v):
        part = [0.0] * G
        for lane in range(G):
            acc = 0.0
            for i in range(lane, d, G):
                acc = acc + float(v[i])
            part[lane] = acc
        m = 1
        while m < G:
            part = [part[lane] + part[lane ^ m] for lane in range(G)]
            m <<= 1
        return part[0]
    return f


class Result(dict):
    __getattr__ = dict.__getitem__


def fit(evaluate, d, normal_factory, vsum=seq_sum, log=math.log, num_draws=1000, max_iters=100,
        history_size=6, rank=None):
    """Pathfinder.fit/2 (:30-56). normal_factory() returns a fresh normal() of the seeded generator;
    rank[i] = position of kernel dimension i in the flat vector (None: identity). Returns mu, sigma,
    elbo, num_iters, best_index, status, draws [num_draws][d] (kernel order, unconstrained) and the
    whole path (path, grads, elbos) and the number of pairs pushed, for the tests that look inside."""
    assert max_iters >= 1 and num_draws >= 1 and history_size >= 1
    rank = list(range(d)) if rank is None else [int(r) for r in rank]
    perm = [0] * d                       # perm[r] = kernel dimension of flat entry r
    for i, r in enumerate(rank):
        perm[r] = i

    def dot(a, b):
        return vsum([float(x) * float(y) for x, y in zip(a, b)])

    # :59-66
    normal = normal_factory()
    q = np.zeros(d)
    for r in range(d):
        q[perm[r]] = normal() * 0.1
    logp, g = evaluate(q)
    g = np.array(g, dtype=np.float64)
    path, grads, logps = [q.copy()], [g.copy()], [float(logp)]
    s_list, y_list, pushes = [], [], 0

    for _ in range(max_iters):          # :78
        direction = _direction(g, s_list, y_list, dot)
        q_new = q + ALPHA * direction   # :81
        logp_new, g_new = evaluate(q_new)
        g_new = np.array(g_new, dtype=np.float64)
        if not math.isfinite(logp_new):  # :85-86
            break
        with np.errstate(all="ignore"):
            s = q_new - q               # :88
            y = g_new - g               # :89
        ys = dot(y, s)
        if ys > PUSH_MIN:               # :93-96
            s_list = [s] + s_list[:history_size - 1]
            y_list = [y] + y_list[:history_size - 1]
            pushes += 1
        q, g = q_new, g_new
        path.append(q.copy())
        grads.append(g.copy())
        logps.append(float(logp_new))

    # :156-171, then Enum.max_by (:43): the first of the largest
    elbos, sigmas = [], []
    cst = entropy_const(d)
    with np.errstate(all="ignore"):
        for lp, gq in zip(logps, grads):
            sigma = np.array([1.0 / math.sqrt(abs(float(x)) + GRAD_EPS) if not math.isnan(x) else math.nan
                              for x in gq])
            elbos.append(lp + (cst + vsum([_log(log, float(x)) for x in sigma])))
            sigmas.append(sigma)
    best = -1
    for i, e in enumerate(elbos):
        if math.isfinite(e) and (best < 0 or e > elbos[best]):
            best = i
    if best < 0:
        mu = np.full(d, np.nan)
        sigma = np.full(d, np.nan)
        elbo = math.nan
    else:
        mu, sigma, elbo = path[best], sigmas[best], elbos[best]

    # :173-190, from the generator as seeded (:44 passes `rng`, not the one lbfgs_path advanced)
    normal = normal_factory()
    draws = np.zeros((num_draws, d))
    for n in range(num_draws):
        for r in range(d):
            z = normal()
            draws[n, perm[r]] = mu[perm[r]] + sigma[perm[r]] * z
    return Result(mu=np.array(mu), sigma=np.array(sigma), elbo=elbo, num_iters=len(path), best_index=best,
                  status=1 if best < 0 else 0, draws=draws, path=path, grads=grads, elbos=elbos,
                  pushes=pushes)


def _log(log, x):
    if math.isnan(x):
        return math.nan
    if x == 0.0:
        return -math.inf      # sigma = 0 where |g| is infinite
    return log(x)


def _direction(grad, s_list, y_list, dot):
    """lbfgs_direction (:117-154)."""
    if not s_list:
        return grad
    rhos = []
    for s, y in zip(s_list, y_list):     # :122-126
        ys = dot(y, s)
        rhos.append(1.0 / ys if ys > 0 else 0.0)
    q = grad
    alphas = []
    for s, y, rho in zip(s_list, y_list, rhos):   # :128-135, newest to oldest
        a = rho * dot(s, q)
        q = q - a * y
        alphas.append(a)
    s0, y0 = s_list[0], y_list[0]
    yy = dot(y0, y0)
    gamma = dot(s0, y0) / (yy if yy > GAMMA_MIN else GAMMA_MIN)   # :140
    r = gamma * q
    for s, y, rho, a in reversed(list(zip(s_list, y_list, rhos, alphas))):   # :143-151
        beta = rho * dot(y, r)
        r = r + (a - beta) * s
    return r


# ---- the two modes over the checker's models ------------------------------------------------------
def rng_factory(seed, math_mode):
    L = O.lib()

    def factory():
        r = O.Rng()
        L.exo_rng_seed(C.byref(r), seed)
        return lambda: L.exo_rng_normal(C.byref(r), math_mode)
    return factory


def _rank_of(model):
    order = model.flat_order()      # order[r] = kernel dimension of flat entry r
    rank = [0] * len(order)
    for r, i in enumerate(order):
        rank[i] = r
    return rank


def fit_lane(model, lanes, seed, **kw):
    """The device's statement: `model` an oracle Model (gen_checker.model for a generated one)."""
    cfg = O.Cfg(1, lanes)
    return fit(lambda q: model.logp_grad(q, cfg), model.d, rng_factory(seed, 1), vsum=lane_sum(lanes, model.d),
               log=O.lib().exo_det_log, rank=_rank_of(model), **kw)


def fit_reference(model, seed, **kw):
    cfg = O.Cfg(0, 1)
    return fit(lambda q: model.logp_grad(q, cfg), model.d, rng_factory(seed, 0), vsum=seq_sum, log=math.log,
               rank=_rank_of(model), **kw)
