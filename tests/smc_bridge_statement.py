"""A plain-Python statement of bridged SMC (DESIGN.md "Bridged SMC", include/exmc_hip_smc_bridge.h): the
tempered sampler of tests/smc_statement.py along the geometric bridge from a normalised diagonal normal
q0 = N(mu, diag sigma^2) to the model's density, log pi_beta = beta logp + (1 - beta) log q0, with the
log evidence. TEST INFRASTRUCTURE: the product never imports it.

It takes particle_sum, the generators, weights, the bisection, the cumulative sums and the scale from
smc_statement and restates the seven items of the contract (line numbers of smc.ex where they still apply):
  1 base      lb(q) = -(vsum(0.5 * (z * z) + log(sigma))) - 0.5 d log(2 pi), z = (q - mu) / sigma: the logq of
              exmc_fit_psis.hpp in its EXMC_FIT_SIGMA form; absent mu 0.0, sigma 0.5; not finite or
              sigma <= 0: refused
  2 init      q_i = mu_i + sigma_i * v in the flat order; lp with the -1.0e10 rule; lb
  3 next beta on lr = lp - lb: the ESS at 1.0 - beta first, new_beta = 1.0 when it is >= threshold;
              otherwise the bisection of :157-178, then min(., 1.0)
  4 evidence  inc = mx + log(sw / N) at new_beta - beta, summed in stage order from 0.0
  5 resample  every stage, one uniform of the run generator per stage; q, lp and lb gathered
  6 mutation  log_alpha = (new_beta lp' + omb lb') - (new_beta lp + omb lb), omb = 1.0 - new_beta; accepted
              when u == 0.0 or log(u) < log_alpha; a NaN log_alpha rejects
  7 the rest  max_stages, status, the histories and acceptance_rates as in smc_statement
The two modes are smc_statement's: lane mode (the device's arithmetic, vsum the lane layout's sum of
fit_psis_statement) and reference mode (libm, left-to-right sums, one running generator). The index search
of the resampling is a bisection of the non-decreasing cumulative sums: the first k with cum_k >= pos."""
import bisect
import math

import numpy as np

import fit_psis_statement as FS
import oracle as O
import smc_statement as SS
from pathfinder_statement import Result, _rank_of, seq_sum

DEFAULT_MU = 0.0
DEFAULT_SIGMA = 0.5       # smc.ex:51, the start of the existing mode


def base_arrays(d, mu=None, sigma=None):
    """item 1: the base of a call, checked"""
    mu = np.full(d, DEFAULT_MU) if mu is None else np.array(mu, dtype=np.float64).reshape(-1)
    sigma = np.full(d, DEFAULT_SIGMA) if sigma is None else np.array(sigma, dtype=np.float64).reshape(-1)
    if mu.shape != (d,) or sigma.shape != (d,):
        raise ValueError("the base needs d entries")
    if not (np.all(np.isfinite(mu)) and np.all(np.isfinite(sigma)) and np.all(sigma > 0.0)):
        raise ValueError("the base needs finite mu and finite sigma > 0")
    return mu, sigma


def base_logq(mu, sigma, vsum, log):
    """q -> lb(q)"""
    d = len(mu)
    ls = np.array([log(float(s)) for s in sigma])
    c = 0.5 * d * math.log(2.0 * math.pi)

    def lb(q):
        with np.errstate(all="ignore"):
            z = (np.asarray(q, dtype=np.float64) - mu) / sigma
            t = 0.5 * (z * z) + ls
        return -vsum(t) - c
    return lb


def increment(lrs, delta, psum, exp, log):
    """item 4: mx + log(sw / N) of the unnormalised weights at delta"""
    x = [delta * v for v in lrs]
    mx = max(x)
    sw = psum([exp(xi - mx) for xi in x])
    return mx + log(sw / float(len(lrs)))


def resample_indices(nw, u):
    """smc.ex:181-190, the search by bisection"""
    n = len(nw)
    u_start = u / n
    cum = SS.cumulative(nw)
    return [min(bisect.bisect_left(cum, u_start + i / n), n - 1) for i in range(n)]


def pooled_log_evidence(log_evidences):
    """the log of the mean of exp(log_evidence) over runs"""
    le = np.asarray(log_evidences, dtype=np.float64).reshape(-1)
    m = float(np.max(le))
    if not math.isfinite(m):
        return m
    return m + math.log(float(np.mean(np.exp(le - m))))


def sample(evaluate, d, run_gen, slot_gens, mu=None, sigma=None, vsum=seq_sum, psum=seq_sum, exp=math.exp,
           log=math.log, threshold_ratio=0.5, num_mh_steps=5, max_stages=SS.DEFAULT_MAX_STAGES, rank=None):
    """Bridged SMC with num_particles = len(slot_gens). Returns what smc_statement.sample returns, and logb
    [N], log_evidence, log_evidence_steps (a list of num_stages); bisect holds per stage (evaluations of the
    bisection, met, direct): direct says the evaluation at 1.0 - beta ended the temper."""
    n = len(slot_gens)
    assert n >= 1 and num_mh_steps >= 1 and max_stages >= 1 and math.isfinite(threshold_ratio)
    mu, sigma = base_arrays(d, mu, sigma)
    lb_of = base_logq(mu, sigma, vsum, log)
    rank = list(range(d)) if rank is None else [int(r) for r in rank]
    perm = [0] * d                       # perm[r] = kernel dimension of flat entry r
    for i, r in enumerate(rank):
        perm[r] = i
    exp = SS._guard(exp, math.inf)
    non_finite = [0]

    def logp(q):
        v = float(evaluate(q))
        if math.isfinite(v):
            return v
        non_finite[0] += 1
        return SS.NON_FINITE

    particles = []
    for j in range(n):                   # item 2
        q = np.zeros(d)
        for r in range(d):
            i = perm[r]
            q[i] = mu[i] + sigma[i] * slot_gens[j].normal()
        particles.append(q)
    logps = [logp(q) for q in particles]
    logbs = [lb_of(q) for q in particles]

    threshold = threshold_ratio * n      # :59
    beta, log_evidence = 0.0, 0.0
    betas, ess_hist, acc_hist, indices, bis, steps = [], [], [], [], [], []
    while beta < 1.0 and len(betas) < max_stages:        # :78
        lrs = [a - b for a, b in zip(logps, logbs)]
        _, ess1 = SS.weights(lrs, 1.0 - beta, psum, exp)                     # item 3
        if ess1 >= threshold:
            new_beta = 1.0
            bis.append((0, False, True))
        else:
            nb, evals, met = SS.find_next_beta(lrs, beta, threshold, psum, exp)
            new_beta = min(nb, 1.0)
            bis.append((evals, met, False))
        nw, ess = SS.weights(lrs, new_beta - beta, psum, exp)
        inc = increment(lrs, new_beta - beta, psum, exp, log)                # item 4
        steps.append(inc)
        log_evidence = log_evidence + inc
        idx = resample_indices(nw, run_gen.uniform())                        # item 5
        particles = [particles[i].copy() for i in idx]
        logps = [logps[i] for i in idx]
        logbs = [logbs[i] for i in idx]
        indices.append(idx)
        scale = SS.estimate_scale(particles, d, psum)    # :126
        omb = 1.0 - new_beta
        accepted = 0
        for _ in range(num_mh_steps):    # item 6
            for j in range(n):
                g = slot_gens[j]
                prop = particles[j].copy()
                for r in range(d):
                    i = perm[r]
                    prop[i] = particles[j][i] + g.normal() * scale[i]
                lp_prop, lb_prop = logp(prop), lb_of(prop)
                with np.errstate(all="ignore"):
                    tc = new_beta * logps[j] + omb * logbs[j]
                    tp = new_beta * lp_prop + np.float64(omb) * np.float64(lb_prop)
                    log_alpha = float(tp - tc)
                u = g.uniform()
                if not math.isnan(log_alpha) and (u == 0.0 or log(u) < log_alpha):
                    particles[j], logps[j], logbs[j] = prop, lp_prop, lb_prop
                    accepted += 1
        acc_hist.append(accepted / max(n * num_mh_steps, 1))
        betas.append(new_beta)
        ess_hist.append(ess)
        beta = new_beta
    return Result(particles=np.array(particles).reshape(n, d), logp=np.array(logps), logb=np.array(logbs),
                  betas=betas, ess_history=ess_hist, acceptance_rates=acc_hist, num_stages=len(betas),
                  status=0 if beta >= 1.0 else 1, log_evidence=log_evidence, log_evidence_steps=steps,
                  indices=indices, bisect=bis, non_finite=non_finite[0])


def padded(results, max_stages):
    """The arrays of exmc_hip_smc_bridge_host for a batch of statement runs"""
    out = SS.padded(results, max_stages)
    out["logb"] = np.stack([r.logb for r in results])
    out["log_evidence"] = np.array([r.log_evidence for r in results], dtype=np.float64)
    h = np.full((len(results), max_stages), np.nan)
    for i, r in enumerate(results):
        h[i, :r.num_stages] = r.log_evidence_steps
    out["log_evidence_steps"] = h
    return out


# ---- the two modes over the checker's models ------------------------------------------------------
def sample_lane(model, lanes, seed, num_particles=500, run=0, **kw):
    cfg = O.Cfg(1, lanes)
    L = O.lib()
    run_gen, slots = SS.lane_generators(SS.run_seed(seed, run), num_particles)
    return sample(lambda q: model.logp_grad(q, cfg)[0], model.d, run_gen, slots, vsum=FS.lane_sum(lanes, model.d),
                  psum=SS.particle_sum, exp=L.exo_det_exp, log=L.exo_det_log, rank=_rank_of(model), **kw)


def sample_reference(model, seed, num_particles=500, **kw):
    cfg = O.Cfg(0, 1)
    run_gen, slots = SS.reference_generators(seed, num_particles)
    return sample(lambda q: model.logp_grad(q, cfg)[0], model.d, run_gen, slots, rank=_rank_of(model), **kw)
