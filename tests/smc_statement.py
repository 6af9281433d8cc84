"""A plain-Python statement of Exmc.SMC (lib/exmc/smc.ex), written from its text and citing its lines.
TEST INFRASTRUCTURE: the product never imports it.

The statement is parametrised by
  evaluate(q) -> logp           the model's value (Compiler.compile's logp_fn)
  psum(v) -> float              a sum over the particles of a run (Enum.sum)
  exp(x), log(x) -> float       :math.exp, :math.log
  run_gen, slot_gens[j]         generators with .normal() and .uniform(): the one that serves the uniform
                                of a resampling, and the one of particle slot j
and comes in two modes:
  lane mode       the device's arithmetic: the checker's model in the lane layout (oracle Cfg(1, G)),
                  exo_rng_normal(..., 1), exo_rng_uniform, exo_det_exp, exo_det_log, particle_sum as
                  exmc_smc.hpp states it, and the per-slot generators of include/exmc_hip_smc.h
  reference mode  the reference's arithmetic as far as Python has it: Cfg(0, 1), libm, left-to-right
                  sums, and ONE running generator: run_gen and every slot_gens[j] are the same object,
                  and the loops below visit them in the reference's own order
Products and sums round separately.

Stated deviations from smc.ex (DESIGN.md "SMC"): the generators of lane mode; at u = 0 the reference
raises (:math.log(0.0)) and here the proposal is accepted; max_stages bounds the loop (status 1); the
particles are in the unconstrained kernel space in kernel order."""
import ctypes as C
import math

import numpy as np

import oracle as O
from pathfinder_statement import Result, _rank_of, seq_sum

# smc.ex:12-17, the header's literals
DEFAULTS = dict(num_particles=500, threshold_ratio=0.5, num_mh_steps=5, seed=0)
INIT_SCALE = 0.5          # :51
NON_FINITE = -1.0e10      # :35, :223
VAR_FLOOR = 1.0e-10       # :205
RW_FACTOR = 2.38          # :205
BISECT_EVALS = 51         # iter = 0 .. 50 (:157)
DEFAULT_MAX_STAGES = 1000
SCAN_BLOCK = 4096         # exmc_psis_ratio.hpp kRatioScan
MASK64 = (1 << 64) - 1


def particle_sum(v):
    """exmc_smc.hpp particle_sum: partial t of 256 adds the terms j = t (mod 256) in ascending j from 0.0;
    the partials are combined by the xor butterfly m = 1, 2, ..., 128, lane t taking part[t] + part[t ^ m]."""
    v = np.asarray(v, dtype=np.float64)
    part = np.zeros(256)
    for j0 in range(0, len(v), 256):
        row = v[j0:j0 + 256]
        part[:len(row)] = part[:len(row)] + row
    lane = np.arange(256)
    m = 1
    while m < 256:
        part = part + part[lane ^ m]
        m <<= 1
    return float(part[0])


class Gen:
    """one :rand exsss generator of the checker; math_mode 1: the device's normal_s"""

    def __init__(self, seed, math_mode):
        self.r, self.mode, self.L = O.Rng(), math_mode, O.lib()
        self.L.exo_rng_seed(C.byref(self.r), seed & MASK64)

    def normal(self):
        return self.L.exo_rng_normal(C.byref(self.r), self.mode)

    def uniform(self):
        return self.L.exo_rng_uniform(C.byref(self.r))


def run_seed(seed, run):
    return (seed + 7919 * run) & MASK64


def lane_generators(seed_r, n):
    """include/exmc_hip_smc.h: the run generator and the generator of every slot"""
    return Gen(seed_r, 1), [Gen(seed_r ^ (((j + 1) << 32) & MASK64), 1) for j in range(n)]


def reference_generators(seed, n):
    g = Gen(seed, 0)          # :28
    return g, [g] * n


def weights(logps, delta, psum, exp):
    """:107-117 and :161-167: the normalised weights at delta and their ESS"""
    x = [delta * lp for lp in logps]
    mx = max(x)
    w = [exp(xi - mx) for xi in x]
    sw = psum(w)
    nw = [wi / sw for wi in w]
    return nw, 1.0 / psum([a * a for a in nw])


def find_next_beta(logps, beta, threshold, psum, exp):
    """:147-178. Returns (beta, evaluations, met): met says the ESS came within 1.0 of the threshold."""
    lo, hi = beta, 1.0
    for it in range(BISECT_EVALS):
        mid = (lo + hi) / 2
        _, ess = weights(logps, mid - beta, psum, exp)
        if abs(ess - threshold) < 1.0:
            return mid, it + 1, True
        if ess < threshold:
            hi = mid
        else:
            lo = mid
    return (lo + hi) / 2, BISECT_EVALS, False


def cumulative(nw):
    """Enum.scan (:185) in the order of exmc_psis_ratio.hpp: blocks of 4096 from 0.0, the bases left to right"""
    cum, base = [], 0.0
    for b0 in range(0, len(nw), SCAN_BLOCK):
        r = 0.0
        for x in nw[b0:b0 + SCAN_BLOCK]:
            r = r + x
            cum.append(base + r)
        base = base + r
    return cum


def resample_indices(nw, u):
    """:181-190"""
    n = len(nw)
    u_start = u / n
    cum = cumulative(nw)
    idx = []
    for i in range(n):
        pos = u_start + i / n
        idx.append(next((k for k, c in enumerate(cum) if c >= pos), n - 1))
    return idx


def estimate_scale(particles, d, psum):
    """:197-207"""
    n = len(particles)
    out = np.zeros(d)
    for dim in range(d):
        vals = [float(p[dim]) for p in particles]
        mean = psum(vals) / n
        var = psum([(v - mean) * (v - mean) for v in vals]) / max(n - 1, 1)
        out[dim] = math.sqrt(max(var, VAR_FLOOR)) * RW_FACTOR / math.sqrt(d)
    return out


def _guard(f, at_fail):
    def g(x):
        try:
            return f(x)
        except (OverflowError, ValueError):
            return at_fail
    return g


def sample(evaluate, d, run_gen, slot_gens, psum=seq_sum, exp=math.exp, log=math.log, threshold_ratio=0.5,
           num_mh_steps=5, max_stages=DEFAULT_MAX_STAGES, rank=None):
    """SMC.sample/2 (:19-44) with num_particles = len(slot_gens). rank[i] = position of kernel dimension i in
    the flat vector (None: identity). Returns particles [N][d] (kernel order, unconstrained), logp [N],
    betas, ess_history, acceptance_rates (lists of num_stages), num_stages, status, and what the tests
    look at: indices (per stage, None without a resampling), bisect (per stage: evaluations, met) and
    non_finite, the evaluations that took the -1.0e10 branch."""
    n = len(slot_gens)
    assert n >= 1 and num_mh_steps >= 1 and max_stages >= 1 and math.isfinite(threshold_ratio)
    rank = list(range(d)) if rank is None else [int(r) for r in rank]
    perm = [0] * d                       # perm[r] = kernel dimension of flat entry r
    for i, r in enumerate(rank):
        perm[r] = i
    exp = _guard(exp, math.inf)
    non_finite = [0]

    def logp(q):
        v = float(evaluate(q))
        if math.isfinite(v):             # is_number (:35) fails for NaN and both infinities
            return v
        non_finite[0] += 1
        return NON_FINITE

    particles = []
    for j in range(n):                   # :46-56
        q = np.zeros(d)
        for r in range(d):
            q[perm[r]] = slot_gens[j].normal() * INIT_SCALE
        particles.append(q)
    logps = [logp(q) for q in particles]     # :32-36

    threshold = threshold_ratio * n      # :59
    beta = 0.0
    betas, ess_hist, acc_hist, indices, bisect = [], [], [], [], []
    while beta < 1.0 and len(betas) < max_stages:        # :78
        nb, evals, met = find_next_beta(logps, beta, threshold, psum, exp)   # :103
        bisect.append((evals, met))
        new_beta = min(nb, 1.0)          # :104
        nw, ess = weights(logps, new_beta - beta, psum, exp)                 # :105-117
        if ess < threshold:              # :120
            idx = resample_indices(nw, run_gen.uniform())
            particles = [particles[i].copy() for i in idx]
            logps = [logps[i] for i in idx]
            indices.append(idx)
        else:
            indices.append(None)
        scale = estimate_scale(particles, d, psum)       # :126
        accepted = 0
        for _ in range(num_mh_steps):    # :211
            for j in range(n):           # :214
                g = slot_gens[j]
                prop = particles[j].copy()
                for r in range(d):       # :216-221
                    i = perm[r]
                    prop[i] = particles[j][i] + g.normal() * scale[i]
                lp_prop = logp(prop)     # :222-223
                log_alpha = new_beta * (lp_prop - logps[j])   # :227
                u = g.uniform()          # :232
                if u == 0.0 or log(u) < log_alpha:            # :234; u = 0: a stated deviation
                    particles[j], logps[j] = prop, lp_prop
                    accepted += 1
        acc_hist.append(accepted / max(n * num_mh_steps, 1))  # :245
        betas.append(new_beta)
        ess_hist.append(ess)
        beta = new_beta
    return Result(particles=np.array(particles).reshape(n, d), logp=np.array(logps), betas=betas,
                  ess_history=ess_hist, acceptance_rates=acc_hist, num_stages=len(betas),
                  status=0 if beta >= 1.0 else 1, indices=indices, bisect=bisect, non_finite=non_finite[0])


def padded(results, max_stages):
    """The arrays of exmc_hip_smc_host for a batch of statement runs: histories [R][max_stages], NaN at
    and after num_stages."""
    out = dict(particles=np.stack([r.particles for r in results]), logp=np.stack([r.logp for r in results]),
               num_stages=np.array([r.num_stages for r in results], np.int32),
               status=np.array([r.status for r in results], np.int32))
    for k in ("betas", "ess_history", "acceptance_rates"):
        h = np.full((len(results), max_stages), np.nan)
        for i, r in enumerate(results):
            h[i, :r.num_stages] = r[k]
        out[k] = h
    return out


# ---- the two modes over the checker's models ------------------------------------------------------
def sample_lane(model, lanes, seed, num_particles=500, run=0, **kw):
    """The device's statement of run `run` of a call: `model` an oracle Model (gen_checker.model for a
    generated one)."""
    cfg = O.Cfg(1, lanes)
    L = O.lib()
    run_gen, slots = lane_generators(run_seed(seed, run), num_particles)
    return sample(lambda q: model.logp_grad(q, cfg)[0], model.d, run_gen, slots, psum=particle_sum,
                  exp=L.exo_det_exp, log=L.exo_det_log, rank=_rank_of(model), **kw)


def sample_reference(model, seed, num_particles=500, **kw):
    cfg = O.Cfg(0, 1)
    run_gen, slots = reference_generators(seed, num_particles)
    return sample(lambda q: model.logp_grad(q, cfg)[0], model.d, run_gen, slots, psum=seq_sum, exp=math.exp,
                  log=math.log, rank=_rank_of(model), **kw)
