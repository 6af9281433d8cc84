"""The momentum every NUTS transition draws, held to its law. A momentum is drawn fresh, independently of the
state, from N(0, M); its kinetic energy p' M^-1 p / 2 is then Gamma(d / 2, 1) whatever the mass matrix M, and
it is recoverable from the trace: ke_t = energy_t + logp_{t-1}, with the start point's logp for t = 0
(tests/test_gpu_momentum_long_way.py establishes this against the checker). So the kinetic energies of a run
with fixed tuning are i.i.d. draws of a known law, through whichever path drew the normals:
  eight_schools at 16 lanes, diagonal mass   the window of generator words the previous transition left
                                             (draw_momentum_window, normal_wedge_once), 1030 chains x 100 draws
  eight_schools at 16 lanes, dense mass      the Cholesky factor applied to the normals
  sv_ncp at 64 lanes                         130 chains x 40 draws, d = 102
The first transition of a launch has no window; it is a group of its own in every run, so the two paths are
not averaged together. The start point's logp is the device's own (exmc_hip_logp_grad_host). KS and the counts
beyond the 0.01 and 0.99 quantiles, per group.

Level: 1e-6 over at most 24 statistical assertions (3 runs x 2 groups x 3: 18), 4.2e-8 each. Seeds are fixed.
Nothing is excluded: every transition of every chain counts, divergent or not."""
import ctypes as C

import numpy as np
import pytest

import exact_distributions as E
from exmc_amd import models, sampler

pytestmark = pytest.mark.gpu

A = E.level(24)
TAIL_P = 0.01


def kinetic(energy, logp, logp0):
    """energy, logp [C][S] of the trace, logp0 the start point's -> ke [C][S]"""
    prev = np.concatenate([np.full((logp.shape[0], 1), logp0), logp[:, :-1]], axis=1)
    return energy + prev


def hold_to_gamma(ke, d, what):
    assert np.all(np.isfinite(ke))
    shape = d / 2.0
    q_lo, q_hi = E.gamma_ppf(TAIL_P, shape), E.gamma_ppf(1.0 - TAIL_P, shape)
    for name, x in (("first transition", ke[:, 0]), ("later transitions", ke[:, 1:])):
        dist, r = E.ks(x, lambda v: E.gamma_cdf(v, shape), A)
        up, ulim = E.tail_count(x, [q_hi], lambda v: E.gamma_sf(v, shape), A)
        dn, dlim = E.tail_count(-x, [-q_lo], lambda v: E.gamma_cdf(-v, shape), A)
        print("%s, %s, n=%d: KS %.3g <= %.3g; above the 0.99 quantile %d in %d..%d; below the 0.01 quantile %d in %d..%d"
              % (what, name, x.size, dist, r, up[0], ulim[0][0], ulim[1][0], dn[0], dlim[0][0], dlim[1][0]))
        assert dist <= r, (what, name)
        assert E.within(up, ulim), (what, name)
        assert E.within(dn, dlim), (what, name)


def _run(spec, tuning, lanes, chains, draws, seed):
    comp = sampler.compile(spec)
    try:
        opts = dict(num_warmup=0, num_samples=draws, seed=seed, lanes_per_chain=lanes)
        _, _, extra = sampler.sample_compiled_tuned(comp, tuning, spec.default_init, opts, num_chains=chains)
        q0 = np.ascontiguousarray(spec.to_unconstrained(spec.default_init))
        lp, g = np.zeros(1), np.zeros(spec.d)
        dp = C.POINTER(C.c_double)
        comp.check(comp.L.exmc_hip_logp_grad_host(comp.h, q0.ctypes.data_as(dp), 1, lanes, lp.ctypes.data_as(dp),
                                                  g.ctypes.data_as(dp)))
    finally:
        comp.close()
    raw = extra["raw"]
    assert raw["energy"].shape == (chains, draws)
    return kinetic(raw["energy"], raw["logp"], lp[0])


def test_eight_schools_window_draw(hip):
    spec = models.eight_schools()
    tuning = dict(epsilon=0.3, inv_mass=np.linspace(0.5, 2.0, spec.d), chol_cov=None)
    hold_to_gamma(_run(spec, tuning, 16, 1030, 100, seed=31), spec.d, "eight_schools, 16 lanes, diagonal mass")


def test_eight_schools_dense_mass(hip):
    spec = models.eight_schools()
    d = spec.d
    a = np.random.default_rng(701).normal(size=(d, d)) * 0.4
    cov = np.ascontiguousarray(a @ a.T + 0.5 * np.eye(d))
    chol = np.ascontiguousarray(np.linalg.cholesky(cov))
    tuning = dict(epsilon=0.2, inv_mass=cov, cov=cov, chol_cov=chol)
    hold_to_gamma(_run(spec, tuning, 16, 1030, 100, seed=32), d, "eight_schools, 16 lanes, dense mass")


def test_sv_ncp_64_lanes(hip):
    spec = models.sv_ncp(models.sv_returns())
    tuning = dict(epsilon=0.05, inv_mass=np.linspace(0.5, 2.0, spec.d), chol_cov=None)
    hold_to_gamma(_run(spec, tuning, 64, 130, 40, seed=33), spec.d, "sv_ncp, 64 lanes")
