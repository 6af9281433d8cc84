"""The draws ADVI and Pathfinder return, held to their law. By their statements (tests/advi_statement.py:
draws[s, i] = mu[i] + sigma[i] * v with sigma = exp(log_sigma); tests/pathfinder_statement.py: draws[n, i] =
mu[i] + sigma[i] * z) a draw is mu + sigma v with v a standard normal variate of the fit's own generator
(seed + 7919 c), one per dimension and draw. So (draw - mu) / sigma, pooled over draws, dimensions and fits,
is an i.i.d. standard normal sample whatever the fit found: eight_schools, 130 fits (two wavefronts' worth and
more, the last partial) x 1000 draws x 10 dimensions = 1.3e6 values per method, few iterations.
  KS against N(0, 1); the mean per dimension; the correlation of every pair of dimensions, within each fit
  (1000 draws) and pooled over the fits (130 000 draws) -- a variate used for two lanes would show there.
A fit or path that failed would be excluded: one the CPU statement of the same seed reports as failed (a path
of status 1, a fit with a sample that took the non-finite branch), or whose mu or sigma the device returns
non-finite. The options and seeds are such that there is none, and the test asserts that nothing was excluded.
The statements say which fits count; no value of theirs is compared with the device's.

Level: 1e-6 over at most 16 statistical assertions (2 methods x 4: 8), 6.25e-8 each, split again over the
dimensions, pairs and fits an assertion covers. Seeds are fixed."""
import math

import numpy as np
import pytest

import advi_statement as AS
import exact_distributions as E
import oracle as O
import pathfinder_statement as PFS
from exmc_amd import advi, models, pathfinder, sampler

pytestmark = pytest.mark.gpu

A = E.level(16)
FITS, DRAWS = 130, 1000
ADVI_OPTS = dict(num_draws=DRAWS, max_iters=4, window_size=2, num_mc_samples=1, learning_rate=0.01, seed=51)
PF_OPTS = dict(num_draws=DRAWS, max_iters=5, history_size=3, seed=52)


def hold_to_standard_normal(v, what):
    """v [fits][draws][d]"""
    Cn, S, d = v.shape
    assert np.all(np.isfinite(v)) and v.size >= 1000000
    dist, r = E.ks(v, E.normal_cdf, A)
    zm = np.abs(v.mean(axis=(0, 1))) * math.sqrt(Cn * S)
    zb = E.normal_bound(A / d)
    iu = np.triu_indices(d, 1)
    within = np.array([np.abs(np.corrcoef(v[c].T)[iu]).max() for c in range(Cn)])
    wb = E.correlation_bound(S, A / (Cn * iu[0].size))
    pooled = np.abs(np.corrcoef(v.reshape(-1, d).T)[iu]).max()
    pb = E.correlation_bound(Cn * S, A / iu[0].size)
    print("%s n=%d: KS %.3g <= %.3g; max dimension mean %.2f <= %.2f sigma; max |r| within a fit %.3g <= %.3g, "
          "pooled %.3g <= %.3g" % (what, v.size, dist, r, zm.max(), zb, within.max(), wb, pooled, pb))
    assert dist <= r
    assert zm.max() <= zb, int(np.argmax(zm))
    assert within.max() <= wb, int(np.argmax(within))
    assert pooled <= pb


def standardise(draws, mu, sigma, failed):
    """(draw - mu) / sigma of the fits that did not fail; nothing may have"""
    bad = failed | ~np.all(np.isfinite(mu), axis=1) | ~np.all(np.isfinite(sigma) & (sigma > 0.0), axis=1)
    assert not bad.any(), np.flatnonzero(bad)
    return (draws - mu[:, None, :]) / sigma[:, None, :]


def test_advi_draws_are_mu_plus_sigma_times_a_standard_normal(hip):
    comp = sampler.compile(models.eight_schools())
    try:
        out = advi.fit_raw(comp, ADVI_OPTS, num_fits=FITS)
    finally:
        comp.close()
    assert out["draws"].shape == (FITS, DRAWS, 10) and np.all(out["num_iters"] >= 1)
    kw = {k: x for k, x in ADVI_OPTS.items() if k not in ("seed", "num_draws")}
    m = O.eight_schools()
    failed = np.array([AS.fit_lane(m, 16, ADVI_OPTS["seed"] + 7919 * c, num_draws=1, **kw).non_finite > 0 for c in range(FITS)])
    v = standardise(out["draws"], out["mu"], np.exp(out["log_sigma"]), failed)
    hold_to_standard_normal(v, "advi")


def test_pathfinder_draws_are_mu_plus_sigma_times_a_standard_normal(hip):
    comp = sampler.compile(models.eight_schools())
    try:
        out = pathfinder.fit_raw(comp, PF_OPTS, num_paths=FITS)
    finally:
        comp.close()
    assert out["draws"].shape == (FITS, DRAWS, 10)
    kw = {k: x for k, x in PF_OPTS.items() if k not in ("seed", "num_draws")}
    m = O.eight_schools()
    failed = np.array([PFS.fit_lane(m, 16, PF_OPTS["seed"] + 7919 * c, num_draws=1, **kw).status != 0 for c in range(FITS)])
    v = standardise(out["draws"], out["mu"], out["sigma"], failed | (out["status"] != 0))
    hold_to_standard_normal(v, "pathfinder")
