"""eight_schools at 16 lanes sums its three likelihood terms over the lanes that hold one (2 .. 9,
exmc_device.hpp row_seqsum_lanes), watches the range of its two numerators once, and the outer merge
of doubling 0 in tree_prefix decides its U-turn by one test instead of three equal ones. Bit for bit
against the checker: transitions whose tree ends at doubling 0 by a U-turn next to ones that go on,
and the model's value and gradient -- alone and inside one transition -- on data and points where a
sum's first term is -0.0, where the range watch fails and the exact divisions run through the same
sums, and at the clamp of log tau.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from exmc_amd import _lib, models, sampler
from test_gpu_leaf_pairs import _assert_equal, _both
from test_gpu_parity import _dp, _oracle_transitions, _rand_q, es  # noqa: F401  (es: fixture)

pytestmark = pytest.mark.gpu

LANES = 16

# (eps, seed): of the checker's 396 transitions, (one leapfrog without divergence, one leapfrog
# divergent, going on) = (134, 10, 252), (262, 12, 122), (51, 2, 343)
DOUBLING0 = [(1.6, 7), (1.6, 12), (1.1, 12)]


@pytest.mark.parametrize("eps,seed", DOUBLING0)
def test_doubling0_uturn_bit_exact(es, hip, eps, seed):
    o, t, ostate, hstate, _ = _both(es, hip, 33, 12, eps, 10, seed)
    one = o["n_steps"] == 1
    assert (one & (o["divergent"] == 0)).sum() >= 50   # ended by the U-turn test of doubling 0
    assert (~one).sum() >= 100                         # the same test let the tree go on
    _assert_equal(o, t, ostate, hstate)


Y = [3.0, -1.0, 2.0, 0.5, -2.5, 1.0, 4.0, -0.25]
SIGMA = [1.0, 1.0, 2.0, 1.0, 0.5, 1.0, 1.0, 4.0]
N_RANDOM = 300
ZERO_RESID, MU_HUGE, MU_INF, TAU_HI, TAU_LO = range(5)


@pytest.fixture(scope="module")
def es_unit(hip):
    spec = models.eight_schools(y=Y, sigma=SIGMA)
    return spec, sampler.compile(spec), O.model_for(spec)


@pytest.fixture(scope="module")
def points(es_unit):
    """The points and the checker's value and gradient at each, computed once."""
    spec, comp, om = es_unit
    base = np.array([0.0, 0.0] + Y)    # mu = 0, tau = 1, theta_j = y_j: every residual is exactly 0
    rows = [base.copy() for _ in range(5)]
    rows[MU_HUGE][0] = 1e300
    rows[MU_INF][0] = np.inf
    rows[TAU_HI][1] = 250.0
    rows[TAU_LO][1] = -250.0
    q = np.ascontiguousarray(np.vstack([np.array(rows), _rand_q(np.random.default_rng(23), N_RANDOM, spec.d, 1.5)]))
    cfg = O.Cfg(1, LANES)
    lp = np.zeros(q.shape[0])
    g = np.zeros(q.shape)
    for c in range(q.shape[0]):
        lp[c], g[c] = om.logp_grad(q[c], cfg)
    # lane 2's first term is -0.0 (sigma_0 = 1: -0.5 * 0 - log 1); the watch fails on a zero residual
    assert lp[ZERO_RESID] == -32.147670257289946
    assert lp[MU_HUGE] == -np.inf and lp[MU_INF] == -np.inf
    assert np.isfinite(lp[5:]).all()
    q.setflags(write=False); lp.setflags(write=False); g.setflags(write=False)
    return q, lp, g


def test_row_sums_logp_grad_bit_exact(es_unit, hip, points):
    spec, comp, om = es_unit
    q, olp, og = points
    n = q.shape[0]
    hq = q.copy()
    lp = np.zeros(n)
    g = np.zeros((n, spec.d))
    _lib.check(hip.exmc_hip_logp_grad_host(comp.h, _dp(hq), n, LANES, _dp(lp), _dp(g)))
    for c in range(n):
        assert np.array_equal(olp[c:c + 1], lp[c:c + 1], equal_nan=True), (c, olp[c], lp[c])
        assert np.array_equal(og[c], g[c], equal_nan=True), (c, og[c], g[c])


def test_row_sums_inside_one_transition_bit_exact(es_unit, hip, points):
    """One transition from every point, so that the model's copies inside tree_prefix run on them."""
    spec, comp, om = es_unit
    q0, lp0, g0 = points
    n, d = q0.shape
    cfg = O.Cfg(1, LANES)
    im = np.ascontiguousarray(np.random.default_rng(29).uniform(0.3, 3.0, size=d))
    rngs = np.zeros((n, 2), dtype=np.uint64)
    for c in range(n):
        r = O.Rng()
        O.lib().exo_rng_seed(C.byref(r), 5000 + c)
        rngs[c] = (r.a, r.b)
    q, g, logp = q0.copy(), g0.copy(), lp0.copy()
    hq, hg, hl, hr = q.copy(), g.copy(), logp.copy(), rngs.copy()
    t, tr = sampler._host_trace(n, 1, d)
    _lib.check(hip.exmc_hip_transitions_host(comp.h, _dp(hq), _dp(hl), _dp(hg),
                                             hr.ctypes.data_as(C.POINTER(C.c_uint64)), n, 1, 0.45,
                                             _dp(im), 10, LANES, tr))
    o = _oracle_transitions(om, q, logp, g, rngs, 1, 0.45, im, 10, cfg)
    assert (o["n_steps"][5:] >= 3).sum() >= 100    # trees that ran the pairs of the unit
    for k in ("tree_depth", "n_steps", "divergent"):
        assert np.array_equal(o[k], t[k]), k
    for k in ("draws", "logp", "accept_prob", "energy"):
        assert np.array_equal(o[k], t[k], equal_nan=True), k
    for a, b in ((q, hq), (g, hg), (logp, hl)):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(rngs, hr)
