"""tree_prefix leaves the half-Cauchy term's logarithm out of its seven leapfrogs and evaluates the
seven as one lane-batched log_ge1 behind the seventh (EightSchools::logp_grad_pre / logp_finish,
M::kPrefixLogBatch); a row broadcast of a double is one 64-bit DPP move (exmc_device.hpp dpp_move).
Bit for bit against the checker: whole transitions at settings whose trees end at every leapfrog
count the unit can end at, go on into the walk, and diverge inside the unit at the first and at the
second leaf of a pair; the same settings with the tree capped inside the unit and at its end; and
one transition from the special points of test_gpu_es_row_sums (the exact-division replay, an
infinite value, the clamp of log tau) and from its random points.

The settings are chosen from the checker alone: for each step size, the first of seeds 1 .. 40
whose 33 x 12 transitions show at least MIN_COUNT of every class the step size is there for (the
classes and the checker's counts stand beside each setting and are asserted).
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from exmc_amd import _lib, sampler
from test_gpu_es_row_sums import (MU_HUGE, MU_INF, N_RANDOM, TAU_HI, TAU_LO, ZERO_RESID, es_unit,  # noqa: F401
                                  points)
from test_gpu_leaf_pairs import _assert_equal, _both, _start
from test_gpu_parity import _dp, _oracle_transitions, es  # noqa: F401  (es: fixture)

pytestmark = pytest.mark.gpu

LANES = 16
N_CHAINS, N_DRAWS = 33, 12   # eight full waves and one wave with three idle groups
MIN_COUNT = 5


def _classes(o):
    """How many of the checker's transitions fall into each class of tree.
    n1 .. n7: the tree ended at that many leapfrogs (inside the unit, or at its end); walk: 15 and more,
    so the tree went on past the unit; div0: leaf 0 diverged; div_first / div_second: a leaf inside
    the unit diverged as the first / the second leaf of its pair (leaf 0 is doubling 0 and leaf i >= 1
    the first of a pair iff i is odd, so the leaves up to a diverged first leaf count even)."""
    n = o["n_steps"].ravel()
    dv = o["divergent"].ravel() != 0
    return dict(n1=int((n == 1).sum()), n3=int((n == 3).sum()), n5=int((n == 5).sum()), n7=int((n == 7).sum()),
                walk=int((n >= 15).sum()), div0=int((dv & (n == 1)).sum()),
                div_first=int((dv & (n % 2 == 0) & (n >= 2) & (n <= 6)).sum()),
                div_second=int((dv & (n % 2 == 1) & (n >= 3) & (n <= 7)).sum()))


# eps: (the classes it is there for, the first qualifying seed, the checker's counts at that seed).
# Together: trees that end at 1, 3, 5 and 7 leapfrogs, trees of 15 and more, and divergences inside the
# unit at leaf 0, at a first and at a second leaf. Every class is reached at 33 x 12 within the seeds.
SETTINGS = {
    0.45: (("n3", "n7", "walk"), 1,
           dict(n1=0, n3=8, n5=0, n7=262, walk=120, div0=0, div_first=0, div_second=0)),
    1.1: (("n1", "n3", "n5", "n7", "walk", "div0", "div_first", "div_second"), 2,
          dict(n1=106, n3=126, n5=26, n7=46, walk=8, div0=70, div_first=66, div_second=66)),
    1.6: (("n1", "n3", "div0", "div_first", "div_second"), 1,
          dict(n1=205, n3=151, n5=0, n7=0, walk=0, div0=27, div_first=40, div_second=98)),
}


def _qualifies(cls, wanted):
    return all(cls[k] >= MIN_COUNT for k in wanted)


def test_settings_are_the_first_seeds_that_qualify(es):
    """The checker alone (no kernel runs): each setting's seed is the first of 1 .. 40 that shows its classes."""
    spec, comp, om = es
    seen = set()
    for eps, (wanted, seed, counts) in SETTINGS.items():
        assert 1 <= seed <= 40
        for s in range(1, seed + 1):
            cfg, q, im, g, logp, rngs = _start(om, spec.d, N_CHAINS, s)
            cls = _classes(_oracle_transitions(om, q, logp, g, rngs, N_DRAWS, eps, im, 10, cfg))
            assert _qualifies(cls, wanted) == (s == seed), (eps, s, cls)
        assert cls == counts, (eps, cls)
        seen |= set(wanted)
    assert seen == {"n1", "n3", "n5", "n7", "walk", "div0", "div_first", "div_second"}


@pytest.mark.parametrize("eps", sorted(SETTINGS))
def test_whole_transitions_bit_exact(es, hip, eps):
    wanted, seed, counts = SETTINGS[eps]
    o, t, ostate, hstate, _ = _both(es, hip, N_CHAINS, N_DRAWS, eps, 10, seed)
    cls = _classes(o)
    print(eps, seed, cls)
    assert cls == counts
    _assert_equal(o, t, ostate, hstate)


@pytest.mark.parametrize("max_depth", [1, 2, 3])
@pytest.mark.parametrize("eps", sorted(SETTINGS))
def test_tree_capped_inside_the_unit_bit_exact(es, hip, eps, max_depth):
    """max_tree_depth 1, 2, 3: the tree stops behind doubling 0, behind doubling 1 and at the unit's end."""
    wanted, seed, counts = SETTINGS[eps]
    o, t, ostate, hstate, _ = _both(es, hip, N_CHAINS, N_DRAWS, eps, max_depth, seed)
    full = (1 << max_depth) - 1
    assert (o["tree_depth"] <= max_depth).all() and (o["n_steps"] <= full).all()
    # stopped by the cap (at 1.6 no tree of the checker reaches seven leapfrogs, capped or not: n7 = 0)
    if counts["n7"] + counts["walk"] >= MIN_COUNT or max_depth < 3:
        assert (o["n_steps"] == full).sum() >= MIN_COUNT
    if eps > 1.0:
        assert (o["divergent"] != 0).sum() >= MIN_COUNT    # ... next to trees that a divergence stopped
    _assert_equal(o, t, ostate, hstate)


def test_one_transition_from_special_and_random_points_bit_exact(es_unit, hip, points):  # noqa: F811
    """One transition from each point, so that logp_grad_pre / logp_finish run on it inside the unit: zero
    residuals (the range watch fails, the exact divisions produce the lane values), mu = 1e300 and inf
    (a value of -inf; the logarithm's other lanes hold garbage), log tau = +-250 (zc at the clamp)."""
    spec, comp, om = es_unit
    q0, lp0, g0 = points
    n, d = q0.shape
    assert n == 5 + N_RANDOM
    cfg = O.Cfg(1, LANES)
    im = np.ascontiguousarray(np.random.default_rng(31).uniform(0.3, 3.0, size=d))
    rngs = np.zeros((n, 2), dtype=np.uint64)
    for c in range(n):
        r = O.Rng()
        O.lib().exo_rng_seed(C.byref(r), 7000 + c)
        rngs[c] = (r.a, r.b)
    q, g, logp = q0.copy(), g0.copy(), lp0.copy()
    hq, hg, hl, hr = q.copy(), g.copy(), logp.copy(), rngs.copy()
    t, tr = sampler._host_trace(n, 1, d)
    _lib.check(hip.exmc_hip_transitions_host(comp.h, _dp(hq), _dp(hl), _dp(hg),
                                             hr.ctypes.data_as(C.POINTER(C.c_uint64)), n, 1, 0.45,
                                             _dp(im), 10, LANES, tr))
    o = _oracle_transitions(om, q, logp, g, rngs, 1, 0.45, im, 10, cfg)
    assert (o["n_steps"][5:] >= 3).sum() >= 100    # trees that ran the pairs of the unit
    special = (ZERO_RESID, MU_HUGE, MU_INF, TAU_HI, TAU_LO)
    print({k: [o[k][c, 0] for c in special] for k in ("n_steps", "divergent", "logp")})
    for c in list(special) + [slice(5, n)]:
        for k in ("tree_depth", "n_steps", "divergent"):
            assert np.array_equal(o[k][c], t[k][c]), (c, k)
        for k in ("draws", "logp", "accept_prob", "energy"):
            assert np.array_equal(o[k][c], t[k][c], equal_nan=True), (c, k)
        for a, b in ((q, hq), (g, hg), (logp, hl)):
            assert np.array_equal(a[c], b[c], equal_nan=True), c
    assert np.array_equal(rngs, hr)
