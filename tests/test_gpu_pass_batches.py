"""The leaf-pair pass of eight_schools at 16 lanes evaluates independent exponentials and logarithms of
one pass together. What this file guards in the library as built: M::kLeafPairExp -- the three
exponentials of a leaf pair as one lane-batched evaluation -- and M::kOuterLogPair -- the outer merge's
two logarithms as one main path with two fix-ups (exmc_nuts.hpp leaf_pair, nuts_run). Whole transitions
through exmc_hip_transitions_host against the checker, bit for bit, on all seven trace columns and the
final state. Every case first asserts on the checker's own output that it shows what it is there for: the
longest merge chains of a pass (pair, inner merges at every stack level, outer merge), trees ended inside
a subtree (a turning node passes the levels at which nodes park), divergences in the lone leaf and in
either leaf of a pair, and non-finite or huge arguments through the doubling-0 leaf. 33 chains: the last
wave has one live lane group. Two more batches were checked by this file once, each alone and together
with the others ("Round 8"): a merge's proposal weight with the next merge's
log_sum_exp exponential (M::kPassExpPairs: measured to lose, no model switches it on), and the two model
logarithms of a leaf pair (measured not to gain; its code is gone from the tree).
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from exmc_amd import _lib, sampler
from test_gpu_leaf_pairs import LANES, _assert_equal, _full, _start
from test_gpu_parity import _dp, _oracle_transitions, es  # noqa: F401  (es: fixture)

pytestmark = pytest.mark.gpu

N_CHAINS, N_DRAWS, SEED = 33, 12, 11


def _no_poke(q):
    return []


def _poke(q):
    """four chains of the mixed case's starts overwritten; returns the chains touched"""
    q[0, 2] = 1e160
    q[3, 0] = 1e200
    q[1, 1] = 250.0
    q[2, 1] = -250.0
    return [0, 1, 2, 3]


def _checker(es, eps, max_depth, poke):
    """(checker's columns, checker's final state, the start both sides run from)"""
    spec, comp, om = es
    cfg, q, im, g, logp, rngs = _start(om, spec.d, N_CHAINS, SEED)
    for c in poke(q):
        logp[c], g[c] = om.logp_grad(q[c], cfg)
    start = (q.copy(), g.copy(), logp.copy(), rngs.copy(), im)
    o = _oracle_transitions(om, q, logp, g, rngs, N_DRAWS, eps, im, max_depth, cfg)
    return o, (q, g, logp, rngs), start


def _kernel(es, hip, start, eps, max_depth):
    spec, comp, om = es
    q, g, logp, rngs, im = start
    hq, hg, hl, hr = q.copy(), g.copy(), logp.copy(), rngs.copy()
    t, tr = sampler._host_trace(N_CHAINS, N_DRAWS, spec.d)
    _lib.check(hip.exmc_hip_transitions_host(comp.h, _dp(hq), _dp(hl), _dp(hg),
                                             hr.ctypes.data_as(C.POINTER(C.c_uint64)), N_CHAINS,
                                             N_DRAWS, eps, _dp(im), max_depth, LANES, tr))
    return t, (hq, hg, hl, hr)


# what the checker's output must show for the case to be worth running
def _cap4(o, start):
    assert (o["tree_depth"] == 4).all() and (o["n_steps"] == 15).all()   # pair, inner, inner, outer in one pass


def _cap6(o, start):
    assert (o["tree_depth"] == 6).all() and (o["n_steps"] == 63).all()   # the longest chains, all LDS levels


def _mixed(o, start):
    assert set(np.unique(o["tree_depth"])) >= {1, 2, 3, 4, 5}
    ended_inside = set(o["n_steps"][~_full(o["n_steps"])].tolist())
    assert ended_inside >= {4, 5, 9, 11, 13, 23}
    assert int((o["divergent"] != 0).sum()) == 2


def _diverging(o, start):
    n = set(o["n_steps"][o["divergent"] != 0].tolist())
    assert n >= {1, 2, 3}   # the lone leaf, the first and the second leaf of a pair


def _poked(o, start):
    logp0 = start[2]
    assert logp0[0] == -np.inf and logp0[3] == -np.inf
    assert np.isfinite(logp0[1]) and logp0[1] < -1e171
    for c in (0, 1, 3):   # every draw: one leaf, divergent, nothing accepted
        assert (o["n_steps"][c] == 1).all() and (o["divergent"][c] != 0).all() and (o["accept_prob"][c] == 0.0).all()
    n2 = o["n_steps"][2].tolist()
    assert {275, 215, 39} <= set(n2)
    assert o["divergent"][2][n2.index(275)] != 0   # a divergence at an odd leaf count, in the spilled levels


CASES = {
    "depth_cap_4": (0.02, 4, _no_poke, _cap4),
    "depth_cap_6": (0.02, 6, _no_poke, _cap6),
    "mixed_depths": (0.45, 10, _no_poke, _mixed),
    "divergences": (1.6, 10, _no_poke, _diverging),
    "poked_starts": (0.45, 10, _poke, _poked),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_pass_batches_transitions_bit_exact(es, hip, case):
    eps, max_depth, poke, shows = CASES[case]
    o, ostate, start = _checker(es, eps, max_depth, poke)
    shows(o, start)
    t, hstate = _kernel(es, hip, start, eps, max_depth)
    _assert_equal(o, t, ostate, hstate)
