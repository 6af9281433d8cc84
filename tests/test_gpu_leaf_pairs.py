"""The one-wave sampling kernel of eight_schools at 16 lanes walks its trees a leaf pair per pass
(exmc_nuts.hpp leaf_pair, M::kLeafPairs) and draws momenta with the lean stepping loop
(draw_momentum_lean). Whole transitions through exmc_hip_transitions_host against the checker, bit
for bit, on cases chosen so that the checker's own output shows what each one is there for: a
divergence in the first and in the second leaf of a pair, a tree ended inside a subtree, deep and
depth-capped trees, trees without a pair and with exactly one, and a momentum draw that went the
long way. 33 chains: the last wave has one live lane group.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from exmc_amd import _lib, sampler
from test_gpu_parity import _dp, _oracle_transitions, _rand_q, es  # noqa: F401  (es: fixture)

pytestmark = pytest.mark.gpu

LANES = 16


def _start(om, d, n_chains, seed):
    """Random chain states, a random diagonal mass and per-chain generator states."""
    cfg = O.Cfg(1, LANES)
    rng = np.random.default_rng(seed)
    q = _rand_q(rng, n_chains, d, 0.7)
    im = np.ascontiguousarray(rng.uniform(0.3, 3.0, size=d))
    g = np.zeros((n_chains, d))
    logp = np.zeros(n_chains)
    for c in range(n_chains):
        logp[c], g[c] = om.logp_grad(q[c], cfg)
    rngs = np.zeros((n_chains, 2), dtype=np.uint64)
    for c in range(n_chains):
        r = O.Rng()
        O.lib().exo_rng_seed(C.byref(r), 1000 * seed + c)
        rngs[c] = (r.a, r.b)
    return cfg, q, im, g, logp, rngs


def _both(es, hip, n_chains, n_draws, eps, max_depth, seed):
    """(checker's columns, kernel's columns, checker's final state, kernel's final state, rngs at the start)"""
    spec, comp, om = es
    cfg, q, im, g, logp, rngs = _start(om, spec.d, n_chains, seed)
    rngs0 = rngs.copy()
    hq, hg, hl, hr = q.copy(), g.copy(), logp.copy(), rngs.copy()
    t, tr = sampler._host_trace(n_chains, n_draws, spec.d)
    _lib.check(hip.exmc_hip_transitions_host(comp.h, _dp(hq), _dp(hl), _dp(hg),
                                             hr.ctypes.data_as(C.POINTER(C.c_uint64)), n_chains,
                                             n_draws, eps, _dp(im), max_depth, LANES, tr))
    o = _oracle_transitions(om, q, logp, g, rngs, n_draws, eps, im, max_depth, cfg)
    return o, t, (q, g, logp, rngs), (hq, hg, hl, hr), rngs0


def _assert_equal(o, t, ostate, hstate):
    for k in ("tree_depth", "n_steps", "divergent", "draws", "logp", "accept_prob", "energy"):
        assert np.array_equal(o[k], t[k]), k
    for a, b in zip(ostate, hstate):
        assert np.array_equal(a, b)


def _full(n_steps):
    """n_steps of a tree whose every doubling was completed: 2^k - 1"""
    return (n_steps & (n_steps + 1)) == 0


# what the checker's output must show for the case to be worth running
def _mixed(o):
    assert set(np.unique(o["tree_depth"])) >= {2, 3, 4}      # ... a tree of depth >= 4 among them
    assert (~_full(o["n_steps"])).any()                      # a tree ended inside a subtree


def _diverging(o):
    n = o["n_steps"][o["divergent"] != 0]
    # leaf 0 is doubling 0; leaf i >= 1 is the first leaf of a pair iff i is odd, so the count of
    # leaves up to and including a diverged first leaf is even, up to a diverged second leaf odd
    assert ((n % 2 == 0) & (n >= 2)).any()
    assert ((n % 2 == 1) & (n >= 3)).any()


def _capped(o):
    assert (o["tree_depth"] == 5).all() and (o["n_steps"] == 31).all()


def _no_pair(o):
    assert (o["n_steps"] == 1).all()


def _one_pair(o):
    assert (o["n_steps"] <= 3).all() and (o["n_steps"] == 3).any()


CASES = {
    "mixed_depths": (0.45, 10, 7, _mixed),
    "divergences": (1.6, 10, 7, _diverging),
    "full_pairs_depth_cap": (0.02, 5, 7, _capped),
    "no_pair": (0.45, 1, 7, _no_pair),
    "one_pair": (0.45, 2, 7, _one_pair),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_leaf_pair_transitions_bit_exact(es, hip, case):
    eps, max_depth, seed, shows = CASES[case]
    o, t, ostate, hstate, _ = _both(es, hip, 33, 12, eps, max_depth, seed)
    shows(o)
    _assert_equal(o, t, ostate, hstate)


def _words_between(r0, r1, limit):
    """generator words from state r0 to state r1 (one word a step), or None past `limit`"""
    r = O.Rng(int(r0[0]), int(r0[1]))
    for n in range(limit + 1):
        if (r.a, r.b) == (int(r1[0]), int(r1[1])):
            return n
        O.lib().exo_rng_uniform(C.byref(r))
    return None


def _long_way_draws(r0, d, n_draws, cfg):
    """The checker's generator walked through a chain's run (per transition: d normal variates, then
    one uniform; the tree draws from a copy): for every momentum draw that took more than its first
    word, (dimension, whether the draw before it in the same transition did too). Also the state
    the walk ends in."""
    L = O.lib()
    r = O.Rng(int(r0[0]), int(r0[1]))
    out = []
    for _ in range(n_draws):
        prev_long = False
        for i in range(d):
            before = (r.a, r.b)
            L.exo_rng_normal(C.byref(r), cfg.math_mode)
            long_way = _words_between(before, (r.a, r.b), 64) > 1
            if long_way:
                out.append((i, prev_long))
            prev_long = long_way
        L.exo_rng_uniform(C.byref(r))
    return out, (r.a, r.b)


MOMENTUM_SEED = 3


def test_momentum_long_way_draws_bit_exact(es, hip):
    """64 chains x 20 draws: the energy column (-jlp0: the momentum as drawn) and the generator
    states behind the run. A transition consumes d words for its momentum and one more at its end
    when every normal variate takes its first word; a chain that consumed more than 20 (d + 1) words
    drew at least one variate the long way. Stepping the checker's generator shows which draws did,
    and that both ways draw_momentum_lean finds the head word of such a draw's state are in the
    sample: from the state its pass started at (dimension 0) and from the lane of the dimension
    before (a later dimension whose predecessor took its first word)."""
    spec = es[0]
    n_chains, n_draws = 64, 20
    o, t, ostate, hstate, rngs0 = _both(es, hip, n_chains, n_draws, 0.45, 10, MOMENTUM_SEED)
    least = n_draws * (spec.d + 1)
    words = [_words_between(rngs0[c], ostate[3][c], least + 400) for c in range(n_chains)]
    assert None not in words and min(words) >= least
    assert sum(w > least for w in words) >= 8   # expected: 0.015 x 200 words = 3 per chain
    cfg = O.Cfg(1, LANES)
    long_way = []
    for c in range(n_chains):
        lw, end = _long_way_draws(rngs0[c], spec.d, n_draws, cfg)
        assert end == (int(ostate[3][c][0]), int(ostate[3][c][1]))   # the walk is the checker's stream
        long_way += lw
    assert any(i == 0 for i, _ in long_way)                       # head word: the pass's entry state
    assert any(i > 0 and not prev for i, prev in long_way)        # head word: the previous lane's tail
    assert any(prev for _, prev in long_way)                      # ... the entry state of a later pass
    assert np.array_equal(o["energy"], t["energy"])
    assert np.array_equal(ostate[3], hstate[3])
    _assert_equal(o, t, ostate, hstate)
