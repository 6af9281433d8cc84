"""The one-wave sampling kernel of eight_schools at 16 lanes walks a chain's generator once per
transition (exmc_nuts.hpp RngRowWindow, M::kRngWindow): tree_prefix builds a window of W = 14 words
from the state behind the momentum, takes its ten uniforms from it, and the NEXT transition's
momentum reads its normals out of the same window -- draw r the word at 1 + r + shift, shift = the
words earlier draws of that momentum consumed beyond their first (draw_momentum_window). W = 14
holds every word up to shift 2; a group that gets past it goes on in the stepping loop. A call's first
transition has no window. Whole transitions through exmc_hip_transitions_host against the checker,
bit for bit -- every column and the final state, the generator included.

Every case first derives the extra words of every momentum draw from the checker's generator alone
(the main stream does not depend on the tree: per transition ten normals, then one uniform) and
asserts that the stream shows what the case is there for. 33 chains: chains 4w .. 4w + 3 share a
wave, and the last wave has one live lane group.

The streaming twin of the kernel starts from a seed and its own warmup (exmc_hip_stream_begin), not
from given states and generators. Its windows, shifts, prefix divergences and depth caps are reached
by steering that start (num_warmup, target_accept, max_tree_depth, seed) and held to the checker's
sample/3 in tests/test_gpu_stream_push.py.
"""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import oracle as O
from exmc_amd import _lib, sampler
from test_gpu_leaf_pairs import LANES, _assert_equal, _both, _start
from test_gpu_parity import _dp, _oracle_transitions, es  # noqa: F401  (es: fixture)

pytestmark = pytest.mark.gpu

N_CHAINS = 33
WINDOW = 14                    # EXMC_RNG_WINDOW
LAST_SHIFT = WINDOW - 12       # the state behind the momentum is 11 + shift <= WINDOW - 1


def _extra_words(seed, n_chains, n_draws, d):
    """[chain, draw]: generator words the ten normals of that momentum consumed beyond one each, from
    the generators _start seeds (exo_rng_seed(1000 seed + c))."""
    L = O.lib()
    out = np.zeros((n_chains, n_draws), np.int64)
    for c in range(n_chains):
        r = O.Rng()
        L.exo_rng_seed(C.byref(r), 1000 * seed + c)
        for s in range(n_draws):
            w = O.Rng(r.a, r.b)
            for _ in range(d):
                L.exo_rng_normal(C.byref(r), 1)
            n = 0
            while (w.a, w.b) != (r.a, r.b):
                L.exo_rng_next(C.byref(w))
                n += 1
                assert n < 200
            out[c, s] = n - d
            L.exo_rng_uniform(C.byref(r))
    return out


def _counts(x):
    return dict(Counter(x.ravel().tolist()))


def _waves(x):
    """[wave, group, draw] of the full waves"""
    return x[:32].reshape(8, 4, -1)


def test_shifts_small(es, hip):
    """Shifts 1 and 2, inside the window, one draw past it, and a wave whose groups stand at
    different shifts in the same momentum draw (the per-lane fetch, not the one DPP shift)."""
    x = _extra_words(7, N_CHAINS, 12, es[0].d)
    assert _counts(x) == {0: 331, 1: 34, 2: 28, 3: 3}
    w = _waves(x[:, 1:])   # a call's first momentum has no window
    assert any(len(set(col.tolist()) - {0}) >= 2 for wave in w for col in wave.T)
    o, t, ostate, hstate, _ = _both(es, hip, N_CHAINS, 12, 0.45, 10, 7)
    _assert_equal(o, t, ostate, hstate)


def test_window_overflow(es, hip):
    """400 draws. Of the momenta drawn from a window (every draw of a chain but its first), 770
    end at the last shift the window holds (2) and 97 run past it: the stepping loop entered mid-way,
    after 1 to 4 further words. (A window of 16 words would have 35 at its last shift, 4, and 5 past it.)"""
    x = _extra_words(11, N_CHAINS, 400, es[0].d)
    assert _counts(x) == {0: 11403, 1: 927, 2: 773, 3: 57, 4: 35, 5: 3, 6: 2}
    assert (x[:, 1:] == LAST_SHIFT).sum() == 770 and (x[:, 1:] > LAST_SHIFT).sum() == 97
    assert (x[:, 1:] == 4).sum() == 35 and (x[:, 1:] > 4).sum() == 5
    o, t, ostate, hstate, _ = _both(es, hip, N_CHAINS, 400, 0.45, 10, 11)
    _assert_equal(o, t, ostate, hstate)


def test_no_window_on_entry(es, hip):
    """Three calls of one draw, then one of nine, on the same states and generators: the checker's
    twelve draws, and after every call the state the checker has there."""
    spec, comp, om = es
    x = _extra_words(7, N_CHAINS, 12, spec.d)
    assert (x[:, :4] > 0).any() and (x[:, 4:] > 0).any()   # long-way draws with and without a window
    cfg, q, im, g, logp, rngs = _start(om, spec.d, N_CHAINS, 7)
    hq, hg, hl, hr = q.copy(), g.copy(), logp.copy(), rngs.copy()
    for n_draws in (1, 1, 1, 9):
        t, tr = sampler._host_trace(N_CHAINS, n_draws, spec.d)
        _lib.check(hip.exmc_hip_transitions_host(comp.h, _dp(hq), _dp(hl), _dp(hg),
                                                 hr.ctypes.data_as(C.POINTER(C.c_uint64)), N_CHAINS,
                                                 n_draws, 0.45, _dp(im), 10, LANES, tr))
        o = _oracle_transitions(om, q, logp, g, rngs, n_draws, 0.45, im, 10, cfg)
        _assert_equal(o, t, (q, g, logp, rngs), (hq, hg, hl, hr))


def test_ends_inside_prefix(es, hip):
    """Trees that stop at leaves 1-5: such a group drew fewer of the tree's uniforms and its copy of
    the generator is discarded; the window, and with it the next momentum, does not depend on that."""
    x = _extra_words(7, N_CHAINS, 12, es[0].d)
    o, t, ostate, hstate, _ = _both(es, hip, N_CHAINS, 12, 1.6, 10, 7)
    n = o["n_steps"]
    assert set(n.ravel().tolist()) >= {1, 2, 3, 4, 5}
    assert ((n[:, :-1] <= 5) & (x[:, 1:] > 0)).any()   # ... followed by a momentum with a long-way draw
    _assert_equal(o, t, ostate, hstate)


def test_cap_depth_1(es, hip):
    o, t, ostate, hstate, _ = _both(es, hip, N_CHAINS, 12, 0.45, 1, 7)
    assert (o["n_steps"] == 1).all()
    _assert_equal(o, t, ostate, hstate)
