"""The one-wave sampling kernel of eight_schools at 16 lanes runs doublings 0, 1 and 2 of every
transition as one straight-line unit (exmc_nuts.hpp tree_prefix, M::kTreePrefix): seven leapfrogs
back to back, the tree's own exponentials and logarithms in six lane-batched evaluations, then the
merges in the walk's order with uniforms read ahead. Whole transitions through
exmc_hip_transitions_host against the checker, bit for bit -- every output column and the final
state -- on cases chosen so that the checker's own output shows what each one is there for: trees
that end inside the unit at every leaf while others of the same wave go on past it, divergences at
each of its leaves (which uniform an outer merge takes depends on where its subtree ended), and
depth caps inside, at and one doubling past the unit's end. 33 chains: the last wave has one live
lane group. The seed of `diverged_sixth_leaf` comes from a search with the checker over seeds 1..39
at step size 1.1 (most of them show a diverged tree of six leapfrogs: a divergence in the first leaf
of doubling 2's second pair); seed 12 is the one whose diverged trees end at every leaf 1..7 and
nowhere else.
"""
import numpy as np
import pytest

from test_gpu_leaf_pairs import _assert_equal, _both
from test_gpu_parity import es  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PREFIX = 7   # leapfrogs of doublings 0-2


def _diverged_sizes(o):
    return set(o["n_steps"][o["divergent"] != 0].tolist())


def _ends_inside_and_mixed_waves(o):
    n = o["n_steps"]
    assert set(n.ravel().tolist()) >= {1, 3, 4, 5, 7, 9, 11, 13, 15, 23, 31}
    assert _diverged_sizes(o) >= {1, 4}
    # chains 4w..4w+3 share a wave: in some draw one of them ends before the unit does, another goes past it
    w = n[:32].reshape(8, 4, -1)
    assert ((w < PREFIX).any(axis=1) & (w > PREFIX).any(axis=1)).any()


def _diverging_in_prefix(o):
    assert _diverged_sizes(o) >= {1, 2, 3, 4, 5, 7}
    assert set(o["n_steps"].ravel().tolist()) >= {11, 15, 19}


def _diverging_early(o):
    assert _diverged_sizes(o) == {1, 2, 3, 4, 5}


def _diverged_sixth_leaf(o):
    assert 6 in _diverged_sizes(o)


def _capped_at_prefix(o):
    n = o["n_steps"]
    assert (n <= PREFIX).all() and (n == PREFIX).sum() == 385 and n.size == 396


def _capped_past_prefix(o):
    assert set(o["n_steps"].ravel().tolist()) == {3, 7, 11, 15}


def _no_pair(o):
    assert (o["n_steps"] == 1).all()


def _one_pair(o):
    assert (o["n_steps"] <= 3).all() and (o["n_steps"] == 3).any()


CASES = {
    "ends_inside_mixed_waves": (0.45, 10, 11, _ends_inside_and_mixed_waves),
    "divergences_in_prefix": (1.1, 10, 7, _diverging_in_prefix),
    "divergences_early": (1.6, 10, 7, _diverging_early),
    "diverged_sixth_leaf": (1.1, 10, 12, _diverged_sixth_leaf),
    "cap_at_prefix_end": (0.45, 3, 7, _capped_at_prefix),
    "cap_past_prefix": (0.45, 4, 7, _capped_past_prefix),
    "cap_depth_1": (0.45, 1, 7, _no_pair),
    "cap_depth_2": (0.45, 2, 7, _one_pair),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_tree_prefix_transitions_bit_exact(es, hip, case):
    eps, max_depth, seed, shows = CASES[case]
    o, t, ostate, hstate, _ = _both(es, hip, 33, 12, eps, max_depth, seed)
    shows(o)
    _assert_equal(o, t, ostate, hstate)
