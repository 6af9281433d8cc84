"""exo_sample_rng_states: the checker's cold-start sample/3 with the chain's generator state before
each sampling transition and after the last. Its columns and stats are exo_sample's bit for bit, and
the states follow the main stream of sampler.ex:854-925: d normals (the momentum), then one uniform;
the tree draws from a copy of the generator."""
import ctypes as C

import numpy as np
import pytest

import oracle as O

KEYS = ("draws", "logp", "tree_depth", "n_steps", "divergent", "accept_prob", "energy")
CASES = {
    # name: (model, start, lanes of the kind's sampling layout)
    "eight_schools": (O.eight_schools, [0.0, 0.0] + [0.0] * 8, 16),
    "simple": (O.simple, [0.0, 0.0], 1),
}


@pytest.mark.parametrize("mode_lanes", ["reference", "device"])
@pytest.mark.parametrize("target_accept, max_tree_depth", [(0.8, 10), (0.2, 10), (0.8, 2)])
@pytest.mark.parametrize("name", sorted(CASES))
def test_states_entry_equals_sample_and_walks_the_main_stream(name, target_accept, max_tree_depth, mode_lanes):
    make, q0, lanes = CASES[name]
    m = make()
    cfg = O.Cfg(0, 1) if mode_lanes == "reference" else O.Cfg(1, lanes)
    kw = dict(num_warmup=50, num_samples=40, max_tree_depth=max_tree_depth, target_accept=target_accept,
              seed=7, cfg=cfg)
    for init in (q0, None):           # a given start; the start drawn from the generator
        t0, s0 = O.sample(m, init, **kw)
        t1, s1, states = O.sample_rng_states(m, init, **kw)
        for k in KEYS:
            assert np.array_equal(t0[k], t1[k]), k
        assert s0.step_size == s1.step_size and s0.divergences == s1.divergences
        assert s0.total_leapfrogs == s1.total_leapfrogs
        assert np.array_equal(np.array(s0.inv_mass[:m.d]), np.array(s1.inv_mass[:m.d]))
        assert states.shape == (41, 2) and states.dtype == np.uint64
        L = O.lib()
        for i in range(40):
            r = O.Rng(int(states[i, 0]), int(states[i, 1]))
            for _ in range(m.d):
                L.exo_rng_normal(C.byref(r), cfg.math_mode)
            L.exo_rng_uniform(C.byref(r))
            assert (r.a, r.b) == (int(states[i + 1, 0]), int(states[i + 1, 1])), i
        assert len({(int(a), int(b)) for a, b in states}) == 41
