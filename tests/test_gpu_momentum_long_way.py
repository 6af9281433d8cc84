"""The momentum draw of eight_schools at 16 lanes takes its normals from the window of generator words
the previous transition left (exmc_nuts.hpp draw_momentum_window); a word the ziggurat's table test
rejects goes the long way, whose common case -- one wedge test that accepts -- is one straight-line
attempt (exmc_device.hpp normal_wedge_once) and whose other cases fall back to rng_normal_counted.

Which cases a run meets depends on the generator's stream alone, and the stream of a chain is known from
its seed: a momentum is ten normals, the tree draws from a copy, and one uniform ends the transition
(checked below against the kinetic energies the checker's trace implies). So the seeds are searched on
the CPU with the checker's own generator (exo_rng_seed / _next / _normal): a draw's words are counted by
stepping a copy until it meets the state exo_rng_normal left, its layer is bits 7..14 of its first
word. From the second transition of a launch on (the first has no window):
  wedge_first   a word of a layer other than the tail, two words consumed: the wedge accepted at once
  wedge_again   such a word, three or more words: the wedge rejected, the draw started again
  tail          layer 0 and more than one word: the tail's own loop
  two_groups    transitions in which two groups of one wavefront go the long way in the same round
  past_window   draws after which a group's shift exceeds kMaxShift = 2: it leaves for the stepping loop
(counted while the group is still inside the window). Every seed below 200 was classified this way at
8 chains x 40 draws; 26 of the first 60 show all five, the three kept here are rich in the rare ones.
The test asserts the recorded counts on the checker's stream, then compares every output of the launch
with the checker's sample_tuned, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from exmc_amd import _lib, models, sampler

pytestmark = pytest.mark.gpu

D, LANES, K_MAX_SHIFT = 10, 16, 2
KEYS = ("draws", "logp", "tree_depth", "n_steps", "divergent", "accept_prob", "energy")
EPS = 0.3
INV_MASS = np.linspace(0.5, 2.0, D)

# (seed, chains, draws, what the checker's stream shows)
RUNS = [
    (6, 8, 40, dict(wedge_first=27, wedge_again=26, tail=1, two_groups=11, past_window=4)),
    (15, 8, 40, dict(wedge_first=21, wedge_again=17, tail=2, two_groups=4, past_window=5)),
    (43, 8, 40, dict(wedge_first=21, wedge_again=27, tail=2, two_groups=7, past_window=6)),
]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _momentum(L, r):
    """one momentum from generator r: per draw (words consumed, layer of the first word), and the variates"""
    words, z = [], []
    for _ in range(D):
        probe = O.Rng(r.a, r.b)
        idx = (L.exo_rng_next(C.byref(probe)) >> 7) & 255
        z.append(L.exo_rng_normal(C.byref(r), 1))
        n = 1
        while (probe.a, probe.b) != (r.a, r.b):
            L.exo_rng_next(C.byref(probe))
            n += 1
            assert n < 64
        words.append((n, idx))
    return words, z


def _chain_stream(L, seed, n_draws):
    r = O.Rng()
    L.exo_rng_seed(C.byref(r), seed)
    out = []
    for _ in range(n_draws):
        out.append(_momentum(L, r))
        L.exo_rng_next(C.byref(r))   # the uniform that ends the transition; the tree drew from a copy
    return out


def _classify(streams, n_draws):
    nc = len(streams)
    got = dict(wedge_first=0, wedge_again=0, tail=0, two_groups=0, past_window=0)
    for t in range(1, n_draws):
        for w0 in range(0, nc, 64 // LANES):
            long_groups = 0
            for c in range(w0, min(w0 + 64 // LANES, nc)):
                shift, any_long = 0, False
                for j, (n, idx) in enumerate(streams[c][t][0]):
                    if n == 1:
                        continue
                    if shift > K_MAX_SHIFT:
                        break                       # the stepping loop draws the rest
                    any_long = True
                    got["tail" if idx == 0 else "wedge_first" if n == 2 else "wedge_again"] += 1
                    shift += n - 1
                    got["past_window"] += shift > K_MAX_SHIFT and j < D - 1
                long_groups += any_long
            got["two_groups"] += long_groups >= 2
    return got


@pytest.mark.parametrize("seed,nc,nd,shown", RUNS, ids=lambda x: str(x) if isinstance(x, int) else "")
def test_window_draw_long_way_bit_exact(hip, oracle_lib, seed, nc, nd, shown):
    import torch
    m = O.eight_schools()
    spec = models.eight_schools()
    q0 = np.ascontiguousarray(spec.to_unconstrained(spec.default_init))
    cfg = O.Cfg(1, LANES)
    streams = [_chain_stream(oracle_lib, seed + 7919 * c, nd) for c in range(nc)]
    got = _classify(streams, nd)
    assert got == shown and all(v > 0 for v in got.values()), got
    ref = [O.sample_tuned(m, EPS, INV_MASS, q0, num_samples=nd, seed=seed + 7919 * c, cfg=cfg)[0] for c in range(nc)]
    # the stream model itself: the kinetic energy of every transition's momentum, from the variates counted above,
    # is what the checker's trace implies (energy = kinetic - logp of the start point)
    lp0 = m.logp_grad(q0, cfg)[0]
    for c in range(nc):
        prev = np.concatenate([[lp0], ref[c]["logp"][:-1]])
        z = np.array([streams[c][t][1] for t in range(nd)])
        ke = 0.5 * np.sum((z / np.sqrt(INV_MASS)) ** 2 * INV_MASS, axis=1)
        assert np.allclose(ke, ref[c]["energy"] + prev, rtol=1e-12, atol=1e-12), c

    comp = sampler.compile(spec)
    tuning = dict(epsilon=EPS, inv_mass=INV_MASS, chol_cov=None)
    sampler._apply_mass(comp, tuning)
    tun = sampler._tuning_struct(tuning, spec.d)
    dev = torch.device("cuda:0")
    bufs = {k: torch.zeros((nd, spec.d, nc) if k == "draws" else (nd, nc),
                           dtype=torch.int32 if k in ("tree_depth", "n_steps", "divergent") else torch.float64,
                           device=dev) for k in KEYS}
    tr = _lib.Trace(*[bufs[k].data_ptr() for k in KEYS])
    copts = sampler._c_opts(sampler._merge_opts(dict(num_warmup=0, num_samples=nd, seed=seed, lanes_per_chain=LANES)))
    lf, dv = C.c_int64(), C.c_int32()
    comp.check(hip.exmc_hip_chains_init(comp.h, C.byref(tun), _dp(q0), nc, 0, nc, copts))
    comp.check(hip.exmc_hip_chains_advance(comp.h, nd, 0, tr, C.byref(lf), C.byref(dv)))
    torch.cuda.synchronize()
    for k in KEYS:
        a = bufs[k].cpu().numpy()
        for c in range(nc):
            want = ref[c][k]
            have = a[:, :, c] if k == "draws" else a[:, c]
            assert np.array_equal(have, want), (k, c)
    assert lf.value == sum(int(r["n_steps"].sum()) for r in ref)
