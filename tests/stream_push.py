"""The push-style stream (exmc_hip_stream_begin / _start / _finish) driven through the C ABI, and
its comparison with the checker's sample/3. A plain helper module: tests/test_gpu_stream_push.py
uses it; the product never imports it.

nuts_kernel<M, G, LDSL, false, true> is launched by exmc_hip_stream_start only, for the one resident
chain exmc_hip_stream_begin leaves behind. stream_begin resolves lanes_per_chain first, so the
warmup runs in the sampling layout as in sample/3: the reference of a stream of n + k draws is ONE
cold-start run of the checker under O.Cfg(1, lanes), O.sample_rng_states(...)."""
import ctypes as C
import time

import numpy as np

import oracle as O
from exmc_amd import _lib

KEYS = ("draws", "logp", "tree_depth", "n_steps", "divergent", "accept_prob", "energy")
_CTYPE = dict(draws=C.c_double, logp=C.c_double, tree_depth=C.c_int32, n_steps=C.c_int32,
              divergent=C.c_int32, accept_prob=C.c_double, energy=C.c_double)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _push_run(comp, n, timeout_s):
    """One stream_start(n) / stream_finish on the resident chain. The poll of the published count
    is bounded by a deadline and the run is finished on the library side whatever happens."""
    L, d = comp.L, comp.d
    view, prog = _lib.Trace(), C.POINTER(C.c_int32)()
    comp.check(L.exmc_hip_stream_start(comp.h, n, C.byref(view), C.byref(prog)))
    div = C.c_int32(-1)
    seen = []
    try:
        cols = {}
        for k in KEYS:
            w = d if k == "draws" else 1
            a = np.ctypeslib.as_array(C.cast(getattr(view, k), C.POINTER(_CTYPE[k])), shape=(n * w,))
            cols[k] = a.reshape(n, d) if k == "draws" else a
        deadline = time.monotonic() + timeout_s
        last = 0
        while last < n:
            ready = int(prog[0])       # rows [0, ready) are final: the release comes before the count
            if ready > last:
                seen.append((ready, {k: np.array(cols[k][ready - 1]) for k in KEYS}))
                last = ready
            elif time.monotonic() > deadline:
                raise TimeoutError("stream: count %d of %d at the deadline" % (last, n))
    finally:
        rc = L.exmc_hip_stream_finish(comp.h, C.byref(div))
    comp.check(rc)
    return dict(n=n, cols={k: np.array(cols[k]) for k in KEYS}, divergences=int(div.value),
                progress=int(prog[0]), seen=seen)


def run(comp, q0, runs, num_warmup, max_tree_depth, target_accept, seed, lanes=0, timeout_s=120.0):
    """stream_begin from q0, then one stream_start / poll / stream_finish per entry of `runs` on the
    same resident chain. Returns the tuning and, per run, all seven columns (copied from the
    page-locked view after finish), the divergence count, the final progress[0] and every
    (count seen, copy of row count - 1 taken at that moment) pair the poll observed."""
    q0 = np.ascontiguousarray(q0, dtype=np.float64)
    assert q0.shape == (comp.d,)
    tun = _lib.Tuning()
    opts = _lib.Opts(int(num_warmup), int(sum(runs)), int(max_tree_depth), float(target_accept), int(seed),
                     int(lanes))
    comp.check(comp.L.exmc_hip_stream_begin(comp.h, _dp(q0), opts, C.byref(tun)))
    return dict(epsilon=float(tun.epsilon), inv_mass=np.array(tun.inv_mass[:comp.d]),
                warmup_divergences=int(tun.warmup_divergences),
                runs=[_push_run(comp, int(n), timeout_s) for n in runs])


def reference(model, q0, n_draws, num_warmup, max_tree_depth, target_accept, seed, lanes):
    """The checker's cold-start sample/3 of n_draws draws in the sampling layout:
    (trace, stats, generator states [n_draws + 1][2])."""
    return O.sample_rng_states(model, q0, num_warmup=num_warmup, num_samples=n_draws,
                               max_tree_depth=max_tree_depth, target_accept=target_accept, seed=seed,
                               cfg=O.Cfg(1, lanes))


def assert_equals_checker(got, ot, ost):
    """`got` = run(...), (ot, ost) = the checker's trace and stats of sum(runs) draws. Bit for bit."""
    d = got["inv_mass"].size
    total = sum(r["n"] for r in got["runs"])
    assert total == ot["logp"].size
    assert got["epsilon"] == ost.step_size, (got["epsilon"], ost.step_size)
    assert np.array_equal(got["inv_mass"], np.array(ost.inv_mass[:d]))
    # exo_stats.divergences counts warmup and sampling
    assert got["warmup_divergences"] == ost.divergences - int(ot["divergent"].sum())
    lo = 0
    for i, r in enumerate(got["runs"]):
        n = r["n"]
        # the rows of run i continue the chain where run i - 1 left it: position, gradient,
        # log-density and generator as stored at the end of the launch
        for k in KEYS:
            assert np.array_equal(r["cols"][k], ot[k][lo:lo + n]), (i, k, r["cols"][k], ot[k][lo:lo + n])
        # the counters are reset in stream_start: the count is this run's alone
        assert r["divergences"] == int(ot["divergent"][lo:lo + n].sum()), (i, r["divergences"])
        assert r["progress"] == n, (i, r["progress"])
        counts = [c for c, _ in r["seen"]]
        assert counts and counts[-1] == n and all(a < b for a, b in zip(counts, counts[1:])), (i, counts)
        # publication order: a row read when its count appeared is the row after finish
        for c, row in r["seen"]:
            for k in KEYS:
                assert np.array_equal(row[k], r["cols"][k][c - 1]), (i, c, k)
        lo += n


def extra_words(states, d):
    """Per transition: the generator words its d momentum normals took beyond one each, from the
    checker's generator states alone (the main stream: d normals, then one uniform; the tree draws
    from a copy). Asserts that each state leads to the next that way."""
    L = O.lib()
    n = states.shape[0] - 1
    out = np.zeros(n, np.int64)
    for i in range(n):
        r = O.Rng(int(states[i, 0]), int(states[i, 1]))
        w = O.Rng(r.a, r.b)
        for _ in range(d):
            L.exo_rng_normal(C.byref(r), 1)
        k = 0
        while (w.a, w.b) != (r.a, r.b):
            L.exo_rng_next(C.byref(w))
            k += 1
            assert k < 200
        out[i] = k - d
        L.exo_rng_uniform(C.byref(r))
        assert (r.a, r.b) == (int(states[i + 1, 0]), int(states[i + 1, 1])), i
    return out
