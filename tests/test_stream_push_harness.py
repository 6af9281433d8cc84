"""tests/stream_push.py's comparison without a device: a result assembled from the checker's own rows
passes, and each kind of deviation the GPU tests rely on it to catch is caught."""
import copy

import numpy as np
import pytest

import oracle as O
import stream_push as SP

RUNS = (24, 6)


def _made_from_checker():
    om = O.eight_schools()
    ot, ost, states = SP.reference(om, np.zeros(10), sum(RUNS), 40, 10, 0.3, 1, 16)
    assert 0 < ot["divergent"].sum() < 30
    runs, lo = [], 0
    for n in RUNS:
        cols = {k: ot[k][lo:lo + n].copy() for k in SP.KEYS}
        seen = [(c, {k: cols[k][c - 1].copy() for k in SP.KEYS}) for c in (n // 2, n)]
        runs.append(dict(n=n, cols=cols, divergences=int(cols["divergent"].sum()), progress=n, seen=seen))
        lo += n
    got = dict(epsilon=ost.step_size, inv_mass=np.array(ost.inv_mass[:10]),
               warmup_divergences=ost.divergences - int(ot["divergent"].sum()), runs=runs)
    return got, ot, ost, states


def _next_after(a):
    return np.nextafter(a, np.inf)


def test_comparison_accepts_the_checker_and_catches_each_deviation():
    got, ot, ost, states = _made_from_checker()
    SP.assert_equals_checker(got, ot, ost)
    assert SP.extra_words(states, 10).shape == (30,)

    def broken(change):
        g = copy.deepcopy(got)
        change(g)
        with pytest.raises(AssertionError):
            SP.assert_equals_checker(g, ot, ost)

    def set_(path, f):
        def change(g):
            o = g
            for p in path[:-1]:
                o = o[p]
            o[path[-1]] = f(o[path[-1]])
        return change

    broken(set_(("epsilon",), _next_after))
    broken(lambda g: g["inv_mass"].__setitem__(9, _next_after(g["inv_mass"][9])))
    broken(set_(("warmup_divergences",), lambda v: v + 1))
    for run in (0, 1):                       # one ulp, or one count, in the last row of either run
        for k in SP.KEYS:
            def change(g, run=run, k=k):
                a = g["runs"][run]["cols"][k]
                a[-1] = _next_after(a[-1]) if a.dtype == np.float64 else a[-1] + 1
            broken(change)
        broken(set_(("runs", run, "divergences"), lambda v: v + 1))
        broken(set_(("runs", run, "progress"), lambda v: v - 1))
        broken(set_(("runs", run, "seen"), lambda s: s[::-1]))          # counts must rise
        broken(set_(("runs", run, "seen"), lambda s: s[:1]))            # ... and end at n
        broken(lambda g, run=run: g["runs"][run]["seen"][0][1].__setitem__(     # a row seen before it was final
            "energy", _next_after(g["runs"][run]["seen"][0][1]["energy"])))
    # a second run that restarted from the first run's start instead of continuing
    broken(lambda g: g["runs"][1]["cols"].update({k: ot[k][:6].copy() for k in SP.KEYS}))
