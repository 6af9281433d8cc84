"""The trace row of eight_schools at 16 lanes a chain is written in two stores: lanes 0..9 of a group
put the draw and lanes 10, 11, 12 accept_prob, logp and energy into one 8-byte store, lanes 13, 14, 15
tree_depth, n_steps and divergent into one 4-byte store; an output the caller left null switches its
lane off (exmc_nuts.hpp nuts_kernel, M::kPackedTrace). Here: exmc_hip_chains_init / _advance with 5
chains (four groups fill wave 0, wave 1 holds one chain and nothing else), 3 draws into rows 2..4 of a
7-row trace and 2 more into rows 5..6, with every set of null outputs the issue names. Every given
array equals the checker's sample_chains bit for bit; the rows not written and a guard band round
every array keep their fill pattern. The same through the row-dense form, which keeps the trait off."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
from exmc_amd import _lib, models, sampler

pytestmark = pytest.mark.gpu

KEYS = ("draws", "logp", "tree_depth", "n_steps", "divergent", "accept_prob", "energy")
NC, ROWS, LANES, NW, SEED = 5, 7, 16, 40, 23
GUARD = 64           # elements of fill pattern in front of and behind every array
FILL_F, FILL_I = -7.25, -77

NULL_SETS = [()] + [(k,) for k in KEYS] + [("logp", "energy"), tuple(k for k in KEYS if k != "draws")]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@functools.lru_cache(maxsize=None)
def _reference(dense):
    """the checker's chains (5 draws each) and the tuning they ran under"""
    m = O.eight_schools()
    spec = models.eight_schools()
    q0 = spec.to_unconstrained(spec.default_init)
    if not dense:
        t, st = O.sample_chains(m, NC, init_q=q0, num_warmup=NW, num_samples=5, seed=SEED, cfg=O.Cfg(1, LANES))
        return t, st, None, None
    st, cov, chol = O.warmup_dense(m, q0, num_warmup=320, seed=SEED, cfg=O.Cfg(1, LANES))
    per = [O.sample_tuned_dense(m, st.step_size, cov, chol, q0, num_samples=5, seed=SEED + 7919 * c,
                                cfg=O.Cfg(1, LANES))[0] for c in range(NC)]
    return {k: np.stack([p[k] for p in per]) for k in KEYS}, st, cov, chol


class _Buffers:
    """7-row device arrays in the trace layout, each inside a guard band, all filled with a pattern"""

    def __init__(self, d, nulls):
        import torch
        dev = torch.device("cuda:0")
        self.shape = {k: (ROWS, d, NC) if k == "draws" else (ROWS, NC) for k in KEYS}
        self.t = {}
        ptr = []
        for k in KEYS:
            if k in nulls:
                ptr.append(None)
                continue
            ints = k in ("tree_depth", "n_steps", "divergent")
            n = int(np.prod(self.shape[k]))
            self.t[k] = torch.full((n + 2 * GUARD,), FILL_I if ints else FILL_F,
                                   dtype=torch.int32 if ints else torch.float64, device=dev)
            ptr.append(self.t[k].data_ptr() + GUARD * self.t[k].element_size())
        self.tr = _lib.Trace(*ptr)

    def host(self, k):
        a = self.t[k].cpu().numpy()
        return a[:GUARD], a[GUARD:-GUARD].reshape(self.shape[k]), a[-GUARD:]


def _check(buf, ref, written):
    """rows in `written` (trace row -> draw of the reference) hold the checker's values, everything else the pattern"""
    for k in buf.t:
        lo, body, hi = buf.host(k)
        fill = FILL_I if body.dtype == np.int32 else FILL_F
        assert np.all(lo == fill) and np.all(hi == fill), k
        for row in range(ROWS):
            if row in written:
                want = ref[k][:, written[row]]               # [chain] or [chain][dim]
                want = want.T if k == "draws" else want      # the device layout is [dim][chain]
                assert np.array_equal(body[row], want), (k, row, body[row], want)
            else:
                assert np.all(body[row] == fill), (k, row)


def _run(hip, dense, nulls):
    import torch
    ref, st, cov, chol = _reference(dense)
    spec = models.eight_schools()
    comp = sampler.compile(spec)
    init = spec.default_init
    opts = dict(num_warmup=320 if dense else NW, num_samples=5, seed=SEED, lanes_per_chain=LANES, dense_mass=dense)
    tuning = sampler.warmup(comp, init, opts)
    assert tuning["epsilon"] == st.step_size
    if dense:
        assert np.array_equal(tuning["cov"], cov) and np.array_equal(tuning["chol_cov"], chol)
    else:
        assert np.array_equal(tuning["inv_mass"], np.array(st.inv_mass[:spec.d]))
    sampler._apply_mass(comp, tuning)
    tun = sampler._tuning_struct(tuning, spec.d)
    iq = np.ascontiguousarray(spec.to_unconstrained(init))
    copts = sampler._c_opts(sampler._merge_opts(dict(num_warmup=0, num_samples=5, seed=SEED, lanes_per_chain=LANES)))
    buf = _Buffers(spec.d, nulls)
    lf, dv = C.c_int64(), C.c_int32()
    comp.check(hip.exmc_hip_chains_init(comp.h, C.byref(tun), _dp(iq), NC, 0, NC, copts))
    comp.check(hip.exmc_hip_chains_advance(comp.h, 3, 2, buf.tr, C.byref(lf), C.byref(dv)))
    torch.cuda.synchronize()
    assert lf.value == int(ref["n_steps"][:, :3].sum()) and dv.value == int(ref["divergent"][:, :3].sum())
    _check(buf, ref, {2: 0, 3: 1, 4: 2})
    # two more draws of the same chains
    comp.check(hip.exmc_hip_chains_advance(comp.h, 2, 5, buf.tr, C.byref(lf), C.byref(dv)))
    torch.cuda.synchronize()
    assert lf.value == int(ref["n_steps"][:, 3:].sum()) and dv.value == int(ref["divergent"][:, 3:].sum())
    _check(buf, ref, {2: 0, 3: 1, 4: 2, 5: 3, 6: 4})


@pytest.mark.parametrize("nulls", NULL_SETS, ids=lambda n: "null:" + ("+".join(n) if n else "none"))
def test_packed_trace_rows_bit_exact(hip, nulls):
    _run(hip, False, nulls)


@pytest.mark.parametrize("nulls", [(), ("logp", "energy")], ids=lambda n: "null:" + ("+".join(n) if n else "none"))
def test_row_dense_form_keeps_its_trace_writes(hip, nulls):
    """opts[:dense_mass]: RowDenseModel sets kPackedTrace back to false; same checks against the dense checker"""
    _run(hip, True, nulls)
