"""The compiled lane layouts of the six hand-written kinds, as the C ABI reports them.

For each kind: which lanes_per_chain run a logp_grad launch (every other count from 1 to 64 is
EXMC_ERR_UNSUPPORTED), the three default accessors, which lane counts take a dense warmup, that
the push-style stream and the independent-adaptation form run in the kind's default layout only,
and the flat order the handle starts with (sv, sv_ncp and logistic: the names sorted as strings;
the others: identity). Generated models' layouts are pinned by test_gpu_codegen*.py."""
import ctypes as C

import numpy as np
import pytest

from exmc_amd import _lib, models

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED = _lib.OK, _lib.ERR_UNSUPPORTED
KEYS = ("draws", "logp", "tree_depth", "n_steps", "divergent", "accept_prob", "energy")

# kind: lanes that run, (sampling, warmup, dense) defaults, dense accepted at, dense refused at
LAYOUTS = {
    "eight_schools": ({1, 2, 4, 8, 16}, (16, 16, 1), (1, 16), (8, 2)),
    "simple": ({1}, (1, 1, 1), (1,), (16,)),
    "sv": ({32, 64}, (64, 64, 64), (64,), (1, 32)),
    "sv_ncp": ({64}, (64, 64, 64), (64,), (1, 16)),
    "logistic": ({4, 8, 16, 64}, (16, 64, 16), (16,), (1, 64)),
    "radon": ({32, 64}, (64, 64, 64), (64,), (1, 32)),
}
SORTED_NAMES = {"sv", "sv_ncp", "logistic"}


def _spec(name):
    if name in ("sv", "sv_ncp"):
        return getattr(models, name)(models.sv_returns())
    return getattr(models, name)()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _opts(lanes, num_warmup=10, num_samples=4):
    return _lib.Opts(num_warmup=num_warmup, num_samples=num_samples, max_tree_depth=10,
                     target_accept=0.8, seed=42, lanes_per_chain=lanes)


class Handle:
    def __init__(self, L, spec):
        self.L, self.spec = L, spec
        self.h = C.c_void_p()
        _lib.check(L.exmc_hip_model_create(spec.kind, 0, _dp(spec.data), len(spec.data), 0, C.byref(self.h)), L)
        self.q0 = np.ascontiguousarray(spec.to_unconstrained(spec.default_init))

    def close(self):
        self.L.exmc_hip_model_destroy(self.h)

    def trace(self, n_chains, n):
        d = self.spec.d
        t = {"draws": np.zeros((n_chains, n, d)), "logp": np.zeros((n_chains, n)),
             "accept_prob": np.zeros((n_chains, n)), "energy": np.zeros((n_chains, n)),
             "tree_depth": np.zeros((n_chains, n), np.int32), "n_steps": np.zeros((n_chains, n), np.int32),
             "divergent": np.zeros((n_chains, n), np.int32)}
        return t, _lib.Trace(*[t[k].ctypes.data for k in KEYS])


@pytest.fixture(params=sorted(LAYOUTS))
def kind(request, hip):
    hd = Handle(hip, _spec(request.param))
    yield request.param, hd
    hd.close()


def test_lane_counts_that_run(kind):
    name, hd = kind
    q = np.ascontiguousarray(np.stack([hd.q0, hd.q0 + 0.01]))
    lp, g = np.zeros(2), np.zeros_like(q)
    ran = {lanes for lanes in range(1, 65)
           if hd.L.exmc_hip_logp_grad_host(hd.h, _dp(q), 2, lanes, _dp(lp), _dp(g)) == OK}
    assert ran == LAYOUTS[name][0]
    for lanes in set(range(1, 65)) - ran:
        assert hd.L.exmc_hip_logp_grad_host(hd.h, _dp(q), 2, lanes, _dp(lp), _dp(g)) == UNSUPPORTED


def test_default_accessors(kind):
    name, hd = kind
    got = (hd.L.exmc_hip_model_default_lanes(hd.h), hd.L.exmc_hip_model_default_warmup_lanes(hd.h),
           hd.L.exmc_hip_model_default_dense_lanes(hd.h))
    assert got == LAYOUTS[name][1]


def test_dense_warmup_layouts(kind):
    name, hd = kind
    _, _, accepted, refused = LAYOUTS[name]
    d = hd.spec.d
    for lanes in accepted + refused:
        tun = _lib.Tuning()
        cov, chol = np.zeros((d, d)), np.zeros((d, d))
        rc = hd.L.exmc_hip_warmup_dense(hd.h, _dp(hd.q0), _opts(lanes), C.byref(tun), _dp(cov), _dp(chol))
        assert rc == (OK if lanes in accepted else UNSUPPORTED), (lanes, rc)
        if rc == OK:
            assert tun.epsilon > 0.0
        _lib.check(hd.L.exmc_hip_model_clear_dense_mass(hd.h), hd.L)


def test_stream_and_independent_forms_run_in_the_default_layout(kind):
    name, hd = kind
    L = hd.L
    default = LAYOUTS[name][1][0]
    # the stream is refused at a layout whose one-chain warmup other tests run (stream_begin warms up first)
    others = {"eight_schools": 8, "logistic": 64, "sv": 32, "radon": 32}
    for lanes in (default, others.get(name)):
        if lanes is None:
            continue
        want = OK if lanes == default else UNSUPPORTED
        if lanes == default or name in ("eight_schools", "logistic"):
            tun = _lib.Tuning()
            _lib.check(L.exmc_hip_stream_begin(hd.h, _dp(hd.q0), _opts(lanes), C.byref(tun)), L)
            view, prog = _lib.Trace(), C.POINTER(C.c_int32)()
            rc = L.exmc_hip_stream_start(hd.h, 3, C.byref(view), C.byref(prog))
            if rc == OK:
                div = C.c_int32()
                _lib.check(L.exmc_hip_stream_finish(hd.h, C.byref(div)), L)
            assert rc == want, ("stream", lanes, rc)
        t, tr = hd.trace(2, 4)
        lf, dv = C.c_int64(), C.c_int32()
        rc = L.exmc_hip_sample_independent_host(hd.h, _dp(hd.q0), 2, 0, 2, _opts(lanes), tr, None,
                                                C.byref(lf), C.byref(dv))
        assert rc == want, ("independent", lanes, rc)
        del t


def _warmup(hd, perm=None):
    if perm is not None:
        p = np.ascontiguousarray(perm, dtype=np.int32)
        _lib.check(hd.L.exmc_hip_model_set_flat_order(hd.h, p.ctypes.data_as(C.POINTER(C.c_int32)), len(p)), hd.L)
    tun = _lib.Tuning()
    _lib.check(hd.L.exmc_hip_warmup(hd.h, _dp(hd.q0), _opts(0, num_warmup=30), C.byref(tun)), hd.L)
    return tun.epsilon, np.array(tun.inv_mass[:hd.spec.d])


def test_initial_flat_order(kind, hip):
    name, hd = kind
    names = hd.spec.var_names
    sorted_perm = sorted(range(len(names)), key=lambda i: names[i])
    identity = list(range(len(names)))
    want = sorted_perm if name in SORTED_NAMES else identity
    eps0, im0 = _warmup(hd)
    other = Handle(hip, hd.spec)
    try:
        eps1, im1 = _warmup(other, want)
        assert eps0 == eps1 and np.array_equal(im0, im1)
        if name in SORTED_NAMES:   # the order is visible in the draws: identity gives other bits
            eps2, im2 = _warmup(other, identity)
            assert eps0 != eps2 or not np.array_equal(im0, im2)
    finally:
        other.close()
