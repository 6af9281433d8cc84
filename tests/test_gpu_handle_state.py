"""What one call leaves on a model handle for the next (include/exmc_hip.h, "Handle state").

Every other GPU test makes one kind of call on a fresh handle. Callers keep one handle and make
many different calls on it (the NIF resource of HipSampler.compile, sampler.Compiled, the sharded
API), and the handle holds state between calls: the flat order, an installed dense mass, resident
chains and the buffers behind them. These tests call the library through exmc_amd._lib directly --
not through exmc_amd.sampler, whose clear_dense_mass calls would hide a leak -- and check the
contract the header states:

- pair rule: for every ordered pair (A, B) of the catalogue, B after A on one handle returns what B
  returns on a fresh handle given only the settings the contract says A leaves (a dense mass), bit
  for bit; a probe that reads the dense mass then checks what B left in turn;
- continuation rule: chains_init -> X -> chains_advance and stream_begin -> X -> stream_next either
  continue the resident chains exactly as without X, or return EXMC_ERR_BADARG once X evicted them,
  or continue the chains X itself made resident -- never other draws;
- a flat order set and set back is a fresh handle;
- every op leaves a footprint a leak would show in (a non-diagonal dense mass, a multi_step mass
  that differs from the resident chains', warmups that adapt away from the identity).

Each op of the catalogue is a small call with fixed inputs and returns every output bit (tuning,
all seven trace columns, counters, cov / chol, diagnostics); timings are not outputs."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import gen_models as GM
import oracle as O
from exmc_amd import _lib, models, sampler

pytestmark = pytest.mark.gpu

GOLD_SV = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_traces.npz"))["sv_returns"]
OK, BADARG, UNSUPPORTED = _lib.OK, _lib.ERR_BADARG, _lib.ERR_UNSUPPORTED
KEYS = ("draws", "logp", "tree_depth", "n_steps", "divergent", "accept_prob", "energy")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


# ---- model configurations --------------------------------------------------------------------
# name: (spec factory, lanes of the calls, lanes of the one-chain warmup (0: the library's own form),
#        warmup length, draws, dense warmup length, step size of the tuned runs, step size of transitions)
CONFIGS = {
    "es1": (models.eight_schools, 1, 1, 150, 12, 300, 0.3, 0.4),
    "es16": (models.eight_schools, 16, 16, 150, 12, 300, 0.3, 0.4),
    "sv64": (lambda: models.sv(GOLD_SV), 64, 64, 110, 6, 160, 0.05, 0.08),
    # a generated lane layout (codegen_lanes.py; the model test_gpu_codegen_lanes builds) whose
    # one-chain warmup has a form of its own (lanes 0 -> 64: the chain over the whole wavefront)
    "walk16": (None, 16, 0, 110, 8, 160, 0.2, 0.2),
}
MAX_DEPTH = 6


class Ctx:
    def __init__(self, name):
        make, self.lanes, self.warmup_lanes, self.nw, self.ns, self.nw_dense, eps, eps_t = CONFIGS[name]
        self.name = name
        if make is None:
            from exmc_amd import codegen as cg
            spec = cg.compile_ir(GM.walk_ir(), name="walk16", default_init=GM.WALK_INIT, lanes=16)
            self.L = _lib.bind(spec.lib_path)
        else:
            spec = make()
            self.L = _lib.load()
        self.spec, d = spec, spec.d
        self.d = d
        self.data = np.ascontiguousarray(spec.data, dtype=np.float64)
        self.order = np.ascontiguousarray(spec.flat_order(), dtype=np.int32)
        self.q0 = np.ascontiguousarray(spec.to_unconstrained(spec.default_init))
        with self.handle() as h:
            self.dense_lanes = self.L.exmc_hip_model_default_dense_lanes(h)
        rng = np.random.default_rng(20261016)
        self.lg_q = np.ascontiguousarray(self.q0[None, :] + 0.1 * rng.normal(size=(3, d)))
        # multi_step: a mass that differs from the resident chains' in every entry
        self.ms_q = np.ascontiguousarray(self.lg_q[:2])
        self.ms_p = np.ascontiguousarray(rng.normal(size=(2, d)))
        self.ms_im = np.ascontiguousarray(rng.uniform(1.7, 2.5, size=d))
        self.ms_eps = eps_t / 2
        # the tuning the chains of sample_chains / chains_init run under, and a warm start
        self.tun_s = self._tuning(eps, rng.uniform(0.6, 1.4, size=d))
        self.ws = self._tuning(eps, rng.uniform(0.6, 1.4, size=d))
        # transitions_host from explicit state
        self.t_q = np.ascontiguousarray(self.lg_q[:2])
        self.t_lp, self.t_g = np.zeros(2), np.zeros((2, d))
        with self.handle() as h:
            _lib.check(self.L.exmc_hip_logp_grad_host(h, _dp(self.t_q), 2, self.lanes, _dp(self.t_lp),
                                                      _dp(self.t_g)), self.L)
        self.ms_g = self.t_g.copy()
        self.t_rng = np.zeros((2, 2), dtype=np.uint64)
        for c in range(2):
            r = O.Rng()
            O.lib().exo_rng_seed(C.byref(r), 500 + c)
            self.t_rng[c] = (r.a, r.b)
        self.t_im = np.ascontiguousarray(rng.uniform(0.6, 1.4, size=d))
        self.t_eps = eps_t
        # a fixed non-diagonal SPD dense mass
        A = rng.normal(size=(d, d)) * (0.3 / np.sqrt(d))
        self.cov = np.ascontiguousarray(A @ A.T + 0.7 * np.eye(d))
        self.chol = np.ascontiguousarray(np.linalg.cholesky(self.cov))
        # a device trace [draw][dim][chain] for the diagnostics
        import torch
        self.dev = torch.device("cuda", 0)
        S, Cn = 40, 4
        x = rng.normal(size=(S, d, Cn))
        for s in range(1, S):
            x[s] = 0.6 * x[s - 1] + x[s]
        self.diag_trace = torch.tensor(x, dtype=torch.float64, device=self.dev)
        self.diag_shape = (S, Cn)
        torch.cuda.synchronize()
        self.fresh = {}

    def _tuning(self, eps, im):
        t = _lib.Tuning()
        t.epsilon = float(eps)
        for i in range(self.d):
            t.inv_mass[i] = float(im[i])
        return t

    @contextlib.contextmanager
    def handle(self):
        h = C.c_void_p()
        _lib.check(self.L.exmc_hip_model_create(self.spec.kind, self.d, _dp(self.data), int(self.data.size), 0,
                                                C.byref(h)), self.L)
        try:
            _lib.check(self.L.exmc_hip_model_set_flat_order(h, _ip(self.order), self.d), self.L)
            yield h
        finally:
            self.L.exmc_hip_model_destroy(h)

    def opts(self, nw, ns, seed, lanes):
        return _lib.Opts(nw, ns, MAX_DEPTH, 0.8, seed, lanes)

    def dev_trace(self, rows, chains):
        import torch
        f64, i32 = torch.float64, torch.int32
        t = dict(draws=torch.zeros((rows, self.d, chains), dtype=f64, device=self.dev))
        for k, dt in (("logp", f64), ("tree_depth", i32), ("n_steps", i32), ("divergent", i32),
                      ("accept_prob", f64), ("energy", f64)):
            t[k] = torch.zeros((rows, chains), dtype=dt, device=self.dev)
        torch.cuda.synchronize()     # (the library writes on a stream of its own)
        return t, _lib.Trace(*[t[k].data_ptr() for k in KEYS])


_ctx = {}


def ctx(name):
    if name not in _ctx:
        _ctx[name] = Ctx(name)
    return _ctx[name]


def _out(rc, **kw):
    return {"rc": rc} if rc != OK else kw


def _tun(cx, t):
    return dict(eps=np.float64(t.epsilon), inv_mass=np.array(t.inv_mass[:cx.d]),
                wdiv=np.int64(t.warmup_divergences))


def _host(cx, t, prefix=""):
    return {prefix + k: t[k] for k in KEYS}


def _devd(t, prefix=""):
    return {prefix + k: t[k].cpu().numpy() for k in KEYS}


# ---- the catalogue ---------------------------------------------------------------------------
def op_logp_grad(cx, h):
    lp, g = np.zeros(3), np.zeros((3, cx.d))
    rc = cx.L.exmc_hip_logp_grad_host(h, _dp(cx.lg_q), 3, cx.lanes, _dp(lp), _dp(g))
    return _out(rc, logp=lp, grad=g)


def op_multi_step(cx, h):
    n = 4
    aq, ap, ag = (np.zeros((2, n, cx.d)) for _ in range(3))
    al = np.zeros((2, n))
    rc = cx.L.exmc_hip_multi_step_host(h, _dp(cx.ms_q), _dp(cx.ms_p), _dp(cx.ms_g), cx.ms_eps, _dp(cx.ms_im), n, 2,
                                       cx.lanes, _dp(aq), _dp(ap), _dp(al), _dp(ag))
    return _out(rc, all_q=aq, all_p=ap, all_logp=al, all_g=ag)


def op_transitions(cx, h):
    q, lp, g, r = cx.t_q.copy(), cx.t_lp.copy(), cx.t_g.copy(), cx.t_rng.copy()
    t, tr = sampler._host_trace(2, 3, cx.d)
    rc = cx.L.exmc_hip_transitions_host(h, _dp(q), _dp(lp), _dp(g), r.ctypes.data_as(C.POINTER(C.c_uint64)), 2, 3,
                                        cx.t_eps, _dp(cx.t_im), MAX_DEPTH, cx.lanes, tr)
    return _out(rc, state_q=q, state_logp=lp, state_grad=g, state_rng=r, **_host(cx, t))


def _warmup(cx, h, seed):
    tun = _lib.Tuning()
    rc = cx.L.exmc_hip_warmup(h, _dp(cx.q0), cx.opts(cx.nw, 0, seed, cx.warmup_lanes), C.byref(tun))
    return _out(rc, **_tun(cx, tun))


def op_warmup(cx, h):
    return _warmup(cx, h, 11)


def op_warmup_host(cx, h):
    """the host-driven form: one launch per transition through the sampling kernel"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("EXMC_HIP_HOST_WARMUP", "1")
        return _warmup(cx, h, 11)


def op_warmup_from(cx, h):
    tun = _lib.Tuning()
    rc = cx.L.exmc_hip_warmup_from(h, _dp(cx.q0), cx.opts(cx.nw, 0, 12, cx.warmup_lanes), C.byref(cx.ws),
                                   C.byref(tun))
    return _out(rc, **_tun(cx, tun))


def op_warmup_dense(cx, h):
    tun, cov, chol = _lib.Tuning(), np.zeros((cx.d, cx.d)), np.zeros((cx.d, cx.d))
    rc = cx.L.exmc_hip_warmup_dense(h, _dp(cx.q0), cx.opts(cx.nw_dense, 0, 13, cx.dense_lanes), C.byref(tun),
                                    _dp(cov), _dp(chol))
    return _out(rc, cov=cov, chol=chol, **_tun(cx, tun))


def op_set_dense_mass(cx, h):
    return _out(cx.L.exmc_hip_model_set_dense_mass(h, _dp(cx.cov), _dp(cx.chol), cx.d))


def op_clear_dense_mass(cx, h):
    return _out(cx.L.exmc_hip_model_clear_dense_mass(h))


def op_sample_host(cx, h):
    t, tr = sampler._host_trace(1, cx.ns, cx.d)
    tun, dv = _lib.Tuning(), C.c_int32()
    rc = cx.L.exmc_hip_sample_host(h, _dp(cx.q0), cx.opts(cx.nw, cx.ns, 17, cx.lanes), tr, C.byref(tun),
                                   C.byref(dv))
    return _out(rc, div=np.int32(dv.value), **_tun(cx, tun), **_host(cx, t))


def op_sample_warm_host(cx, h):
    t, tr = sampler._host_trace(1, cx.ns, cx.d)
    tun, dv = _lib.Tuning(), C.c_int32()
    rc = cx.L.exmc_hip_sample_warm_host(h, _dp(cx.q0), cx.opts(cx.nw, cx.ns, 19, cx.lanes), C.byref(cx.ws), tr,
                                        C.byref(tun), C.byref(dv))
    return _out(rc, div=np.int32(dv.value), **_tun(cx, tun), **_host(cx, t))


def op_sample_dense_host(cx, h):
    t, tr = sampler._host_trace(1, cx.ns, cx.d)
    tun, dv = _lib.Tuning(), C.c_int32()
    cov, chol = np.zeros((cx.d, cx.d)), np.zeros((cx.d, cx.d))
    rc = cx.L.exmc_hip_sample_dense_host(h, _dp(cx.q0), cx.opts(cx.nw_dense, cx.ns, 23, cx.dense_lanes), tr,
                                         C.byref(tun), _dp(cov), _dp(chol), C.byref(dv))
    return _out(rc, cov=cov, chol=chol, div=np.int32(dv.value), **_tun(cx, tun), **_host(cx, t))


def op_sample_chains_host(cx, h):
    t, tr = sampler._host_trace(3, cx.ns, cx.d)
    lf, dv = C.c_int64(), C.c_int32()
    rc = cx.L.exmc_hip_sample_chains_host(h, C.byref(cx.tun_s), _dp(cx.q0), 3, 0, 3, cx.opts(0, cx.ns, 29, cx.lanes),
                                          tr, C.byref(lf), C.byref(dv))
    return _out(rc, lf=np.int64(lf.value), div=np.int32(dv.value), **_host(cx, t))


def _advance(cx, h, n, off, trd, tr):
    lf, dv = C.c_int64(), C.c_int32()
    rc = cx.L.exmc_hip_chains_advance(h, n, off, tr, C.byref(lf), C.byref(dv))
    return rc, np.int64(lf.value), np.int32(dv.value)


def op_chains(cx, h):
    """chains_init of ONE chain (what a one-chain stream's resident state looks like) + two advances
    into a device trace"""
    rc = cx.L.exmc_hip_chains_init(h, C.byref(cx.tun_s), _dp(cx.q0), 1, 0, 1, cx.opts(0, 0, 31, cx.lanes))
    if rc:
        return _out(rc)
    trd, tr = cx.dev_trace(cx.ns, 1)
    n1 = cx.ns // 2
    rc, lf1, dv1 = _advance(cx, h, n1, 0, trd, tr)
    if rc:
        return _out(rc)
    rc, lf2, dv2 = _advance(cx, h, cx.ns - n1, n1, trd, tr)
    return _out(rc, lf1=lf1, dv1=dv1, lf2=lf2, dv2=dv2, **_devd(trd))


def op_sample_independent(cx, h):
    t, tr = sampler._host_trace(3, cx.ns, cx.d)
    tune = np.zeros((3, 3 + cx.d))
    lf, dv = C.c_int64(), C.c_int32()
    rc = cx.L.exmc_hip_sample_independent_host(h, _dp(cx.q0), 3, 0, 3, cx.opts(cx.nw, cx.ns, 37, 0), tr, _dp(tune),
                                               C.byref(lf), C.byref(dv))
    return _out(rc, tune=tune, lf=np.int64(lf.value), div=np.int32(dv.value), **_host(cx, t))


def _next(cx, h, n, prefix):
    t, tr = sampler._host_trace(1, n, cx.d)
    dv = C.c_int32()
    rc = cx.L.exmc_hip_stream_next_host(h, n, tr, C.byref(dv))
    return rc, dict({prefix + "div": np.int32(dv.value)}, **_host(cx, t, prefix))


def op_stream(cx, h):
    tun = _lib.Tuning()
    rc = cx.L.exmc_hip_stream_begin(h, _dp(cx.q0), cx.opts(cx.nw, 0, 41, cx.lanes), C.byref(tun))
    if rc:
        return _out(rc)
    out = _tun(cx, tun)
    n1 = cx.ns // 2
    for n, pre in ((n1, "a_"), (cx.ns - n1, "b_")):
        rc, o = _next(cx, h, n, pre)
        if rc:
            return _out(rc)
        out.update(o)
    return out


def op_stream_push(cx, h):
    """stream_begin + stream_start / stream_finish (the push form runs in the kind's default layout)"""
    tun = _lib.Tuning()
    rc = cx.L.exmc_hip_stream_begin(h, _dp(cx.q0), cx.opts(cx.nw, 0, 43, 0), C.byref(tun))
    if rc:
        return _out(rc)
    n = cx.ns
    view, prog = _lib.Trace(), C.POINTER(C.c_int32)()
    rc = cx.L.exmc_hip_stream_start(h, n, C.byref(view), C.byref(prog))
    if rc:
        return _out(rc)
    dv = C.c_int32()
    rc = cx.L.exmc_hip_stream_finish(h, C.byref(dv))
    if rc:
        return _out(rc)

    def col(ptr, ct, w=1):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(n * w,)).copy()
    return dict(_tun(cx, tun), progress=np.int32(prog[0]), div=np.int32(dv.value),
                draws=col(view.draws, C.c_double, cx.d), logp=col(view.logp, C.c_double),
                tree_depth=col(view.tree_depth, C.c_int32), n_steps=col(view.n_steps, C.c_int32),
                divergent=col(view.divergent, C.c_int32), accept_prob=col(view.accept_prob, C.c_double),
                energy=col(view.energy, C.c_double))


def _diag(fn, per_chain):
    def op(cx, h):
        import torch
        S, Cn = cx.diag_shape
        out = torch.zeros((cx.d, Cn) if per_chain else (cx.d,), dtype=torch.float64, device=cx.dev)
        torch.cuda.synchronize()
        rc = getattr(cx.L, fn)(h, cx.diag_trace.data_ptr(), S, cx.d, Cn, out.data_ptr())
        torch.cuda.synchronize()
        return _out(rc, out=out.cpu().numpy())
    return op


OPS = {
    "logp_grad": op_logp_grad,
    "multi_step": op_multi_step,
    "transitions": op_transitions,
    "warmup": op_warmup,
    "warmup_host": op_warmup_host,
    "warmup_from": op_warmup_from,
    "warmup_dense": op_warmup_dense,
    "set_dense_mass": op_set_dense_mass,
    "clear_dense_mass": op_clear_dense_mass,
    "sample_host": op_sample_host,
    "sample_warm_host": op_sample_warm_host,
    "sample_dense_host": op_sample_dense_host,
    "sample_chains_host": op_sample_chains_host,
    "chains": op_chains,
    "sample_independent": op_sample_independent,
    "stream": op_stream,
    "stream_push": op_stream_push,
    "ess": _diag("exmc_hip_ess", True),
    "ess_bulk": _diag("exmc_hip_ess_bulk", True),
    "rhat": _diag("exmc_hip_rhat", False),
}

# The C entry points each op calls (the CPU guard, test_handle_state_catalogue.py, checks that every
# entry point taking a model handle is here or exempt).
ENTRY_POINTS = {
    "logp_grad": ["exmc_hip_logp_grad_host"],
    "multi_step": ["exmc_hip_multi_step_host"],
    "transitions": ["exmc_hip_transitions_host"],
    "warmup": ["exmc_hip_warmup"],
    "warmup_host": ["exmc_hip_warmup"],
    "warmup_from": ["exmc_hip_warmup_from"],
    "warmup_dense": ["exmc_hip_warmup_dense"],
    "set_dense_mass": ["exmc_hip_model_set_dense_mass"],
    "clear_dense_mass": ["exmc_hip_model_clear_dense_mass"],
    "sample_host": ["exmc_hip_sample_host"],
    "sample_warm_host": ["exmc_hip_sample_warm_host"],
    "sample_dense_host": ["exmc_hip_sample_dense_host"],
    "sample_chains_host": ["exmc_hip_sample_chains_host"],
    "chains": ["exmc_hip_chains_init", "exmc_hip_chains_advance"],
    "sample_independent": ["exmc_hip_sample_independent_host"],
    "stream": ["exmc_hip_stream_begin", "exmc_hip_stream_next_host"],
    "stream_push": ["exmc_hip_stream_begin", "exmc_hip_stream_start", "exmc_hip_stream_finish"],
    "ess": ["exmc_hip_ess"],
    "ess_bulk": ["exmc_hip_ess_bulk"],
    "rhat": ["exmc_hip_rhat"],
}
EXEMPT = {
    "exmc_hip_model_create": "makes the handle",
    "exmc_hip_model_destroy": "ends the handle",
    "exmc_hip_model_set_flat_order": "the flat order has a test of its own (test_flat_order_set_and_reset)",
    "exmc_hip_model_dim": "accessor of a creation constant",
    "exmc_hip_model_default_lanes": "accessor of a creation constant",
    "exmc_hip_model_default_warmup_lanes": "accessor of a creation constant",
    "exmc_hip_model_default_dense_lanes": "accessor of a creation constant",
    "exmc_hip_model_stream": "accessor of the handle's HIP stream",
    "exmc_hip_last_kernel_ms": "a timing, not an output",
    "exmc_hip_multi_step": "the device form exmc_hip_multi_step_host runs through (catalogue: multi_step)",
    "exmc_hip_sample_chains": "the device form exmc_hip_sample_chains_host runs through; itself chains_init + "
                              "chains_advance (catalogue: sample_chains_host, chains)",
    "exmc_hip_sample_independent": "the device form exmc_hip_sample_independent_host runs through "
                                   "(catalogue: sample_independent)",
}

# What the contract says each op leaves (include/exmc_hip.h, "Handle state").
SETS_DENSE = {"set_dense_mass", "warmup_dense", "sample_dense_host"}
CLEARS_DENSE = {"warmup", "warmup_host", "warmup_from", "clear_dense_mass", "sample_host", "sample_warm_host",
                "sample_independent", "stream", "stream_push"}
READS_DENSE = {"sample_chains_host", "chains"}
# ops whose outputs the resident chains cannot change and which leave those chains in place
NEUTRAL = {"logp_grad", "multi_step", "ess", "ess_bulk", "rhat"}
OWN_CHAINS = {"sample_chains_host", "chains"}     # leave chains of their own for chains_advance
OWN_STREAM = {"stream", "stream_push"}            # leave a stream of their own for stream_next
PROBE = "sample_chains_host"


def leaves(cx, name, out, dense):
    """the dense mass (cov, chol) or None the contract says the handle carries after op `name`"""
    if "rc" in out:
        return dense     # a refused call changes nothing
    if name == "set_dense_mass":
        return (cx.cov, cx.chol)
    if name in SETS_DENSE:
        return (out["cov"], out["chol"])
    if name in CLEARS_DENSE:
        return None
    return dense


def _key(dense):
    return None if dense is None else (dense[0].tobytes(), dense[1].tobytes())


def expected(cx, name, dense=None):
    """op `name` on a fresh handle given only the dense mass `dense` (when the op reads one)"""
    if name not in READS_DENSE:
        dense = None
    k = (name, _key(dense))
    if k not in cx.fresh:
        with cx.handle() as h:
            if dense is not None:
                _lib.check(cx.L.exmc_hip_model_set_dense_mass(h, _dp(dense[0]), _dp(dense[1]), cx.d), cx.L)
            cx.fresh[k] = OPS[name](cx, h)
    return cx.fresh[k]


def same(a, b):
    if a.keys() != b.keys():
        return False
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def diff(a, b):
    if "rc" in a or "rc" in b:
        return "rc %s vs %s" % (a.get("rc", OK), b.get("rc", OK))
    return "differs in " + ", ".join(k for k in a if k in b and np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes())


# refusals the catalogue may meet, by op and config: the generated lane layout has no dense form
def refusal_ok(cx, name, out):
    if "rc" not in out:
        return True
    return out["rc"] == UNSUPPORTED and cx.name == "walk16" and (name in SETS_DENSE or name in READS_DENSE)


# ---- footprints: each op shows what a leak would change ------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_footprints(cfg, hip):
    cx = ctx(cfg)
    assert np.abs(cx.cov - np.diag(np.diag(cx.cov))).max() > 0.01
    assert np.all(cx.ms_im > np.array(cx.tun_s.inv_mass[:cx.d]) + 0.2)     # multi_step's mass is not the chains'
    for name in OPS:
        out = expected(cx, name)
        assert refusal_ok(cx, name, out), (name, out)
        assert same(out, expected(cx, name)), name
    for name in ("warmup", "warmup_host", "sample_host"):        # adapted away from the identity
        assert not np.all(expected(cx, name)["inv_mass"] == 1.0), name
    for name in ("warmup_from", "sample_warm_host"):             # (from the non-identity warm start)
        assert not np.all(expected(cx, name)["inv_mass"] == 1.0), name
    # the probe reads a dense mass: a leak would change its draws
    probe, probe_dense = expected(cx, PROBE), expected(cx, PROBE, (cx.cov, cx.chol))
    if cx.name == "walk16":     # (the generated 16-lane layout refuses a dense mass: a leak shows as the refusal)
        assert probe_dense == {"rc": UNSUPPORTED} and "rc" not in probe
    else:
        assert not np.array_equal(probe["draws"], probe_dense["draws"])
    for name in ("warmup_dense", "sample_dense_host"):      # (in the kind's dense layout)
        cov = expected(cx, name)["cov"]
        assert np.abs(cov - np.diag(np.diag(cov))).max() > 0, name
    # the multi_step mass would change the resident chains' draws
    with cx.handle() as h:
        tun = cx._tuning(cx.tun_s.epsilon, cx.ms_im)
        t, tr = sampler._host_trace(3, cx.ns, cx.d)
        lf, dv = C.c_int64(), C.c_int32()
        _lib.check(cx.L.exmc_hip_sample_chains_host(h, C.byref(tun), _dp(cx.q0), 3, 0, 3, cx.opts(0, cx.ns, 29, cx.lanes),
                                                    tr, C.byref(lf), C.byref(dv)), cx.L)
    assert not np.array_equal(t["draws"], probe["draws"])


# ---- pair rule -----------------------------------------------------------------------------------
@pytest.mark.parametrize("a", list(OPS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_pair_rule(cfg, a, hip):
    """A on a new handle, then every B, then the probe: B (and the probe) equal a fresh handle given
    only the dense mass the contract says A (A then B) leaves."""
    cx = ctx(cfg)
    bad = []
    for b in OPS:
        with cx.handle() as h:
            out_a = OPS[a](cx, h)
            assert same(out_a, expected(cx, a)), (a, diff(out_a, expected(cx, a)))
            dense = leaves(cx, a, out_a, None)
            out_b = OPS[b](cx, h)
            if not same(out_b, expected(cx, b, dense)):
                bad.append("%s -> %s: %s" % (a, b, diff(out_b, expected(cx, b, dense))))
            dense = leaves(cx, b, out_b, dense)
            out_p = OPS[PROBE](cx, h)
            if not same(out_p, expected(cx, PROBE, dense)):
                bad.append("%s -> %s -> %s (probe): %s" % (a, b, PROBE, diff(out_p, expected(cx, PROBE, dense))))
    assert not bad, "\n".join(bad)


# ---- continuation rule ---------------------------------------------------------------------------
def _chains_run(cx, h, x, dense):
    """[set_dense_mass ->] chains_init (3 chains) -> advance -> X -> advance; the second advance's rows"""
    if dense:
        _lib.check(cx.L.exmc_hip_model_set_dense_mass(h, _dp(cx.cov), _dp(cx.chol), cx.d), cx.L)
    _lib.check(cx.L.exmc_hip_chains_init(h, C.byref(cx.tun_s), _dp(cx.q0), 3, 0, 3, cx.opts(0, 0, 47, cx.lanes)),
               cx.L)
    n1 = cx.ns // 2
    trd, tr = cx.dev_trace(cx.ns, 3)
    rc, _, _ = _advance(cx, h, n1, 0, trd, tr)
    _lib.check(rc, cx.L)
    out_x = OPS[x](cx, h) if x is not None else {}
    assert refusal_ok(cx, x, out_x), (x, out_x)
    return out_x, _continue_chains(cx, h)


def _continue_chains(cx, h):
    n2 = cx.ns - cx.ns // 2
    trd, tr = cx.dev_trace(n2, 3)
    rc, lf, dv = _advance(cx, h, n2, 0, trd, tr)
    return _out(rc, lf=lf, dv=dv, **_devd(trd))


def _stream_run(cx, h, x):
    tun = _lib.Tuning()
    _lib.check(cx.L.exmc_hip_stream_begin(h, _dp(cx.q0), cx.opts(cx.nw, 0, 53, cx.lanes), C.byref(tun)), cx.L)
    rc, _ = _next(cx, h, cx.ns // 2, "")
    _lib.check(rc, cx.L)
    out_x = OPS[x](cx, h) if x is not None else {}
    assert refusal_ok(cx, x, out_x), (x, out_x)
    return out_x, _continue_stream(cx, h)


def _continue_stream(cx, h):
    rc, o = _next(cx, h, cx.ns - cx.ns // 2, "")
    return _out(rc, **o)


@pytest.mark.parametrize("x", list(OPS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_continuation_rule(cfg, x, hip):
    """chains_init -> X -> chains_advance and stream_begin -> X -> stream_next: the uninterrupted
    continuation when X leaves the resident chains alone, EXMC_ERR_BADARG when X evicted them, the
    continuation of X's own chains when X made chains of its own resident -- nothing else."""
    cx = ctx(cfg)
    variants = [("chains", False), ("stream", False)]
    if cx.name != "walk16":
        variants.append(("chains", True))      # chains under an installed dense mass
    for kind, dense in variants:
        run = (lambda h, x_: _chains_run(cx, h, x_, dense)) if kind == "chains" else (lambda h, x_: _stream_run(cx, h, x_))
        with cx.handle() as h:
            out_x, got = run(h, x)
        own = OWN_CHAINS if kind == "chains" else OWN_STREAM
        if x in NEUTRAL or (x == "clear_dense_mass" and not dense) or "rc" in out_x:
            with cx.handle() as h:
                want = run(h, None)[1]                      # the uninterrupted sequence (a refused X changes nothing)
            assert "rc" not in want
        elif x in own:
            with cx.handle() as h:                          # X's own chains, continued
                if dense:
                    _lib.check(cx.L.exmc_hip_model_set_dense_mass(h, _dp(cx.cov), _dp(cx.chol), cx.d), cx.L)
                OPS[x](cx, h)
                want = _continue_chains(cx, h) if kind == "chains" else _continue_stream(cx, h)
            assert "rc" not in want
        else:
            want = {"rc": BADARG}                           # X evicted the resident chains
        assert same(got, want), (kind, "dense" if dense else "diagonal", x, diff(got, want))


# ---- flat order ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["es16", "sv64"])
def test_flat_order_set_and_reset(cfg, hip):
    """set_flat_order(p) then set_flat_order(default) is a fresh handle for every op; under p the
    RNG-consuming ops differ (the setting has a footprint)."""
    cx = ctx(cfg)
    p = np.ascontiguousarray(np.random.default_rng(3).permutation(cx.d).astype(np.int32))
    assert not np.array_equal(p, cx.order)
    with cx.handle() as h:
        _lib.check(cx.L.exmc_hip_model_set_flat_order(h, _ip(p), cx.d), cx.L)
        under_p = OPS["sample_host"](cx, h)
    assert not np.array_equal(under_p["draws"], expected(cx, "sample_host")["draws"])
    bad = []
    for name in OPS:
        with cx.handle() as h:
            _lib.check(cx.L.exmc_hip_model_set_flat_order(h, _ip(p), cx.d), cx.L)
            OPS["sample_host"](cx, h)
            _lib.check(cx.L.exmc_hip_model_set_flat_order(h, _ip(cx.order), cx.d), cx.L)
            out = OPS[name](cx, h)
        if not same(out, expected(cx, name)):
            bad.append("%s: %s" % (name, diff(out, expected(cx, name))))
    assert not bad, "\n".join(bad)


# ---- the Python layer: one Compiled, many calls ----------------------------------------------------
def _py_sequence():
    spec = models.eight_schools()
    init = spec.default_init
    o = dict(num_warmup=150, num_samples=12, seed=61, max_tree_depth=MAX_DEPTH, lanes_per_chain=16)
    od = dict(o, num_warmup=300, dense_mass=True, seed=62)

    def sample_dense(c):
        _, st = sampler.sample(c, init, od)
        return dict(st["raw"], cov=st["cov"], chol=st["chol_cov"], eps=st["step_size"])

    def tuned_dense(c):
        tun = sampler.warmup(c, init, od)
        _, _, ex = sampler.sample_compiled_tuned(c, tun, init, o, num_chains=3)
        return dict(ex["raw"], cov=tun["cov"], eps=tun["epsilon"])

    def sample_diag(c):
        _, st = sampler.sample(c, init, dict(o, seed=63))
        return dict(st["raw"], eps=st["step_size"], im=st["inv_mass_diag"])

    def tuned_diag(c):
        tun = sampler.warmup(c, init, dict(o, seed=64))
        _, _, ex = sampler.sample_compiled_tuned(c, tun, init, dict(o, seed=64), num_chains=3)
        return dict(ex["raw"], eps=tun["epsilon"], im=tun["inv_mass"])

    def chains(c):
        _, st = sampler.sample_chains(c, 3, dict(o, seed=65, init_values=init))
        return dict(st[0]["extra"]["raw"], eps=st[0]["step_size"])

    def stream(push):
        def run(c):
            msgs = []
            sampler.sample_stream(c, msgs.append, init, dict(o, seed=66, stream_chunk=5, stream_push=push))
            rows = [m for m in msgs if m[0] == "exmc_sample"]
            return dict(q=np.array([[m[2][n] for n in spec.var_names] for m in rows]),
                        e=np.array([m[3]["energy"] for m in rows]), n=np.array([m[3]["n_steps"] for m in rows]))
        return run

    def independent(c):
        _, st = sampler.sample_chains(c, 3, dict(o, seed=67, vectorized=False, init_values=init))
        return dict(st[0]["extra"]["raw"], tune=st[0]["extra"]["tuning"])

    return spec, [("sample dense", sample_dense), ("tuned dense", tuned_dense), ("sample", sample_diag),
                  ("tuned", tuned_diag), ("sample_chains", chains), ("stream", stream(False)),
                  ("stream push", stream(True)), ("independent", independent), ("sample dense again", sample_dense),
                  ("sample_chains after dense", chains)]


def test_python_calls_on_one_compiled_equal_fresh_compileds(hip):
    """sampler.sample (dense and diagonal), sample_compiled_tuned (dense and diagonal tunings),
    sample_chains, sample_stream (pull and push) and independent chains one after the other on ONE
    Compiled give what each gives on a Compiled of its own."""
    spec, seq = _py_sequence()
    one = sampler.compile(spec)
    try:
        for name, fn in seq:
            got = fn(one)
            fresh = sampler.compile(spec)
            try:
                want = fn(fresh)
            finally:
                fresh.close()
            assert got.keys() == want.keys()
            for k in got:
                assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (name, k)
    finally:
        one.close()
