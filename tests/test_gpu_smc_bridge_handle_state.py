"""Handle state of the bridged SMC entry points (include/exmc_hip_smc_bridge.h: the rules of exmc_hip_smc.h):
the call reads the flat order and nothing else, and leaves the flat order, a dense mass and resident chains
in place. After a bridged call a following sample_chains on the same handle equals a fresh handle's bit for
bit -- plainly, with a flat order set, with a dense mass installed and with resident chains."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_handle_state as HS
from exmc_amd import _lib

pytestmark = pytest.mark.gpu

CFGS = ["es16", "sv64"]
R, N, STAGES = 2, 5, 2


def _opts(cx):
    return _lib.SmcOpts(N, 0.5, 2, 17, STAGES, cx.lanes)


def _base(cx):
    rng = np.random.default_rng(12)
    return np.ascontiguousarray(rng.normal(size=cx.d) * 0.1), np.ascontiguousarray(np.exp(rng.normal(size=cx.d) * 0.1) * 0.5)


def op_bridge(cx, h):
    out = dict(particles=np.zeros((R, N, cx.d)), logp=np.zeros((R, N)), logb=np.zeros((R, N)), betas=np.zeros((R, STAGES)),
               ess_history=np.zeros((R, STAGES)), acceptance_rates=np.zeros((R, STAGES)),
               num_stages=np.zeros(R, np.int32), status=np.zeros(R, np.int32), log_evidence=np.zeros(R),
               log_evidence_steps=np.zeros((R, STAGES)))
    mu, sigma = _base(cx)
    rc = cx.L.exmc_hip_smc_bridge_host(
        h, _opts(cx), R, 1, HS._dp(mu), HS._dp(sigma),
        *[HS._dp(out[k]) for k in ("particles", "logp", "logb", "betas", "ess_history", "acceptance_rates")],
        *[HS._ip(out[k]) for k in ("num_stages", "status")],
        *[HS._dp(out[k]) for k in ("log_evidence", "log_evidence_steps")])
    if rc:
        return {"rc": rc}
    for k in ("betas", "ess_history", "acceptance_rates", "log_evidence_steps"):
        out[k] = np.nan_to_num(out[k], nan=-7.0)   # NaN after num_stages: compare as a value
    return out


def _fresh(cx):
    k = ("smc_bridge", None)
    if k not in cx.fresh:
        with cx.handle() as h:
            cx.fresh[k] = op_bridge(cx, h)
    return cx.fresh[k]


@pytest.mark.parametrize("cfg", CFGS)
def test_sample_chains_after_a_bridged_call_is_a_fresh_handles(cfg, hip):
    cx = HS.ctx(cfg)
    want = _fresh(cx)
    assert "rc" not in want and (want["num_stages"] >= 1).all() and np.isfinite(want["log_evidence"]).all()
    with cx.handle() as h:
        assert HS.same(op_bridge(cx, h), want)
        got = HS.OPS[HS.PROBE](cx, h)
        again = op_bridge(cx, h)                       # and after the sampling call, with its chains resident
    assert HS.same(got, HS.expected(cx, HS.PROBE)), HS.diff(got, HS.expected(cx, HS.PROBE))
    assert HS.same(again, want)


@pytest.mark.parametrize("cfg", CFGS)
def test_flat_order_stays_and_is_read(cfg, hip):
    cx = HS.ctx(cfg)
    p = np.ascontiguousarray(np.random.default_rng(3).permutation(cx.d).astype(np.int32))
    assert not np.array_equal(p, cx.order)
    with cx.handle() as h:
        _lib.check(cx.L.exmc_hip_model_set_flat_order(h, HS._ip(p), cx.d), cx.L)
        want = HS.OPS["sample_host"](cx, h)
    with cx.handle() as h:
        _lib.check(cx.L.exmc_hip_model_set_flat_order(h, HS._ip(p), cx.d), cx.L)
        under_p = op_bridge(cx, h)
        got = HS.OPS["sample_host"](cx, h)
    assert HS.same(got, want), HS.diff(got, want)
    assert not HS.same(under_p, _fresh(cx))            # the call reads the flat order
    assert not np.array_equal(want["draws"], HS.expected(cx, "sample_host")["draws"])


@pytest.mark.parametrize("cfg", CFGS)
def test_dense_mass_stays(cfg, hip):
    cx = HS.ctx(cfg)
    dense = (cx.cov, cx.chol)
    with cx.handle() as h:
        assert "rc" not in HS.OPS["set_dense_mass"](cx, h)
        bridged = op_bridge(cx, h)
        got = HS.OPS[HS.PROBE](cx, h)
    assert HS.same(bridged, _fresh(cx))                # the call does not read the dense mass
    want = HS.expected(cx, HS.PROBE, dense=dense)
    assert HS.same(got, want), HS.diff(got, want)
    assert not HS.same(want, HS.expected(cx, HS.PROBE))


@pytest.mark.parametrize("cfg", CFGS)
def test_resident_chains_continue_across_a_bridged_call(cfg, hip):
    cx = HS.ctx(cfg)

    def run(between):
        with cx.handle() as h:
            _lib.check(cx.L.exmc_hip_chains_init(h, C.byref(cx.tun_s), HS._dp(cx.q0), 1, 0, 1,
                                                 cx.opts(0, 0, 31, cx.lanes)), cx.L)
            trd, tr = cx.dev_trace(cx.ns, 1)
            n1 = cx.ns // 2
            rc, lf1, dv1 = HS._advance(cx, h, n1, 0, trd, tr)
            assert rc == 0
            if between:
                assert HS.same(op_bridge(cx, h), _fresh(cx))
            rc, lf2, dv2 = HS._advance(cx, h, cx.ns - n1, n1, trd, tr)
            assert rc == 0
            return dict(lf=np.array([lf1, lf2]), dv=np.array([dv1, dv2]), **HS._devd(trd))

    assert HS.same(run(True), run(False))


def test_refused_while_a_stream_run_is_in_flight(hip):
    """every entry point that takes the handle answers EXMC_ERR_BADARG between stream_start and
    stream_finish, and works after"""
    cx = HS.ctx("es16")
    with cx.handle() as h:
        tun = _lib.Tuning()
        _lib.check(cx.L.exmc_hip_stream_begin(h, HS._dp(cx.q0), cx.opts(cx.nw, 0, 43, 0), C.byref(tun)), cx.L)
        view, prog = _lib.Trace(), C.POINTER(C.c_int32)()
        _lib.check(cx.L.exmc_hip_stream_start(h, cx.ns, C.byref(view), C.byref(prog)), cx.L)
        try:
            assert op_bridge(cx, h) == {"rc": _lib.ERR_BADARG}
            assert b"in flight" in cx.L.exmc_hip_last_error()
            rc = cx.L.exmc_hip_smc_bridge(h, _opts(cx), R, 1, None, None, *([None] * 10))
            assert rc == _lib.ERR_BADARG and b"in flight" in cx.L.exmc_hip_last_error()
            st = _lib.SmcState()
            assert cx.L.exmc_hip_smc_bridge_init(h, _opts(cx), R, 1, None, None, None, None, None, None, st, None,
                                                 None) == _lib.ERR_BADARG
            assert b"in flight" in cx.L.exmc_hip_last_error()
            assert cx.L.exmc_hip_smc_bridge_mutate(h, _opts(cx), R, None, None, None, None, None, None, st) == _lib.ERR_BADARG
            assert b"in flight" in cx.L.exmc_hip_last_error()
        finally:
            dv = C.c_int32()
            _lib.check(cx.L.exmc_hip_stream_finish(h, C.byref(dv)), cx.L)
        assert HS.same(op_bridge(cx, h), _fresh(cx))
