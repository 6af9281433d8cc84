"""Handle state of the convergence diagnostics (include/exmc_hip_convergence.h "Handle state"): the call
reads none and changes none. A sampling run after a call equals one on a fresh handle (the flat order is
read by it); an installed dense mass and resident chains survive the call; a handle with a stream run in
flight refuses it."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_handle_state as HS
from exmc_amd import _lib

pytestmark = pytest.mark.gpu

CFGS = ["es16", "sv64"]


def op_conv(cx, h):
    Cn, S = 3, 10
    x = np.ascontiguousarray(cx.q0[None, None, :] + 0.25 * np.random.default_rng(77).normal(size=(Cn, S, cx.d)))
    out = np.zeros((6, cx.d))
    rc = cx.L.exmc_hip_convergence_host(h, HS._dp(x), S, cx.d, Cn, 0, HS._dp(out))
    return {"rc": rc} if rc else dict(out=out)


def _fresh(cx):
    k = ("convergence", None)
    if k not in cx.fresh:
        with cx.handle() as h:
            cx.fresh[k] = op_conv(cx, h)
    return cx.fresh[k]


@pytest.mark.parametrize("cfg", CFGS)
def test_sampling_after_a_call_equals_a_fresh_handle(cfg, hip):
    cx = HS.ctx(cfg)
    want_conv = _fresh(cx)
    assert "rc" not in want_conv
    with cx.handle() as h:
        want = HS.op_sample_host(cx, h)
    with cx.handle() as h:
        assert HS.same(op_conv(cx, h), want_conv)
        got = HS.op_sample_host(cx, h)
        # ... and the call after the sampling run equals its fresh-handle result
        assert HS.same(op_conv(cx, h), want_conv)
    assert "rc" not in want and HS.same(got, want), HS.diff(got, want)


@pytest.mark.parametrize("cfg", CFGS)
def test_an_installed_dense_mass_survives(cfg, hip):
    cx = HS.ctx(cfg)

    def run(between):
        with cx.handle() as h:
            assert "rc" not in HS.op_set_dense_mass(cx, h)
            if between:
                assert "rc" not in op_conv(cx, h)
            return HS.op_sample_chains_host(cx, h)

    with cx.handle() as h:
        diagonal = HS.op_sample_chains_host(cx, h)
    dense = run(False)
    assert "rc" not in dense and not HS.same(dense, diagonal)      # the mass is read by this run
    assert HS.same(run(True), dense)


@pytest.mark.parametrize("cfg", CFGS)
def test_resident_chains_continue_across_a_call(cfg, hip):
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
                assert "rc" not in op_conv(cx, h)
            rc, lf2, dv2 = HS._advance(cx, h, cx.ns - n1, n1, trd, tr)
            assert rc == 0
            return dict(lf=np.array([lf1, lf2]), dv=np.array([dv1, dv2]), **HS._devd(trd))

    assert HS.same(run(True), run(False))


def test_refused_while_a_stream_run_is_in_flight(hip):
    """both entry points answer EXMC_ERR_BADARG between stream_start and stream_finish, and work after"""
    cx = HS.ctx("es16")
    with cx.handle() as h:
        tun = _lib.Tuning()
        _lib.check(cx.L.exmc_hip_stream_begin(h, HS._dp(cx.q0), cx.opts(cx.nw, 0, 43, 0), C.byref(tun)), cx.L)
        view, prog = _lib.Trace(), C.POINTER(C.c_int32)()
        _lib.check(cx.L.exmc_hip_stream_start(h, cx.ns, C.byref(view), C.byref(prog)), cx.L)
        try:
            assert op_conv(cx, h) == {"rc": _lib.ERR_BADARG}
            assert b"in flight" in cx.L.exmc_hip_last_error()
            rc = cx.L.exmc_hip_convergence(h, None, 8, cx.d, 1, 0, None)
            assert rc == _lib.ERR_BADARG and b"in flight" in cx.L.exmc_hip_last_error()
        finally:
            dv = C.c_int32()
            _lib.check(cx.L.exmc_hip_stream_finish(h, C.byref(dv)), cx.L)
        assert HS.same(op_conv(cx, h), _fresh(cx))
