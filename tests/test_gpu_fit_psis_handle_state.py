"""Handle state of the fits' importance diagnostics (include/exmc_hip_fit_psis.h "Handle state"): the calls
read the model and change nothing. A sampling run after a call equals one on a fresh handle (the flat order
is read by it); an installed dense mass and resident chains survive the call; a handle with a stream run in
flight refuses it. Fresh handles throughout, in the pattern of test_gpu_convergence_handle_state.py."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_handle_state as HS
from exmc_amd import _lib

pytestmark = pytest.mark.gpu

CFGS = ["es16", "sv64"]


def op_fit_psis(cx, h):
    Cn, S, R = 3, 40, 7      # tails of 8 samples: the fit and the smoothing run
    rng = np.random.default_rng(77)
    mu = np.ascontiguousarray(cx.q0[None, :] + 0.05 * rng.normal(size=(Cn, cx.d)))
    sigma = np.full((Cn, cx.d), 0.2)
    x = np.ascontiguousarray(mu[:, None, :] + sigma[:, None, :] * rng.normal(size=(Cn, S, cx.d)))
    out, lw, lr = np.zeros((5, Cn)), np.zeros((Cn, S)), np.zeros((Cn, S))
    idx, res = np.zeros((Cn, R), np.int32), np.zeros((Cn, R, cx.d))
    rc = cx.L.exmc_hip_fit_psis_host(h, HS._dp(x), HS._dp(mu), HS._dp(sigma), _lib.FIT_SIGMA, S, cx.d, Cn, 0, 0, R, 5,
                                     HS._dp(out), HS._dp(lw), HS._ip(idx), HS._dp(res), HS._dp(lr), None)
    return {"rc": rc} if rc else dict(out=out, lw=lw, idx=idx, res=res, lr=lr)


def _fresh(cx):
    k = ("fit_psis", None)
    if k not in cx.fresh:
        with cx.handle() as h:
            cx.fresh[k] = op_fit_psis(cx, h)
    return cx.fresh[k]


@pytest.mark.parametrize("cfg", CFGS)
def test_sampling_after_a_call_equals_a_fresh_handle(cfg, hip):
    cx = HS.ctx(cfg)
    want_psis = _fresh(cx)
    assert "rc" not in want_psis and np.all(np.isfinite(want_psis["lr"])) and want_psis["idx"].min() >= 0
    with cx.handle() as h:
        want = HS.op_sample_host(cx, h)
    with cx.handle() as h:
        assert HS.same(op_fit_psis(cx, h), want_psis)
        got = HS.op_sample_host(cx, h)
        # ... and the call after the sampling run equals its fresh-handle result
        assert HS.same(op_fit_psis(cx, h), want_psis)
    assert "rc" not in want and HS.same(got, want), HS.diff(got, want)


@pytest.mark.parametrize("cfg", CFGS)
def test_an_installed_dense_mass_survives(cfg, hip):
    cx = HS.ctx(cfg)

    def run(between):
        with cx.handle() as h:
            assert "rc" not in HS.op_set_dense_mass(cx, h)
            if between:
                assert HS.same(op_fit_psis(cx, h), _fresh(cx))
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
                assert "rc" not in op_fit_psis(cx, h)
            rc, lf2, dv2 = HS._advance(cx, h, cx.ns - n1, n1, trd, tr)
            assert rc == 0
            return dict(lf=np.array([lf1, lf2]), dv=np.array([dv1, dv2]), **HS._devd(trd))

    assert HS.same(run(True), run(False))


def test_refused_while_a_stream_run_is_in_flight(hip):
    """the entry points that take a handle answer EXMC_ERR_BADARG between stream_start and stream_finish, and
    work after"""
    cx = HS.ctx("es16")
    with cx.handle() as h:
        tun = _lib.Tuning()
        _lib.check(cx.L.exmc_hip_stream_begin(h, HS._dp(cx.q0), cx.opts(cx.nw, 0, 43, 0), C.byref(tun)), cx.L)
        view, prog = _lib.Trace(), C.POINTER(C.c_int32)()
        _lib.check(cx.L.exmc_hip_stream_start(h, cx.ns, C.byref(view), C.byref(prog)), cx.L)
        try:
            assert op_fit_psis(cx, h) == {"rc": _lib.ERR_BADARG}
            assert b"in flight" in cx.L.exmc_hip_last_error()
            rc = cx.L.exmc_hip_fit_log_ratio(h, None, None, None, 0, 1, cx.d, 1, 0, None, None)
            assert rc == _lib.ERR_BADARG and b"in flight" in cx.L.exmc_hip_last_error()
            rc = cx.L.exmc_hip_fit_psis(h, None, None, None, 0, 1, cx.d, 1, 0, 0, 0, 0, None, None, None, None, None,
                                        None)
            assert rc == _lib.ERR_BADARG and b"in flight" in cx.L.exmc_hip_last_error()
        finally:
            dv = C.c_int32()
            _lib.check(cx.L.exmc_hip_stream_finish(h, C.byref(dv)), cx.L)
        assert HS.same(op_fit_psis(cx, h), _fresh(cx))
