"""Handle state of the prior entry points (include/exmc_hip_prior.h "Handle state"): the call reads the flat
order and changes nothing. A sampling run after a prior call equals one on a fresh handle (the flat order
it draws its momenta in is in place; sv's is not the identity); an installed dense mass and resident
chains survive the call; a handle with a stream run in flight refuses it."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_handle_state as HS
from exmc_amd import _lib

pytestmark = pytest.mark.gpu

CFGS = ["es16", "sv64"]


def op_prior(cx, h):
    Cn, S = 3, 2
    N = cx.L.exmc_hip_model_n_data(h)
    x, q, out = np.zeros((Cn, S, cx.d)), np.zeros((Cn, S, cx.d)), np.zeros((Cn, S, N))
    st = np.zeros((2, Cn), np.uint64)
    rc = cx.L.exmc_hip_prior_samples_host(h, _lib.PredictiveOpts(17, 1, 0), S, Cn, st.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          HS._dp(x), HS._dp(q), HS._dp(out))
    return {"rc": rc} if rc else dict(x=x, q=q, yrep=out, state=st.view(np.int64))


def _fresh(cx):
    k = ("prior", None)
    if k not in cx.fresh:
        with cx.handle() as h:
            cx.fresh[k] = op_prior(cx, h)
    return cx.fresh[k]


@pytest.mark.parametrize("cfg", CFGS)
def test_sampling_after_a_prior_call_equals_a_fresh_handle(cfg, hip):
    cx = HS.ctx(cfg)
    want_pr = _fresh(cx)
    assert "rc" not in want_pr
    with cx.handle() as h:
        want = HS.op_sample_host(cx, h)
    with cx.handle() as h:
        assert HS.same(op_prior(cx, h), want_pr)
        got = HS.op_sample_host(cx, h)
        # ... and the prior call after the sampling run equals its fresh-handle result
        assert HS.same(op_prior(cx, h), want_pr)
    assert "rc" not in want and HS.same(got, want), HS.diff(got, want)


def test_the_walk_follows_the_flat_order_and_leaves_it(hip):
    """eight_schools has no parents: the walk is the flat order. Reversing it gives another walk (the same
    variates land in other variables); putting it back gives the first one again."""
    cx = HS.ctx("es16")
    ident = np.arange(cx.d, dtype=np.int32)
    rev = np.ascontiguousarray(ident[::-1])
    ip = C.POINTER(C.c_int32)
    with cx.handle() as h:
        a = op_prior(cx, h)
        _lib.check(cx.L.exmc_hip_model_set_flat_order(h, rev.ctypes.data_as(ip), cx.d), cx.L)
        b = op_prior(cx, h)
        b2 = op_prior(cx, h)
        _lib.check(cx.L.exmc_hip_model_set_flat_order(h, ident.ctypes.data_as(ip), cx.d), cx.L)
        c = op_prior(cx, h)
    assert HS.same(a, _fresh(cx)) and HS.same(c, a) and HS.same(b, b2) and not HS.same(a, b)
    # the first variate of a chain is mu's (N(0, 5)) in the identity order and theta_trans_7's (N(0, 1)) reversed
    assert np.array_equal(a["x"][:, 0, 0], 5.0 * b["x"][:, 0, 9])


@pytest.mark.parametrize("cfg", CFGS)
def test_an_installed_dense_mass_survives(cfg, hip):
    cx = HS.ctx(cfg)

    def run(between):
        with cx.handle() as h:
            assert "rc" not in HS.op_set_dense_mass(cx, h)
            if between:
                assert "rc" not in op_prior(cx, h)
            return HS.op_sample_chains_host(cx, h)

    with cx.handle() as h:
        diagonal = HS.op_sample_chains_host(cx, h)
    dense = run(False)
    assert "rc" not in dense and not HS.same(dense, diagonal)      # the mass is read by this run
    assert HS.same(run(True), dense)


@pytest.mark.parametrize("cfg", CFGS)
def test_resident_chains_continue_across_a_prior_call(cfg, hip):
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
                assert "rc" not in op_prior(cx, h)
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
            assert op_prior(cx, h) == {"rc": _lib.ERR_BADARG}
            assert b"in flight" in cx.L.exmc_hip_last_error()
            rc = cx.L.exmc_hip_prior_samples(h, _lib.PredictiveOpts(1, 0, 0), 1, 1, None, None, None, None)
            assert rc == _lib.ERR_BADARG and b"in flight" in cx.L.exmc_hip_last_error()
        finally:
            dv = C.c_int32()
            _lib.check(cx.L.exmc_hip_stream_finish(h, C.byref(dv)), cx.L)
        assert HS.same(op_prior(cx, h), _fresh(cx))
