"""Handle state of the LOO-PIT entry points (include/exmc_hip_loo_pit.h "Handle state"): the call reads none
and changes none. After LOO-PIT every op of the catalogue (tests/test_gpu_handle_state.py) equals its
fresh-handle result, and LOO-PIT after every op equals its own; an installed dense mass and resident
chains survive the call; exmc_hip_psis_stats gives the same bytes before and after it; a handle with a
stream run in flight refuses it."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_handle_state as HS
from exmc_amd import _lib

pytestmark = pytest.mark.gpu

CFGS = ["es16", "sv64"]
Cn, S = 70, 2     # two blocks of chains


def _trace(cx):
    return np.ascontiguousarray(cx.q0[None, None, :] + 0.25 * np.random.default_rng(77).normal(size=(Cn, S, cx.d)))


def op_loo_pit(cx, h):
    N = cx.L.exmc_hip_model_n_data(h)
    out = np.zeros((4, N))
    rc = cx.L.exmc_hip_loo_pit_host(h, _lib.PredictiveOpts(17, 1, 0), HS._dp(_trace(cx)), S, cx.d, Cn, 0, HS._dp(out))
    return {"rc": rc} if rc else dict(out=out)


def op_psis(cx, h):
    N = cx.L.exmc_hip_model_n_data(h)
    out = np.zeros((3, N))
    rc = cx.L.exmc_hip_psis_stats_host(h, HS._dp(_trace(cx)), S, cx.d, Cn, 0, HS._dp(out))
    return {"rc": rc} if rc else dict(out=out)


def _fresh(cx):
    k = ("loo_pit", None)
    if k not in cx.fresh:
        with cx.handle() as h:
            cx.fresh[k] = op_loo_pit(cx, h)
    return cx.fresh[k]


@pytest.mark.parametrize("cfg", CFGS)
def test_after_and_before_every_op(cfg, hip):
    cx = HS.ctx(cfg)
    want = _fresh(cx)
    assert "rc" not in want and np.isfinite(want["out"]).all()
    bad = []
    for name, op in HS.OPS.items():
        with cx.handle() as h:
            if not HS.same(op_loo_pit(cx, h), want):
                bad.append(("first", name))
            got = op(cx, h)                                    # the op after LOO-PIT == the op on a fresh handle
            if not HS.same(got, HS.expected(cx, name)):
                bad.append((name, "after loo_pit", HS.diff(got, HS.expected(cx, name))))
            if not HS.same(op_loo_pit(cx, h), want):           # LOO-PIT after the op == LOO-PIT on a fresh handle
                bad.append(("loo_pit after", name))
    assert not bad, bad


@pytest.mark.parametrize("cfg", CFGS)
def test_psis_stats_is_the_same_before_and_after(cfg, hip):
    cx = HS.ctx(cfg)
    with cx.handle() as h:
        before = op_psis(cx, h)
        assert HS.same(op_loo_pit(cx, h), _fresh(cx))
        after = op_psis(cx, h)
    assert "rc" not in before and HS.same(before, after)
    # ... and the k of LOO-PIT is that k
    assert before["out"][2].tobytes() == np.ascontiguousarray(_fresh(cx)["out"][3]).tobytes()


@pytest.mark.parametrize("cfg", CFGS)
def test_an_installed_dense_mass_survives(cfg, hip):
    cx = HS.ctx(cfg)

    def run(between):
        with cx.handle() as h:
            assert "rc" not in HS.op_set_dense_mass(cx, h)
            if between:
                assert "rc" not in op_loo_pit(cx, h)
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
                assert "rc" not in op_loo_pit(cx, h)
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
            assert op_loo_pit(cx, h) == {"rc": _lib.ERR_BADARG}
            assert b"in flight" in cx.L.exmc_hip_last_error()
            rc = cx.L.exmc_hip_loo_pit(h, _lib.PredictiveOpts(1, 0, 0), None, 1, cx.d, 1, 0, None)
            assert rc == _lib.ERR_BADARG and b"in flight" in cx.L.exmc_hip_last_error()
        finally:
            dv = C.c_int32()
            _lib.check(cx.L.exmc_hip_stream_finish(h, C.byref(dv)), cx.L)
        assert HS.same(op_loo_pit(cx, h), _fresh(cx))
