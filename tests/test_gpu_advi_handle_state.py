"""Handle state of the ADVI entry points (include/exmc_hip_advi.h "Handle state"): the call reads the
flat order and nothing else, and leaves the flat order, a dense mass and resident chains in place.
Against every op of test_gpu_handle_state's catalogue: op then advi, and advi then op, equal their
fresh-handle results; chains_init -> advi -> chains_advance continues the resident chains."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_handle_state as HS
from exmc_amd import _lib

pytestmark = pytest.mark.gpu

CFGS = ["es16", "sv64"]


def _opts(cx, num_draws=2):
    # window 4 with a tolerance of 0.05: some of the three fits stop before max_iters (the window is read back)
    return _lib.AdviOpts(num_draws, 9, 2, 4, 0.05, 0.05, 17, cx.lanes)


def op_advi(cx, h):
    Cn, S, d = 3, 2, cx.d
    out = dict(draws=np.zeros((Cn, S, d)), mu=np.zeros((Cn, d)), log_sigma=np.zeros((Cn, d)),
               elbo_history=np.zeros((Cn, 9)), num_iters=np.zeros(Cn, np.int32), converged=np.zeros(Cn, np.int32))
    rc = cx.L.exmc_hip_advi_host(h, _opts(cx, S), Cn, 1,
                                 *[HS._dp(out[k]) for k in ("draws", "mu", "log_sigma", "elbo_history")],
                                 *[HS._ip(out[k]) for k in ("num_iters", "converged")])
    if rc:
        return {"rc": rc}
    out["elbo_history"] = np.nan_to_num(out["elbo_history"], nan=-7.0)   # NaN after num_iters: compare as a value
    return out


def _fresh(cx):
    k = ("advi", None)
    if k not in cx.fresh:
        with cx.handle() as h:
            cx.fresh[k] = op_advi(cx, h)
    return cx.fresh[k]


@pytest.mark.parametrize("a", list(HS.OPS))
@pytest.mark.parametrize("cfg", CFGS)
def test_advi_after_and_before_every_op(cfg, a, hip):
    cx = HS.ctx(cfg)
    want = _fresh(cx)
    assert "rc" not in want
    with cx.handle() as h:
        HS.OPS[a](cx, h)
        got = op_advi(cx, h)
    assert HS.same(got, want), a
    # advi first: op a sees a fresh handle (advi installs and evicts nothing)
    with cx.handle() as h:
        op_advi(cx, h)
        got = HS.OPS[a](cx, h)
    assert HS.same(got, HS.expected(cx, a)), HS.diff(got, HS.expected(cx, a))


@pytest.mark.parametrize("cfg", CFGS)
def test_resident_chains_continue_across_advi(cfg, hip):
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
                assert "rc" not in op_advi(cx, h)
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
            assert op_advi(cx, h) == {"rc": _lib.ERR_BADARG}
            assert b"in flight" in cx.L.exmc_hip_last_error()
            rc = cx.L.exmc_hip_advi(h, _opts(cx), 3, 1, None, None, None, None, None, None)
            assert rc == _lib.ERR_BADARG and b"in flight" in cx.L.exmc_hip_last_error()
        finally:
            dv = C.c_int32()
            _lib.check(cx.L.exmc_hip_stream_finish(h, C.byref(dv)), cx.L)
        assert HS.same(op_advi(cx, h), _fresh(cx))
