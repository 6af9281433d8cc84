"""Handle state of the model-comparison entry points (include/exmc_hip_compare.h "Handle state"): each
reads no handle state and leaves the flat order, a dense mass and resident chains in place. Against
every op of test_gpu_handle_state's catalogue: op then compare, and compare then op, equal their
fresh-handle results; chains_init -> ic_stats -> chains_advance continues the resident chains."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_handle_state as HS
from exmc_amd import _lib

pytestmark = pytest.mark.gpu

CFGS = ["es16", "sv64"]


def op_compare(cx, h):
    import torch
    S, Cn = cx.diag_shape
    x = cx.diag_trace
    L = cx.L
    N = L.exmc_hip_model_n_data(h)
    ll = torch.zeros((S, N, Cn), dtype=torch.float64, device=cx.dev)
    st = torch.zeros((4, N), dtype=torch.float64, device=cx.dev)
    torch.cuda.synchronize()
    rc = L.exmc_hip_pointwise_loglik(h, x.data_ptr(), S, cx.d, Cn, ll.data_ptr())
    if rc:
        return {"rc": rc}
    rc = L.exmc_hip_ic_stats(h, x.data_ptr(), S, cx.d, Cn, st.data_ptr())
    if rc:
        return {"rc": rc}
    host = np.ascontiguousarray(x.cpu().numpy().transpose(2, 0, 1))
    sh = np.zeros((4, N))
    rc = L.exmc_hip_ic_stats_host(h, host.ctypes.data_as(C.POINTER(C.c_double)), S, cx.d, Cn,
                                  sh.ctypes.data_as(C.POINTER(C.c_double)))
    if rc:
        return {"rc": rc}
    torch.cuda.synchronize()
    return dict(n=np.int64(N), ll=ll.cpu().numpy(), st=st.cpu().numpy(), sh=sh)


ENTRY_POINTS = {"compare": ["exmc_hip_model_n_data", "exmc_hip_pointwise_loglik", "exmc_hip_ic_stats",
                            "exmc_hip_ic_stats_host"]}


def _fresh_compare(cx):
    k = ("compare", None)
    if k not in cx.fresh:
        with cx.handle() as h:
            cx.fresh[k] = op_compare(cx, h)
    return cx.fresh[k]


@pytest.mark.parametrize("a", list(HS.OPS))
@pytest.mark.parametrize("cfg", CFGS)
def test_compare_after_and_before_every_op(cfg, a, hip):
    cx = HS.ctx(cfg)
    want = _fresh_compare(cx)
    assert "rc" not in want
    with cx.handle() as h:
        HS.OPS[a](cx, h)
        got = op_compare(cx, h)
    assert HS.same(got, want), a
    # compare first: op a sees a fresh handle (compare installs and evicts nothing)
    with cx.handle() as h:
        op_compare(cx, h)
        got = HS.OPS[a](cx, h)
    assert HS.same(got, HS.expected(cx, a)), HS.diff(got, HS.expected(cx, a))


@pytest.mark.parametrize("cfg", CFGS)
def test_resident_chains_continue_across_ic_stats(cfg, hip):
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
                assert "rc" not in op_compare(cx, h)
            rc, lf2, dv2 = HS._advance(cx, h, cx.ns - n1, n1, trd, tr)
            assert rc == 0
            return dict(lf=np.array([lf1, lf2]), dv=np.array([dv1, dv2]), **HS._devd(trd))

    assert HS.same(run(True), run(False))
