"""Posterior predictive replicates on the device (exmc_amd/csrc/exmc_predictive.hpp,
include/exmc_hip_predictive.h, exmc_amd/predictive.py) against the statement of predictive.ex and its
sample/2 callbacks (tests/predictive_statement.py), bit for bit: every built-in kind on two wavefronts
(the second partial); continuation through the carried generators; sharding by chain_lo; the host form and
the block form; hostile rows; refusals. tests/test_predictive_statement.py shows on the CPU that these
inputs take every branch of the samplers."""
import ctypes as C

import numpy as np
import pytest
import torch

import predictive_inputs as PI
import predictive_statement as PS
from exmc_amd import _lib, models, sampler
from exmc_amd import predictive as PP

pytestmark = pytest.mark.gpu

_comp = {}


def comp(kind):
    if kind not in _comp:
        _comp[kind] = sampler.compile(PI.spec(kind))
    return _comp[kind]


def device_call(cm, x, seed, chain_lo, resume=False, state=None, want_state=True):
    """exmc_hip_posterior_predictive on the host array x [S][d][C] -> (yrep [S][N][C], state [2][C] uint64)"""
    S, d, Cn = x.shape
    N = cm.L.exmc_hip_model_n_data(cm.h)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.empty((S, N, Cn), dtype=torch.float64, device="cuda")
    st = None
    if want_state or state is not None:
        st = torch.from_numpy((np.zeros((2, Cn), np.uint64) if state is None else state).view(np.int64)).cuda()
    torch.cuda.synchronize()
    cm.check(cm.L.exmc_hip_posterior_predictive(cm.h, _lib.PredictiveOpts(seed, chain_lo, 1 if resume else 0),
                                                xd.data_ptr(), S, d, Cn, None if st is None else st.data_ptr(),
                                                out.data_ptr()))
    return out.cpu().numpy(), None if st is None else st.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("kind", PI.KINDS)
def test_parity_with_the_statement(kind, hip):
    x, want, want_state, n = PI.expected(kind)
    assert x.shape[2] == 70 and x.shape[0] == 3 and n["cap"] == 0
    got, state = device_call(comp(kind), x, PI.SEED, PI.CHAIN_LO)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5]
    assert state.tobytes() == want_state.tobytes()
    assert comp(kind).last_kernel_ms > 0.0
    # the Python call: the same matrix, the names in the handle's order
    yrep, names = PP.posterior_predictive(comp(kind), torch.from_numpy(x).cuda(), seed=PI.SEED, chain_lo=PI.CHAIN_LO)
    assert yrep.cpu().numpy().tobytes() == want.tobytes()
    assert len(names) == want.shape[1]
    if kind == models.RADON:
        assert names[0] == ("radon", int(PI.spec(kind).datum_order[0]))
    tr = PP.as_trace(yrep, names)
    assert tr[names[1]].shape == (70, 3) and tr[names[1]][5, 2] == want[2, 1, 5]


@pytest.mark.parametrize("kind", PI.KINDS)
def test_continuation_and_sharding(kind, hip):
    cm = comp(kind)
    x = PI.draws(kind, S=5)
    whole, st = device_call(cm, x, 23, 1)
    a, sa = device_call(cm, x[:2], 23, 1)
    b, sb = device_call(cm, x[2:], 99, 7, resume=True, state=sa)      # a resumed call reads neither seed nor chain_lo
    assert np.concatenate([a, b]).tobytes() == whole.tobytes()
    assert sb.tobytes() == st.tobytes()
    # chains [0, 70) in one call == [0, 32) and [32, 70) with chain_lo = 32, with or without a state
    lo, slo = device_call(cm, x[:, :, :32], 23, 1)
    hi, _ = device_call(cm, x[:, :, 32:], 23, 1 + 32, want_state=False)
    assert np.concatenate([lo, hi], axis=2).tobytes() == whole.tobytes()
    assert slo.tobytes() == np.ascontiguousarray(st[:, :32]).tobytes()


@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.SV_NCP, models.RADON])
def test_host_form_and_block_form(kind, hip):
    cm = comp(kind)
    x = PI.draws(kind, S=5)
    S, d, Cn = x.shape
    whole, st = device_call(cm, x, 31, 0)
    N = whole.shape[1]
    host_in = np.ascontiguousarray(x.transpose(2, 0, 1))            # [C][S][d]
    host_out, host_state = np.zeros((Cn, S, N)), np.zeros((2, Cn), np.uint64)
    cm.check(cm.L.exmc_hip_posterior_predictive_host(
        cm.h, _lib.PredictiveOpts(31, 0, 0), host_in.ctypes.data_as(C.POINTER(C.c_double)), S, d, Cn,
        host_state.ctypes.data_as(C.POINTER(C.c_uint64)), host_out.ctypes.data_as(C.POINTER(C.c_double))))
    assert host_out.tobytes() == np.ascontiguousarray(whole.transpose(2, 0, 1)).tobytes()
    assert host_state.tobytes() == st.tobytes()
    # ... and resumed on the host, without a state out the second time
    first = np.zeros((Cn, 2, N))
    cm.check(cm.L.exmc_hip_posterior_predictive_host(
        cm.h, _lib.PredictiveOpts(31, 0, 0), np.ascontiguousarray(host_in[:, :2]).ctypes.data_as(C.POINTER(C.c_double)),
        2, d, Cn, host_state.ctypes.data_as(C.POINTER(C.c_uint64)), first.ctypes.data_as(C.POINTER(C.c_double))))
    rest = np.zeros((Cn, 3, N))
    cm.check(cm.L.exmc_hip_posterior_predictive_host(
        cm.h, _lib.PredictiveOpts(0, 0, 1), np.ascontiguousarray(host_in[:, 2:]).ctypes.data_as(C.POINTER(C.c_double)),
        3, d, Cn, host_state.ctypes.data_as(C.POINTER(C.c_uint64)), rest.ctypes.data_as(C.POINTER(C.c_double))))
    assert np.concatenate([first, rest], axis=1).tobytes() == host_out.tobytes() and host_state.tobytes() == st.tobytes()
    # the Python forms: a host trace [C][S][d], and the blocks joined
    yrep, names = PP.posterior_predictive(cm, host_in, seed=31)
    assert yrep.cpu().numpy().tobytes() == whole.tobytes()
    blocks = list(PP.posterior_predictive_blocks(cm, torch.from_numpy(x).cuda(), 2, seed=31))
    assert [s0 for s0, _ in blocks] == [0, 2, 4] and [b.shape[0] for _, b in blocks] == [2, 2, 1]
    assert torch.cat([b for _, b in blocks]).cpu().numpy().tobytes() == whole.tobytes()
    with pytest.raises(ValueError, match="posterior_predictive_blocks"):
        PP.posterior_predictive(cm, host_in, seed=31, max_bytes=whole.nbytes - 1)
    with pytest.raises(ValueError):
        next(PP.posterior_predictive_blocks(cm, host_in, 0))


@pytest.mark.parametrize("kind", PI.KINDS)
def test_hostile_rows(kind, hip):
    x, want, want_state, n = PI.expected(kind, "hostile")      # the statement terminated on the CPU
    got, state = device_call(comp(kind), x, PI.SEED, PI.CHAIN_LO)
    fin = np.isfinite(want)
    assert (np.isfinite(got) == fin).all()
    assert got[fin].tobytes() == want[fin].tobytes()
    assert (np.isnan(got) == np.isnan(want)).all()
    assert (got[~fin & ~np.isnan(want)] == want[~fin & ~np.isnan(want)]).all()     # the infinities and their signs
    assert state.tobytes() == want_state.tobytes()


def test_refusals(hip):
    cm = comp(models.SIMPLE)
    x = PI.draws(models.SIMPLE, S=2, Cn=3)
    S, d, Cn = x.shape
    xd = torch.from_numpy(x).cuda()
    out = torch.empty((S, 10, Cn), dtype=torch.float64, device="cuda")
    st = torch.zeros((2, Cn), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L, O = cm.L, _lib.PredictiveOpts
    f = L.exmc_hip_posterior_predictive
    assert f(cm.h, O(1, 0, 0), xd.data_ptr(), S, d, Cn, st.data_ptr(), out.data_ptr()) == _lib.OK
    bad = [(cm.h, O(1, 0, 0), None, S, d, Cn, None, out.data_ptr()),             # no trace
           (cm.h, O(1, 0, 0), xd.data_ptr(), S, d, Cn, None, None),              # no output
           (cm.h, O(1, 0, 0), xd.data_ptr(), S, d + 1, Cn, None, out.data_ptr()),
           (cm.h, O(1, 0, 0), xd.data_ptr(), 0, d, Cn, None, out.data_ptr()),
           (cm.h, O(1, 0, 0), xd.data_ptr(), S, d, 0, None, out.data_ptr()),
           (cm.h, O(1, -1, 0), xd.data_ptr(), S, d, Cn, None, out.data_ptr()),
           (cm.h, O(1, 0, 1), xd.data_ptr(), S, d, Cn, None, out.data_ptr()),    # resume without a state
           (None, O(1, 0, 0), xd.data_ptr(), S, d, Cn, None, out.data_ptr())]
    for args in bad:
        assert f(*args) == _lib.ERR_BADARG, args[1:]
    hin, hout = np.zeros((Cn, S, d)), np.zeros((Cn, S, 10))
    dp = C.POINTER(C.c_double)
    g = L.exmc_hip_posterior_predictive_host
    assert g(cm.h, O(1, 0, 0), hin.ctypes.data_as(dp), S, d, Cn, None, hout.ctypes.data_as(dp)) == _lib.OK
    assert g(cm.h, O(1, 0, 0), None, S, d, Cn, None, hout.ctypes.data_as(dp)) == _lib.ERR_BADARG
    assert g(cm.h, O(1, 0, 0), hin.ctypes.data_as(dp), S, d, Cn, None, None) == _lib.ERR_BADARG
    assert g(cm.h, O(1, 0, 1), hin.ctypes.data_as(dp), S, d, Cn, None, hout.ctypes.data_as(dp)) == _lib.ERR_BADARG
    assert g(cm.h, O(1, -3, 0), hin.ctypes.data_as(dp), S, d, Cn, None, hout.ctypes.data_as(dp)) == _lib.ERR_BADARG
    with pytest.raises(ValueError):
        PP.posterior_predictive(cm, xd.float())


def test_unsupported_models(hip):
    from exmc_amd import codegen
    # EXMC_MODEL_STD_NORMAL has no data: the library makes no handle of it
    h = C.c_void_p()
    assert hip.exmc_hip_model_create(models.STD_NORMAL, 2, None, 0, 0, C.byref(h)) == _lib.ERR_UNSUPPORTED
    # a generated model, compiled WITH its per-datum terms: it has datums for model comparison, none here
    gen = sampler.compile(codegen.compile_ir(codegen.eight_schools_ir(), pointwise=True))
    try:
        assert gen.L.exmc_hip_model_n_data(gen.h) == 8
        for name in _lib.PREDICTIVE_EXPORTS:
            getattr(gen.L, name)
        xd = torch.zeros((2, gen.d, 3), dtype=torch.float64, device="cuda")
        out = torch.zeros((2, 8, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = gen.L.exmc_hip_posterior_predictive(gen.h, _lib.PredictiveOpts(1, 0, 0), xd.data_ptr(), 2, gen.d, 3, None,
                                                 out.data_ptr())
        assert rc == _lib.ERR_UNSUPPORTED
        assert b"posterior predictive" in gen.L.exmc_hip_last_error()
        hin, hout = np.zeros((3, 2, gen.d)), np.zeros((3, 2, 8))
        dp = C.POINTER(C.c_double)
        assert gen.L.exmc_hip_posterior_predictive_host(gen.h, _lib.PredictiveOpts(1, 0, 0), hin.ctypes.data_as(dp), 2,
                                                        gen.d, 3, None, hout.ctypes.data_as(dp)) == _lib.ERR_UNSUPPORTED
        with pytest.raises(_lib.ExmcHipError):
            PP.posterior_predictive(gen, xd)
    finally:
        gen.close()
