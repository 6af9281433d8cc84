"""`Elixir.Exmc.NUTS.HipPriorNative.prior_samples/6` (c_src/exmc_hip_prior_nif.c) called through
tests/host/fake_erl_nif.c, as the BEAM would call it: equal to exmc_hip_prior_samples_host byte for byte, with
and without replicates; a wrong tuple is a badarg; a kind without a handle raises {:exmc_hip_error, 4, _}."""
import ctypes as C

import numpy as np
import pytest

import nif_harness as H
import predictive_inputs as PI
from exmc_amd import _lib, models, sampler

pytestmark = pytest.mark.gpu

ERL_NIF_DIRTY_JOB_IO_BOUND = 2


@pytest.fixture(scope="module")
def mod(tmp_path_factory):
    return H.load_shim(str(tmp_path_factory.mktemp("priornif")), "exmc_hip_prior_nif.c")


@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.SV_NCP])
def test_nif_equals_the_c_call(hip, mod, kind):
    assert mod.name == "Elixir.Exmc.NUTS.HipPriorNative"
    assert mod.table() == [("prior_samples", 6, ERL_NIF_DIRTY_JOB_IO_BOUND)]
    spec = PI.spec(kind)
    Cn, S, d = 5, 3, spec.d
    # a handle of the kind and its data alone, as the NIF makes it (the default flat order)
    h = C.c_void_p()
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    _lib.check(L.exmc_hip_model_create(spec.kind, 0, spec.data.ctypes.data_as(dp), spec.data.size, 0, C.byref(h)), L)
    try:
        N = L.exmc_hip_model_n_data(h)
        wx, wq, wy = np.zeros((Cn, S, d)), np.zeros((Cn, S, d)), np.zeros((Cn, S, N))
        _lib.check(L.exmc_hip_prior_samples_host(h, _lib.PredictiveOpts(19, 2, 0), S, Cn, None, wx.ctypes.data_as(dp),
                                                 wq.ctypes.data_as(dp), wy.ctypes.data_as(dp)), L)
        bx, bq = np.zeros((Cn, S, d)), np.zeros((Cn, S, d))
        _lib.check(L.exmc_hip_prior_samples_host(h, _lib.PredictiveOpts(19, 2, 0), S, Cn, None, bx.ctypes.data_as(dp),
                                                 bq.ctypes.data_as(dp), None), L)
    finally:
        L.exmc_hip_model_destroy(h)
    got = mod.call("prior_samples", H.tuple_term(mod, spec.kind, spec.data), Cn, S, 19, 2, 1)
    assert isinstance(got, tuple) and len(got) == 3
    assert got[0] == wx.tobytes() and got[1] == wq.tobytes() and got[2] == wy.tobytes()
    assert np.isfinite(wx).all() and np.isfinite(wy).all() and len(np.unique(wy)) > Cn * S
    bare = mod.call("prior_samples", H.tuple_term(mod, spec.kind, spec.data), Cn, S, 19, 2, 0)
    assert bare[0] == bx.tobytes() and bare[1] == bq.tobytes() and bare[2] == b""
    assert bx[:, 0].tobytes() == wx[:, 0].tobytes() and bx[:, 1].tobytes() != wx[:, 1].tobytes()
    # for a kind whose handle sampler.compile makes with the same flat order, the compiled handle agrees
    comp = sampler.compile(spec)
    try:
        cx, cq = np.zeros((Cn, S, d)), np.zeros((Cn, S, d))
        comp.check(comp.L.exmc_hip_prior_samples_host(comp.h, _lib.PredictiveOpts(19, 2, 0), S, Cn, None,
                                                      cx.ctypes.data_as(dp), cq.ctypes.data_as(dp), None))
    finally:
        comp.close()
    assert cx.tobytes() == bx.tobytes() and cq.tobytes() == bq.tobytes()


def test_nif_refusals(hip, mod):
    spec = PI.spec(models.EIGHT_SCHOOLS)
    model = lambda: H.tuple_term(mod, spec.kind, spec.data)   # noqa: E731
    with pytest.raises(H.BadArg):                       # a list is not the {kind, data} tuple
        mod.call("prior_samples", [spec.kind, spec.data], 2, 3, 19, 0, 1)
    with pytest.raises(H.BadArg):                       # a 3-tuple neither
        mod.call("prior_samples", H.tuple_term(mod, spec.kind, spec.data, 1), 2, 3, 19, 0, 1)
    with pytest.raises(H.BadArg):                       # a negative chain_lo
        mod.call("prior_samples", model(), 2, 3, 19, -1, 1)
    with pytest.raises(H.BadArg):                       # no chains, no draws
        mod.call("prior_samples", model(), 0, 3, 19, 0, 1)
    with pytest.raises(H.BadArg):
        mod.call("prior_samples", model(), 2, 0, 19, 0, 1)
    with pytest.raises(H.BadArg):                       # replicates is 0 or 1
        mod.call("prior_samples", model(), 2, 3, 19, 0, 2)
    with pytest.raises(H.Raised) as e:                  # a kind the library has no handle for: {:exmc_hip_error, 4, _}
        mod.call("prior_samples", H.tuple_term(mod, models.STD_NORMAL, np.zeros(0)), 2, 3, 19, 0, 1)
    assert e.value.reason[:2] == (H.Atom("exmc_hip_error"), 4)
