"""`Elixir.Exmc.NUTS.HipPredictiveNative.posterior_predictive/6` (c_src/exmc_hip_predictive_nif.c) called
through tests/host/fake_erl_nif.c, as the BEAM would call it: equal to exmc_hip_posterior_predictive_host
byte for byte; a wrong tuple is a badarg; a kind without a handle raises {:exmc_hip_error, 4, _}."""
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
    return H.load_shim(str(tmp_path_factory.mktemp("predictivenif")), "exmc_hip_predictive_nif.c")


@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.SV])
def test_nif_equals_the_c_call(hip, mod, kind):
    assert mod.name == "Elixir.Exmc.NUTS.HipPredictiveNative"
    assert mod.table() == [("posterior_predictive", 6, ERL_NIF_DIRTY_JOB_IO_BOUND)]
    spec = PI.spec(kind)
    Cn, S = 5, 3
    draws = np.ascontiguousarray(PI.draws(kind, S, Cn).transpose(2, 0, 1))     # [C][S][d]
    comp = sampler.compile(spec)
    try:
        N = comp.L.exmc_hip_model_n_data(comp.h)
        want = np.zeros((Cn, S, N))
        dp = C.POINTER(C.c_double)
        comp.check(comp.L.exmc_hip_posterior_predictive_host(comp.h, _lib.PredictiveOpts(19, 2, 0), draws.ctypes.data_as(dp),
                                                             S, spec.d, Cn, None, want.ctypes.data_as(dp)))
    finally:
        comp.close()
    got = mod.call("posterior_predictive", H.tuple_term(mod, spec.kind, spec.data), draws, Cn, S, 19, 2)
    assert got == want.tobytes()
    assert np.isfinite(want).all() and len(np.unique(want)) > Cn * S


def test_nif_refusals(hip, mod):
    spec = PI.spec(models.EIGHT_SCHOOLS)
    draws = np.zeros((2, 3, spec.d))
    model = lambda: H.tuple_term(mod, spec.kind, spec.data)   # noqa: E731
    with pytest.raises(H.BadArg):                       # a list is not the {kind, data} tuple
        mod.call("posterior_predictive", [spec.kind, spec.data], draws, 2, 3, 19, 0)
    with pytest.raises(H.BadArg):                       # a 3-tuple neither
        mod.call("posterior_predictive", H.tuple_term(mod, spec.kind, spec.data, 1), draws, 2, 3, 19, 0)
    with pytest.raises(H.BadArg):                       # a trace of another size
        mod.call("posterior_predictive", model(), draws[:, :, :5], 2, 3, 19, 0)
    with pytest.raises(H.BadArg):                       # a negative chain_lo
        mod.call("posterior_predictive", model(), draws, 2, 3, 19, -1)
    with pytest.raises(H.BadArg):                       # no chains
        mod.call("posterior_predictive", model(), draws, 0, 3, 19, 0)
    with pytest.raises(H.Raised) as e:                  # a kind the library has no handle for: {:exmc_hip_error, 4, _}
        mod.call("posterior_predictive", H.tuple_term(mod, models.STD_NORMAL, np.zeros(0)), np.zeros(2 * 3 * 2), 2, 3, 19, 0)
    assert e.value.reason[:2] == (H.Atom("exmc_hip_error"), 4)
