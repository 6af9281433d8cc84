"""`Elixir.Exmc.NUTS.HipPpcNative.ppc/6` (c_src/exmc_hip_ppc_nif.c) called through
tests/host/fake_erl_nif.c, as the BEAM would call it: its table is its one function; equal to
exmc_hip_ppc_host byte for byte; a wrong tuple is a badarg; a kind without a handle raises
{:exmc_hip_error, 4, _}."""
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
    return H.load_shim(str(tmp_path_factory.mktemp("ppcnif")), "exmc_hip_ppc_nif.c")


@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.SV])
def test_nif_equals_the_c_call(hip, mod, kind):
    assert mod.name == "Elixir.Exmc.NUTS.HipPpcNative"
    assert mod.table() == [("ppc", 6, ERL_NIF_DIRTY_JOB_IO_BOUND)]
    spec = PI.spec(kind)
    Cn, S = 5, 3
    draws = np.ascontiguousarray(PI.draws(kind, S, Cn).transpose(2, 0, 1))     # [C][S][d]
    comp = sampler.compile(spec)
    try:
        N = comp.L.exmc_hip_model_n_data(comp.h)
        datum, t_obs, pv = np.zeros((N, 4)), np.zeros(4), np.zeros(4)
        dp = C.POINTER(C.c_double)
        comp.check(comp.L.exmc_hip_ppc_host(comp.h, _lib.PredictiveOpts(19, 2, 0), draws.ctypes.data_as(dp), S, spec.d, Cn,
                                            datum.ctypes.data_as(dp), t_obs.ctypes.data_as(dp), pv.ctypes.data_as(dp), None))
    finally:
        comp.close()
    got = mod.call("ppc", H.tuple_term(mod, spec.kind, spec.data), draws, Cn, S, 19, 2)
    assert got == (datum.tobytes(), t_obs.tobytes(), pv.tobytes())
    assert np.isfinite(datum).all() and len(np.unique(datum[:, 0])) == N and (pv > 0.0).any()


def test_nif_refusals(hip, mod):
    spec = PI.spec(models.EIGHT_SCHOOLS)
    draws = np.zeros((2, 3, spec.d))
    model = lambda: H.tuple_term(mod, spec.kind, spec.data)   # noqa: E731
    with pytest.raises(H.BadArg):                       # a list is not the {kind, data} tuple
        mod.call("ppc", [spec.kind, spec.data], draws, 2, 3, 19, 0)
    with pytest.raises(H.BadArg):                       # a 3-tuple neither
        mod.call("ppc", H.tuple_term(mod, spec.kind, spec.data, 1), draws, 2, 3, 19, 0)
    with pytest.raises(H.BadArg):                       # a trace of another size
        mod.call("ppc", model(), draws[:, :, :5], 2, 3, 19, 0)
    with pytest.raises(H.BadArg):                       # a negative chain_lo
        mod.call("ppc", model(), draws, 2, 3, 19, -1)
    with pytest.raises(H.BadArg):                       # no chains
        mod.call("ppc", model(), draws, 0, 3, 19, 0)
    with pytest.raises(H.Raised) as e:                  # a kind the library has no handle for: {:exmc_hip_error, 4, _}
        mod.call("ppc", H.tuple_term(mod, models.STD_NORMAL, np.zeros(0)), np.zeros(2 * 3 * 2), 2, 3, 19, 0)
    assert e.value.reason[:2] == (H.Atom("exmc_hip_error"), 4)
