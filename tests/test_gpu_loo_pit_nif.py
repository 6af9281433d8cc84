"""`Elixir.Exmc.NUTS.HipLooPitNative.loo_pit/6` (c_src/exmc_hip_loo_pit_nif.c) called through
tests/host/fake_erl_nif.c, as the BEAM would call it: its table is its one function; equal to
exmc_hip_loo_pit_host byte for byte; a wrong tuple is a badarg; a kind without a handle raises
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
    return H.load_shim(str(tmp_path_factory.mktemp("loopitnif")), "exmc_hip_loo_pit_nif.c")


@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.SV])
def test_nif_equals_the_c_call(hip, mod, kind):
    assert mod.name == "Elixir.Exmc.NUTS.HipLooPitNative"
    assert mod.table() == [("loo_pit", 6, ERL_NIF_DIRTY_JOB_IO_BOUND)]
    spec = PI.spec(kind)
    Cn, S = 70, 3
    draws = np.ascontiguousarray(PI.draws(kind, S, Cn).transpose(2, 0, 1))     # [C][S][d]
    comp = sampler.compile(spec)
    try:
        N = comp.L.exmc_hip_model_n_data(comp.h)
        out = np.zeros((4, N))
        dp = C.POINTER(C.c_double)
        comp.check(comp.L.exmc_hip_loo_pit_host(comp.h, _lib.PredictiveOpts(19, 2, 0), draws.ctypes.data_as(dp), S, spec.d,
                                                Cn, 0, out.ctypes.data_as(dp)))
    finally:
        comp.close()
    got = mod.call("loo_pit", H.tuple_term(mod, spec.kind, spec.data), draws, Cn, S, 19, 2)
    assert got == out.tobytes()
    assert np.isfinite(out).all() and len(np.unique(out[2])) == N and ((out[2] > 0.0) & (out[2] < 1.0)).all()


def test_nif_refusals(hip, mod):
    spec = PI.spec(models.EIGHT_SCHOOLS)
    draws = np.zeros((2, 3, spec.d))
    model = lambda: H.tuple_term(mod, spec.kind, spec.data)   # noqa: E731
    with pytest.raises(H.BadArg):                       # a list is not the {kind, data} tuple
        mod.call("loo_pit", [spec.kind, spec.data], draws, 2, 3, 19, 0)
    with pytest.raises(H.BadArg):                       # a 3-tuple neither
        mod.call("loo_pit", H.tuple_term(mod, spec.kind, spec.data, 1), draws, 2, 3, 19, 0)
    with pytest.raises(H.BadArg):                       # a trace of another size
        mod.call("loo_pit", model(), draws[:, :, :5], 2, 3, 19, 0)
    with pytest.raises(H.BadArg):                       # a negative chain_lo
        mod.call("loo_pit", model(), draws, 2, 3, 19, -1)
    with pytest.raises(H.BadArg):                       # no chains
        mod.call("loo_pit", model(), draws, 0, 3, 19, 0)
    with pytest.raises(H.BadArg):                       # one sample: the library's EXMC_ERR_BADARG is a badarg too
        mod.call("loo_pit", model(), np.zeros((1, 1, spec.d)), 1, 1, 19, 0)
    with pytest.raises(H.Raised) as e:                  # a kind the library has no handle for: {:exmc_hip_error, 4, _}
        mod.call("loo_pit", H.tuple_term(mod, models.STD_NORMAL, np.zeros(0)), np.zeros(2 * 3 * 2), 2, 3, 19, 0)
    assert e.value.reason[:2] == (H.Atom("exmc_hip_error"), 4)
