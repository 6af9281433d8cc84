"""`Elixir.Exmc.NUTS.HipPsisNative.psis_stats/4` (c_src/exmc_hip_psis_nif.c) called through
tests/host/fake_erl_nif.c, as the BEAM would call it: equal to exmc_hip_psis_stats_host bit for bit on
draws in the layout HipNative's sampling functions return."""
import ctypes as C

import numpy as np
import pytest

import nif_harness as H
from exmc_amd import models, sampler
from exmc_amd import model_comparison as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod(tmp_path_factory):
    return H.load_shim(str(tmp_path_factory.mktemp("psisnif")), "exmc_hip_psis_nif.c")


def test_psis_stats_nif_equals_the_c_call(hip, mod):
    assert mod.name == "Elixir.Exmc.NUTS.HipPsisNative"
    spec = models.eight_schools()
    comp = sampler.compile(spec)
    _, stats = sampler.sample_chains_compiled(comp, 6, dict(num_warmup=80, num_samples=30, seed=3))
    draws = np.ascontiguousarray(stats[0]["extra"]["raw"]["draws"])       # [C][S][d], kernel order
    model = H.tuple_term(mod, spec.kind, spec.data)
    got = H.f64(mod.call("psis_stats", model, draws, 6, 30)).reshape(3, 8)
    want = np.zeros((3, 8))
    comp.check(comp.L.exmc_hip_psis_stats_host(comp.h, draws.ctypes.data_as(C.POINTER(C.c_double)), 30, spec.d, 6,
                                               0, want.ctypes.data_as(C.POINTER(C.c_double))))
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() == MC.psis_pointwise_stats(comp, draws)[0].tobytes()
    assert np.all(np.isfinite(got))            # n = 180: M = 36, every datum's tail is fitted
    with pytest.raises(H.BadArg):
        mod.call("psis_stats", H.tuple_term(mod, spec.kind, spec.data), draws[:, :, :5], 6, 30)
    with pytest.raises(H.BadArg):                       # a list is not the {kind, data} tuple
        mod.call("psis_stats", [spec.kind, spec.data], draws, 6, 30)
    with pytest.raises(H.Raised) as e:                  # a kind without datums: {:exmc_hip_error, 4, _}
        mod.call("psis_stats", H.tuple_term(mod, models.STD_NORMAL, np.zeros(0)), np.zeros(6 * 30 * 2), 6, 30)
    assert e.value.reason[:2] == (H.Atom("exmc_hip_error"), 4)
