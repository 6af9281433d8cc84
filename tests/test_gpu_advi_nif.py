"""`Elixir.Exmc.NUTS.HipAdviNative.fit/12` (c_src/exmc_hip_advi_nif.c) called through
tests/host/fake_erl_nif.c, as the BEAM would call it: equal to exmc_hip_advi_host bit for bit; a wrong
tuple is a badarg; a kind without a compiled layout raises {:exmc_hip_error, 4, _}."""

import numpy as np
import pytest

import nif_harness as H
from exmc_amd import advi, models, sampler

pytestmark = pytest.mark.gpu

ERL_NIF_DIRTY_JOB_IO_BOUND = 2
KEYS = ("draws", "mu", "log_sigma", "elbo_history", "num_iters", "converged")


@pytest.fixture(scope="module")
def mod(tmp_path_factory):
    return H.load_shim(str(tmp_path_factory.mktemp("advinif")), "exmc_hip_advi_nif.c")


@pytest.mark.parametrize("which", ["eight_schools", "sv"])
def test_fit_nif_equals_the_c_call(hip, mod, which):
    assert mod.name == "Elixir.Exmc.NUTS.HipAdviNative"
    assert mod.table() == [("fit", 12, ERL_NIF_DIRTY_JOB_IO_BOUND)]
    spec = models.eight_schools() if which == "eight_schools" else models.sv(models.sv_returns())
    lr = 0.05 if which == "eight_schools" else 1.0e-3
    comp = sampler.compile(spec)
    try:
        want = advi.fit_raw(comp, dict(num_draws=3, max_iters=15, num_mc_samples=2, window_size=9, learning_rate=lr,
                                       convergence_tol=0.02, seed=19, chain_lo=2), 5)
    finally:
        comp.close()
    perm = [int(v) for v in spec.flat_order()]      # sv: the string sort, not the kernel order
    got = mod.call("fit", H.tuple_term(mod, spec.kind, spec.data), perm, 5, 2, 3, 15, 2, 9, lr, 0.02, 19, 0)
    assert isinstance(got, tuple) and len(got) == 6
    for b, k in zip(got, KEYS):
        assert b == np.ascontiguousarray(want[k]).tobytes(), k


def test_fit_nif_refusals(hip, mod):
    spec = models.eight_schools()
    model = lambda: H.tuple_term(mod, spec.kind, spec.data)   # noqa: E731
    with pytest.raises(H.BadArg):                       # a list is not the {kind, data} tuple
        mod.call("fit", [spec.kind, spec.data], [], 2, 0, 3, 7, 1, 4, 0.01, 1e-4, 19, 0)
    with pytest.raises(H.BadArg):                       # a 3-tuple neither
        mod.call("fit", H.tuple_term(mod, spec.kind, spec.data, 1), [], 2, 0, 3, 7, 1, 4, 0.01, 1e-4, 19, 0)
    with pytest.raises(H.BadArg):                       # window_size below the bound
        mod.call("fit", model(), [], 2, 0, 3, 7, 1, 1, 0.01, 1e-4, 19, 0)
    with pytest.raises(H.BadArg):                       # no samples
        mod.call("fit", model(), [], 2, 0, 3, 7, 0, 4, 0.01, 1e-4, 19, 0)
    with pytest.raises(H.BadArg):                       # a flat order of the wrong length
        mod.call("fit", model(), [0, 1], 2, 0, 3, 7, 1, 4, 0.01, 1e-4, 19, 0)
    with pytest.raises(H.Raised) as e:                  # a kind no layout row carries: {:exmc_hip_error, 4, _}
        mod.call("fit", H.tuple_term(mod, models.STD_NORMAL, np.zeros(0)), [], 2, 0, 3, 7, 1, 4, 0.01, 1e-4, 19, 0)
    assert e.value.reason[:2] == (H.Atom("exmc_hip_error"), 4)
    with pytest.raises(H.Raised) as e:                  # a lane count that is not compiled in
        mod.call("fit", model(), [], 2, 0, 3, 7, 1, 4, 0.01, 1e-4, 19, 5)
    assert e.value.reason[:2] == (H.Atom("exmc_hip_error"), 4)
