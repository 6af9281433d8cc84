"""`Elixir.Exmc.NUTS.HipPathfinderNative.fit/9` (c_src/exmc_hip_pathfinder_nif.c) called through
tests/host/fake_erl_nif.c, as the BEAM would call it: equal to exmc_hip_pathfinder_host bit for bit;
a wrong tuple is a badarg; a kind without a compiled layout raises {:exmc_hip_error, 4, _}."""

import numpy as np
import pytest

import nif_harness as H
from exmc_amd import models, pathfinder, sampler

pytestmark = pytest.mark.gpu

ERL_NIF_DIRTY_JOB_IO_BOUND = 2


@pytest.fixture(scope="module")
def mod(tmp_path_factory):
    return H.load_shim(str(tmp_path_factory.mktemp("pathfindernif")), "exmc_hip_pathfinder_nif.c")


@pytest.mark.parametrize("which", ["eight_schools", "sv"])
def test_fit_nif_equals_the_c_call(hip, mod, which):
    assert mod.name == "Elixir.Exmc.NUTS.HipPathfinderNative"
    assert mod.table() == [("fit", 9, ERL_NIF_DIRTY_JOB_IO_BOUND)]
    spec = models.eight_schools() if which == "eight_schools" else models.sv(models.sv_returns())
    comp = sampler.compile(spec)
    try:
        want = pathfinder.fit_raw(comp, dict(num_draws=3, max_iters=7, history_size=4, seed=19, chain_lo=2), 5)
    finally:
        comp.close()
    perm = [int(v) for v in spec.flat_order()]      # sv: the string sort, not the kernel order
    got = mod.call("fit", H.tuple_term(mod, spec.kind, spec.data), perm, 5, 2, 3, 7, 4, 19, 0)
    assert isinstance(got, tuple) and len(got) == 7
    for b, k in zip(got, ("draws", "mu", "sigma", "elbo", "num_iters", "best_index", "status")):
        assert b == np.ascontiguousarray(want[k]).tobytes(), k


def test_fit_nif_refusals(hip, mod):
    spec = models.eight_schools()
    model = lambda: H.tuple_term(mod, spec.kind, spec.data)   # noqa: E731
    with pytest.raises(H.BadArg):                       # a list is not the {kind, data} tuple
        mod.call("fit", [spec.kind, spec.data], [], 2, 0, 3, 7, 4, 19, 0)
    with pytest.raises(H.BadArg):                       # a 3-tuple neither
        mod.call("fit", H.tuple_term(mod, spec.kind, spec.data, 1), [], 2, 0, 3, 7, 4, 19, 0)
    with pytest.raises(H.BadArg):                       # history_size above the bound
        mod.call("fit", model(), [], 2, 0, 3, 7, 7, 19, 0)
    with pytest.raises(H.BadArg):                       # a flat order of the wrong length
        mod.call("fit", model(), [0, 1], 2, 0, 3, 7, 4, 19, 0)
    with pytest.raises(H.Raised) as e:                  # a kind no layout row carries: {:exmc_hip_error, 4, _}
        mod.call("fit", H.tuple_term(mod, models.STD_NORMAL, np.zeros(0)), [], 2, 0, 3, 7, 4, 19, 0)
    assert e.value.reason[:2] == (H.Atom("exmc_hip_error"), 4)
    with pytest.raises(H.Raised) as e:                  # a lane count that is not compiled in
        mod.call("fit", model(), [], 2, 0, 3, 7, 4, 19, 5)
    assert e.value.reason[:2] == (H.Atom("exmc_hip_error"), 4)
