"""libexmc_hip.so and a generated model's plug-in in one process: each carries its own copy of the
model-free unit (exmc_amd/csrc/exmc_common.hip -- the diagnostics launches, the native-tree seam, the
last-error string). The same calls in turn through both must give the checker's bits from each, time
their own kernels and keep their own error text."""
import ctypes as C

import numpy as np
import pytest
import torch

import gen_models as GM
import oracle as O
from exmc_amd import _lib, codegen as cg, models, sampler

pytestmark = pytest.mark.gpu

S, D, CN = 16, 2, 8      # 8 chains x 16 draws of the two free variables


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_model_free_calls_from_both_libraries_in_turn(hip):
    base = sampler.compile(models.simple())
    twin = sampler.compile(cg.compile_ir(GM.simple_ir(), name="gen_simple", default_init={"mu": 2.0, "sigma": 1.0}))
    assert base.L is hip and twin.L is not hip
    rng = np.random.default_rng(2)
    x = np.zeros((S, D, CN))
    e = rng.normal(size=(S, D, CN))
    x[0] = e[0]
    for i in range(1, S):
        x[i] = rng.uniform(0.0, 0.9, size=(D, CN)) * x[i - 1] + e[i]
    ref = O.lib()
    want = {"exmc_hip_ess": np.zeros((D, CN)), "exmc_hip_ess_bulk": np.zeros((D, CN)), "exmc_hip_rhat": np.zeros(D)}
    for dim in range(D):
        chains = np.ascontiguousarray(x[:, dim, :].T)
        want["exmc_hip_rhat"][dim] = ref.exo_rhat(O.dptr(chains), CN, S)
        for c in range(CN):
            want["exmc_hip_ess"][dim, c] = ref.exo_ess(O.dptr(np.ascontiguousarray(chains[c])), S)
            want["exmc_hip_ess_bulk"][dim, c] = ref.exo_ess_bulk_mode(O.dptr(np.ascontiguousarray(chains[c])), S, 1)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    q = np.ascontiguousarray(rng.normal(size=(CN, D)))
    p = np.ascontiguousarray(rng.normal(size=(CN, D)))
    g = np.ascontiguousarray(rng.normal(size=(CN, D)))
    lp = np.ascontiguousarray(rng.normal(size=CN))
    for name in ("exmc_hip_ess", "exmc_hip_ess_bulk", "exmc_hip_rhat"):
        for comp in (base, twin):
            out = torch.full(want[name].shape, -1.0, dtype=torch.float64, device="cuda:0")
            comp.check(getattr(comp.L, name)(comp.h, xd.data_ptr(), S, D, CN, out.data_ptr()))
            assert np.array_equal(out.cpu().numpy(), want[name]), (name, comp is twin)
            assert comp.L.exmc_hip_last_kernel_ms(comp.h) > 0.0, (name, comp is twin)
    for comp in (base, twin):
        t = C.c_void_p()
        comp.check(comp.L.exmc_hip_traj_create(0, CN, D, _dp(q), _dp(p), _dp(g), _dp(lp), C.byref(t)))
        # Trajectory::new: the proposal is the start state, nothing accumulated
        q2, g2, lp2, acc = np.zeros((CN, D)), np.zeros((CN, D)), np.zeros(CN), np.ones(CN)
        n, div, dep = (np.ones(CN, dtype=np.int32) for _ in range(3))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
        comp.check(comp.L.exmc_hip_traj_get_result_host(t, _dp(q2), _dp(lp2), _dp(g2), ip(n), ip(div), _dp(acc), ip(dep)))
        comp.L.exmc_hip_traj_destroy(t)
        assert np.array_equal(q2, q) and np.array_equal(g2, g) and np.array_equal(lp2, lp)
        assert not n.any() and not div.any() and not dep.any() and not acc.any()
    # an error in one library's model-free unit is that library's alone
    assert twin.L.exmc_hip_traj_create(0, 0, D, _dp(q), _dp(p), _dp(g), _dp(lp), C.byref(C.c_void_p())) == _lib.ERR_BADARG
    assert hip.exmc_hip_leapfrog_chain_normal_host(0, CN, 0, _dp(q), _dp(p), _dp(g), 1, 0.1, 0.0, 1.0,
                                                   None, None, None, None) == _lib.ERR_BADARG
    assert hip.exmc_hip_last_error().startswith(b"leapfrog_chain_normal:")
    assert hip.exmc_hip_model_create(0, 0, None, 0, 99, C.byref(C.c_void_p())) == _lib.ERR_BADARG
    assert hip.exmc_hip_last_error() == b"device index out of range"
    assert twin.L.exmc_hip_last_error() == b"bad arguments"
