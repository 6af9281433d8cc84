"""Posterior predictive checks on the device (exmc_amd/csrc/exmc_ppc.hpp, include/exmc_hip_ppc.h,
exmc_amd/predictive.py ppc) against the statement of the contract (tests/ppc_statement.py) applied to the
statement's replicates (tests/predictive_statement.py), byte for byte: every built-in kind on two
wavefronts (the second with 6 chains, so that lanes without a chain own datums); one chain and one draw;
a full wavefront; sharding at 64 chains; without the tstat output; the host form and the Python call;
hostile rows, against the statement applied to the device's own replicates; refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import ppc_statement as PPC
import predictive_inputs as PI
import predictive_statement as PS
import test_gpu_predictive as TP
from exmc_amd import _lib, models
from exmc_amd import predictive as PP

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)


def observed(kind):
    return PPC.observed(kind, PI.spec(kind).data)


def device_call(cm, x, seed, chain_lo, tstat=True):
    """exmc_hip_ppc on the host array x [S][d][C] -> the raw outputs, every buffer poisoned before the call"""
    S, d, Cn = x.shape
    N = cm.L.exmc_hip_model_n_data(cm.h)
    B = (Cn + 63) // 64
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    sums = torch.full((B, N, 2), float("nan"), dtype=torch.float64, device="cuda")
    counts = torch.full((B, N, 2), -7, dtype=torch.int64, device="cuda")
    cc = torch.full((4, Cn), -7, dtype=torch.int32, device="cuda")
    ts = torch.full((S, 4, Cn), float("nan"), dtype=torch.float64, device="cuda") if tstat else None
    t_obs, m0, y = np.full(4, np.nan), np.full(1, np.nan), np.full(N, np.nan)
    torch.cuda.synchronize()
    cm.check(cm.L.exmc_hip_ppc(cm.h, _lib.PredictiveOpts(seed, chain_lo, 0), xd.data_ptr(), S, d, Cn, sums.data_ptr(),
                               counts.data_ptr(), cc.data_ptr(), None if ts is None else ts.data_ptr(),
                               t_obs.ctypes.data_as(DP), m0.ctypes.data_as(DP), y.ctypes.data_as(DP)))
    return dict(sums=sums.cpu().numpy(), counts=counts.cpu().numpy(), chain_counts=cc.cpu().numpy(),
                tstat=None if ts is None else ts.cpu().numpy(), t_obs=t_obs, m0=float(m0[0]), y=y)


RAW = ("sums", "counts", "chain_counts", "tstat", "t_obs")


def assert_raw_equal(got, want, keys=RAW):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, np.argwhere(got[k] != want[k])[:5])


_want = {}


def want_parity(kind):
    if kind not in _want:
        x, yrep = PI.expected(kind)[:2]
        _want[kind] = (x, PPC.run(yrep, observed(kind)))
    return _want[kind]


@pytest.mark.parametrize("kind", PI.KINDS)
def test_parity_with_the_statement(kind, hip):
    x, want = want_parity(kind)
    assert x.shape[2] == 70 and x.shape[0] == 3 and want["sums"].shape[0] == 2
    cm = TP.comp(kind)
    got = device_call(cm, x, PI.SEED, PI.CHAIN_LO)
    assert cm.last_kernel_ms > 0.0
    assert got["y"].tobytes() == observed(kind).tobytes() and got["m0"] == want["m0"]
    assert_raw_equal(got, want)


@pytest.mark.parametrize("Cn,S", [(1, 1), (64, 2)])
def test_small_shapes(Cn, S, hip):
    """eight_schools, whose one group of datums is partial: one chain and one draw; exactly one wavefront"""
    kind = models.EIGHT_SCHOOLS
    x = PI.draws(kind, S, Cn)
    yrep = PS.run(kind, PI.spec(kind).data, x, seed=5, chain_lo=3)[0]
    want = PPC.run(yrep, observed(kind))
    assert_raw_equal(device_call(TP.comp(kind), x, 5, 3), want)


@pytest.mark.parametrize("kind", PI.KINDS)
def test_sharding_at_64_chains(kind, hip):
    x, _ = want_parity(kind)
    cm = TP.comp(kind)
    whole = device_call(cm, x, PI.SEED, PI.CHAIN_LO)
    lo = device_call(cm, x[:, :, :64], PI.SEED, PI.CHAIN_LO)
    hi = device_call(cm, x[:, :, 64:], PI.SEED, PI.CHAIN_LO + 64)
    for k in ("sums", "counts"):
        assert lo[k].tobytes() == whole[k][:1].tobytes() and hi[k].tobytes() == whole[k][1:].tobytes(), k
    assert np.concatenate([lo["chain_counts"], hi["chain_counts"]], axis=1).tobytes() == whole["chain_counts"].tobytes()
    assert np.concatenate([lo["tstat"], hi["tstat"]], axis=2).tobytes() == whole["tstat"].tobytes()
    assert lo["t_obs"].tobytes() == whole["t_obs"].tobytes() == hi["t_obs"].tobytes()


@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.LOGISTIC])
def test_without_tstat_the_other_outputs_are_unchanged(kind, hip):
    x, want = want_parity(kind)
    got = device_call(TP.comp(kind), x, PI.SEED, PI.CHAIN_LO, tstat=False)
    assert got["tstat"] is None
    assert_raw_equal(got, want, keys=("sums", "counts", "chain_counts", "t_obs"))


def host_call(cm, x, seed, chain_lo, tstat=True):
    """exmc_hip_ppc_host on x [S][d][C], handed over as [C][S][d]"""
    S, d, Cn = x.shape
    N = cm.L.exmc_hip_model_n_data(cm.h)
    host_in = np.ascontiguousarray(x.transpose(2, 0, 1))
    datum, t_obs, p_value = np.full((N, 4), np.nan), np.full(4, np.nan), np.full(4, np.nan)
    ts = np.full((Cn, S, 4), np.nan) if tstat else None
    cm.check(cm.L.exmc_hip_ppc_host(cm.h, _lib.PredictiveOpts(seed, chain_lo, 0), host_in.ctypes.data_as(DP), S, d, Cn,
                                    datum.ctypes.data_as(DP), t_obs.ctypes.data_as(DP), p_value.ctypes.data_as(DP),
                                    None if ts is None else ts.ctypes.data_as(DP)))
    return host_in, datum, t_obs, p_value, ts


def assert_finished(datum, t_obs, p_value, py, want):
    """the host form's numbers == the Python call's == the statement's finished numbers, byte for byte"""
    for j, k in enumerate(("mean", "var", "p_lt", "p_eq")):
        assert np.ascontiguousarray(datum[:, j]).tobytes() == py[k].tobytes() == want[k].tobytes(), k
    assert py["pit"].tobytes() == want["pit"].tobytes()
    assert t_obs.tobytes() == want["t_obs"].tobytes() == np.array([py["t_obs"][k] for k in PP.PPC_STATS]).tobytes()
    assert p_value.tobytes() == want["p_value"].tobytes() == np.array([py["p_value"][k] for k in PP.PPC_STATS]).tobytes()
    assert list(py["t_obs"]) == list(py["p_value"]) == ["mean", "var", "min", "max"]


@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.SV_NCP, models.RADON])
def test_host_form_and_python_call(kind, hip):
    x, want = want_parity(kind)
    cm = TP.comp(kind)
    host_in, datum, t_obs, p_value, ts = host_call(cm, x, PI.SEED, PI.CHAIN_LO)
    py = PP.ppc(cm, torch.from_numpy(x).cuda(), seed=PI.SEED, chain_lo=PI.CHAIN_LO, tstat=True)
    assert_finished(datum, t_obs, p_value, py, want)
    assert ts.tobytes() == np.ascontiguousarray(want["tstat"].transpose(2, 0, 1)).tobytes()
    assert py["tstat"].cpu().numpy().tobytes() == want["tstat"].tobytes()
    # the names in the handle's order, as posterior_predictive returns them
    assert py["names"] == PP.posterior_predictive(cm, torch.from_numpy(x).cuda())[1] and len(py["names"]) == datum.shape[0]
    if kind == models.RADON:
        assert py["names"][0] == ("radon", int(PI.spec(kind).datum_order[0]))
    # a host trace [C][S][d], no tstat asked for
    py2 = PP.ppc(cm, host_in, seed=PI.SEED, chain_lo=PI.CHAIN_LO)
    assert "tstat" not in py2
    _, datum2, t_obs2, p_value2, ts2 = host_call(cm, x, PI.SEED, PI.CHAIN_LO, tstat=False)
    assert ts2 is None and datum2.tobytes() == datum.tobytes()
    assert_finished(datum2, t_obs2, p_value2, py2, want)


@pytest.mark.parametrize("kind", PI.KINDS)
def test_hostile_rows(kind, hip):
    """the statement applied to the device's own replicates of a trace no sampler would write"""
    x = PI.hostile(kind)
    cm = TP.comp(kind)
    yrep, _ = TP.device_call(cm, x, PI.SEED, PI.CHAIN_LO)
    want = PPC.run(yrep, observed(kind))
    got = device_call(cm, x, PI.SEED, PI.CHAIN_LO)               # ... and the call returns
    for k in ("counts", "chain_counts"):
        assert got[k].tobytes() == want[k].tobytes(), k
    for k in ("sums", "tstat"):
        g, w = got[k], want[k]
        fin = np.isfinite(w)
        assert (np.isfinite(g) == fin).all(), k
        assert g[fin].tobytes() == w[fin].tobytes(), k
        assert (np.isnan(g) == np.isnan(w)).all(), k
        inf = ~fin & ~np.isnan(w)
        assert (g[inf] == w[inf]).all(), k                        # the infinities and their signs
    assert got["t_obs"].tobytes() == want["t_obs"].tobytes()
    if kind != models.LOGISTIC:                                   # (a Bernoulli replicate of a NaN p is 0.0)
        assert not np.isfinite(want["sums"]).all() and not np.isfinite(want["tstat"]).all()


def test_refusals(hip):
    cm = TP.comp(models.SIMPLE)
    x = PI.draws(models.SIMPLE, S=2, Cn=3)
    S, d, Cn = x.shape
    N = 10
    xd = torch.from_numpy(x).cuda()
    sums = torch.zeros((1, N, 2), dtype=torch.float64, device="cuda")
    counts = torch.zeros((1, N, 2), dtype=torch.int64, device="cuda")
    cc = torch.zeros((4, Cn), dtype=torch.int32, device="cuda")
    t_obs, m0 = np.zeros(4), np.zeros(1)
    torch.cuda.synchronize()
    L, O = cm.L, _lib.PredictiveOpts
    f = L.exmc_hip_ppc
    X, SU, CO, CC, T, M = xd.data_ptr(), sums.data_ptr(), counts.data_ptr(), cc.data_ptr(), t_obs.ctypes.data_as(DP), \
        m0.ctypes.data_as(DP)
    assert f(cm.h, O(1, 0, 0), X, S, d, Cn, SU, CO, CC, None, T, M, None) == _lib.OK
    bad = [(cm.h, O(1, 0, 0), None, S, d, Cn, SU, CO, CC, None, T, M, None),       # no trace
           (cm.h, O(1, 0, 0), X, S, d, Cn, None, CO, CC, None, T, M, None),        # a required output missing
           (cm.h, O(1, 0, 0), X, S, d, Cn, SU, None, CC, None, T, M, None),
           (cm.h, O(1, 0, 0), X, S, d, Cn, SU, CO, None, None, T, M, None),
           (cm.h, O(1, 0, 0), X, S, d, Cn, SU, CO, CC, None, None, M, None),
           (cm.h, O(1, 0, 0), X, S, d, Cn, SU, CO, CC, None, T, None, None),
           (cm.h, O(1, 0, 0), X, S, d + 1, Cn, SU, CO, CC, None, T, M, None),
           (cm.h, O(1, 0, 0), X, 0, d, Cn, SU, CO, CC, None, T, M, None),
           (cm.h, O(1, 0, 0), X, S, d, 0, SU, CO, CC, None, T, M, None),
           (cm.h, O(1, -1, 0), X, S, d, Cn, SU, CO, CC, None, T, M, None),
           (cm.h, O(1, 0, 1), X, S, d, Cn, SU, CO, CC, None, T, M, None),          # there is no resume
           (None, O(1, 0, 0), X, S, d, Cn, SU, CO, CC, None, T, M, None)]
    for args in bad:
        assert f(*args) == _lib.ERR_BADARG, args[1:]
    hin, datum, pv = np.zeros((Cn, S, d)), np.zeros((N, 4)), np.zeros(4)
    H, D, P = hin.ctypes.data_as(DP), datum.ctypes.data_as(DP), pv.ctypes.data_as(DP)
    g = L.exmc_hip_ppc_host
    assert g(cm.h, O(1, 0, 0), H, S, d, Cn, D, T, P, None) == _lib.OK
    for args in [(cm.h, O(1, 0, 0), None, S, d, Cn, D, T, P, None), (cm.h, O(1, 0, 0), H, S, d, Cn, None, T, P, None),
                 (cm.h, O(1, 0, 0), H, S, d, Cn, D, None, P, None), (cm.h, O(1, 0, 0), H, S, d, Cn, D, T, None, None),
                 (cm.h, O(1, 0, 0), H, S, d - 1, Cn, D, T, P, None), (cm.h, O(1, 0, 0), H, 0, d, Cn, D, T, P, None),
                 (cm.h, O(1, 0, 0), H, S, d, -1, D, T, P, None), (cm.h, O(1, -3, 0), H, S, d, Cn, D, T, P, None),
                 (cm.h, O(1, 0, 1), H, S, d, Cn, D, T, P, None), (None, O(1, 0, 0), H, S, d, Cn, D, T, P, None)]:
        assert g(*args) == _lib.ERR_BADARG, args[1:]
    with pytest.raises(ValueError):
        PP.ppc(cm, xd.float())


def test_unsupported_models(hip):
    from exmc_amd import codegen, sampler
    # a generated model, compiled WITH its per-datum terms: it has datums for model comparison, none here
    gen = sampler.compile(codegen.compile_ir(codegen.eight_schools_ir(), pointwise=True))
    try:
        assert gen.L.exmc_hip_model_n_data(gen.h) == 8
        for name in _lib.PPC_EXPORTS:
            getattr(gen.L, name)
        xd = torch.zeros((2, gen.d, 3), dtype=torch.float64, device="cuda")
        sums = torch.zeros((1, 8, 2), dtype=torch.float64, device="cuda")
        counts = torch.zeros((1, 8, 2), dtype=torch.int64, device="cuda")
        cc = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
        t_obs, m0 = np.zeros(4), np.zeros(1)
        torch.cuda.synchronize()
        rc = gen.L.exmc_hip_ppc(gen.h, _lib.PredictiveOpts(1, 0, 0), xd.data_ptr(), 2, gen.d, 3, sums.data_ptr(),
                                counts.data_ptr(), cc.data_ptr(), None, t_obs.ctypes.data_as(DP), m0.ctypes.data_as(DP), None)
        assert rc == _lib.ERR_UNSUPPORTED
        assert b"posterior predictive checks" in gen.L.exmc_hip_last_error()
        hin, datum, pv = np.zeros((3, 2, gen.d)), np.zeros((8, 4)), np.zeros(4)
        assert gen.L.exmc_hip_ppc_host(gen.h, _lib.PredictiveOpts(1, 0, 0), hin.ctypes.data_as(DP), 2, gen.d, 3,
                                       datum.ctypes.data_as(DP), t_obs.ctypes.data_as(DP), pv.ctypes.data_as(DP),
                                       None) == _lib.ERR_UNSUPPORTED
        with pytest.raises(_lib.ExmcHipError):
            PP.ppc(gen, xd)
    finally:
        gen.close()
