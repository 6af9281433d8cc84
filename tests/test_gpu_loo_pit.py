"""PSIS-LOO-PIT on the device (exmc_amd/csrc/exmc_loo_pit.hpp, include/exmc_hip_loo_pit.h,
exmc_amd/predictive.py loo_pit) against the host statement of the contract (tests/host/loo_pit_host_checker.c)
fed the host's pointwise terms (tests/ic_checker.py) and the statement's replicates
(tests/predictive_statement.py), byte for byte: every built-in kind on two wavefronts (the second with 6
chains); one chain, one full wavefront and three blocks to merge; datum blocks of the first pass; the
model-free route fed the device's own matrices; the host form and the Python calls; hostile rows, against
the checker fed the device's own matrices; ties; refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import ic_checker as IC
import loo_pit_checker as LC
import ppc_statement as PPC
import predictive_inputs as PI
import predictive_statement as PS
import test_gpu_predictive as TP
from exmc_amd import _lib, models
from exmc_amd import model_comparison as MC
from exmc_amd import predictive as PP

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)


def observed(kind):
    return PPC.observed(kind, PI.spec(kind).data)


def device_call(cm, x, seed, chain_lo, scratch_bytes=0):
    """exmc_hip_loo_pit on the host array x [S][d][C] -> out [4][N], the buffer poisoned before the call"""
    S, d, Cn = x.shape
    N = cm.L.exmc_hip_model_n_data(cm.h)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.full((4, N), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    cm.check(cm.L.exmc_hip_loo_pit(cm.h, _lib.PredictiveOpts(seed, chain_lo, 0), xd.data_ptr(), S, d, Cn, scratch_bytes,
                                   out.data_ptr()))
    return out.cpu().numpy()


def from_ll_call(ll, yrep, y, L=None):
    """exmc_hip_loo_pit_from_ll on host or device matrices [S][N][C] and y [N] -> (rc, out [4][N])"""
    lld = ll if isinstance(ll, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ll)).cuda()
    vd = yrep if isinstance(yrep, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(yrep)).cuda()
    yd = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    S, N, Cn = lld.shape
    out = torch.full((4, N), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = (L or _lib.load()).exmc_hip_loo_pit_from_ll(0, lld.data_ptr(), vd.data_ptr(), yd.data_ptr(), S, N, Cn,
                                                     out.data_ptr())
    return rc, out.cpu().numpy()


def checker(kind, x, seed, chain_lo, tails=False):
    """the host statement on the host's terms and the statement's replicates of the trace x [S][d][C]"""
    blob = PI.spec(kind).data
    yrep = PS.run(kind, blob, x, seed=seed, chain_lo=chain_lo)[0]
    return LC.run(IC.pointwise(kind, blob, x), yrep, observed(kind), tails=tails)


def assert_same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5]


_want = {}


def want_parity(kind):
    """(x, out [4][N], T [N], the plain PIT) on the parity trace, computed once"""
    if kind not in _want:
        x, yrep = PI.expected(kind)[:2]
        y = observed(kind)
        assert np.isfinite(yrep).all()
        out, T = LC.run(IC.pointwise(kind, PI.spec(kind).data, x), yrep, y, tails=True)
        _want[kind] = (x, out, T, PPC.run(yrep, y)["pit"])
    return _want[kind]


@pytest.mark.parametrize("kind", PI.KINDS)
def test_parity_with_the_checker(kind, hip):
    x, want, T, plain = want_parity(kind)
    assert x.shape[2] == 70 and x.shape[0] == 3
    # every datum is smoothed, from a full tail (M = 42), with a finite k
    assert np.all(T == 42) and np.isfinite(want).all()
    assert np.any(want[2] != plain)                   # ... and LOO-PIT is not the plain PIT
    if kind == models.LOGISTIC:
        assert np.all(want[1] > 0)                    # ties: every datum has replicates equal to it
    cm = TP.comp(kind)
    got = device_call(cm, x, PI.SEED, PI.CHAIN_LO)
    assert cm.last_kernel_ms > 0.0
    assert_same(got, want)


@pytest.mark.parametrize("Cn,S", [(1, 2), (64, 2), (130, 5)])
@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.SV, models.RADON])
def test_shapes(kind, Cn, S, hip):
    """one chain (n = 2: nothing smoothed), exactly one wavefront, three blocks to merge with the last of
    two chains; one partial datum group (eight_schools), two with the second of 36 (sv), 15 (radon)"""
    x = PI.draws(kind, S, Cn)
    want, T = checker(kind, x, 5, 3, tails=True)
    if Cn == 1:
        assert np.all(T <= 1) and np.all(np.isposinf(want[3])) and np.isfinite(want[:3]).all()
    else:
        assert np.all(T > 4)
    assert_same(device_call(TP.comp(kind), x, 5, 3), want)


@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.SV_NCP, models.LOGISTIC])
def test_datum_blocks_of_the_first_pass(kind, hip):
    """scratch_bytes for three datum blocks, the last partial, and for one datum at a time: the default's bytes"""
    x, want = want_parity(kind)[:2]
    cm = TP.comp(kind)
    N = want.shape[1]
    Nb = (N + 2) // 3
    assert (N + Nb - 1) // Nb == 3 and N % Nb != 0
    per = x.shape[0] * x.shape[2] * 8
    assert_same(device_call(cm, x, PI.SEED, PI.CHAIN_LO, scratch_bytes=Nb * per), want)
    assert_same(device_call(cm, x, PI.SEED, PI.CHAIN_LO, scratch_bytes=1), want)


def host_call(cm, x, seed, chain_lo, scratch_bytes=0):
    """exmc_hip_loo_pit_host on x [S][d][C], handed over as [C][S][d]"""
    S, d, Cn = x.shape
    N = cm.L.exmc_hip_model_n_data(cm.h)
    host_in = np.ascontiguousarray(x.transpose(2, 0, 1))
    out = np.full((4, N), -7.0)
    cm.check(cm.L.exmc_hip_loo_pit_host(cm.h, _lib.PredictiveOpts(seed, chain_lo, 0), host_in.ctypes.data_as(DP), S, d, Cn,
                                        scratch_bytes, out.ctypes.data_as(DP)))
    return host_in, out


@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.SV_NCP, models.LOGISTIC])
def test_two_routes_host_form_and_python_calls(kind, hip):
    """the fused call == the model-free call on the device's own pointwise and replicate matrices == the
    host form == the Python calls"""
    x, want = want_parity(kind)[:2]
    cm = TP.comp(kind)
    xd = torch.from_numpy(x).cuda()
    fused = device_call(cm, x, PI.SEED, PI.CHAIN_LO)
    ll, names = MC.pointwise_log_likelihood(cm, xd)
    yrep, names2 = PP.posterior_predictive(cm, xd, seed=PI.SEED, chain_lo=PI.CHAIN_LO)
    assert names == names2
    rc, free = from_ll_call(ll, yrep, observed(kind))
    assert rc == _lib.OK
    assert_same(free, fused)
    assert_same(fused, want)
    host_in, hosted = host_call(cm, x, PI.SEED, PI.CHAIN_LO)
    assert_same(hosted, fused)
    n = x.shape[0] * x.shape[2]
    for py in (PP.loo_pit(cm, xd, seed=PI.SEED, chain_lo=PI.CHAIN_LO),
               PP.loo_pit(cm, host_in, seed=PI.SEED, chain_lo=PI.CHAIN_LO, scratch_bytes=1),
               PP.loo_pit_from_pointwise(ll, yrep, observed(kind), names=names),
               PP.loo_pit_from_pointwise(ll.cpu().numpy(), yrep.cpu().numpy(), torch.from_numpy(observed(kind)), names)):
        assert list(py) == ["names", "p_lt", "p_eq", "pit", "k", "k_threshold", "n_high_k"]
        assert py["names"] == names
        for j, key in enumerate(_lib.LOO_PIT_ROWS):
            assert py[key].tobytes() == np.ascontiguousarray(fused[j]).tobytes(), key
        assert py["k_threshold"] == MC.k_threshold(n) and py["n_high_k"] == int(np.sum(~(fused[3] <= MC.k_threshold(n))))
    assert PP.loo_pit_from_pointwise(ll, yrep, observed(kind))["names"] == list(range(want.shape[1]))
    # k is PSIS-LOO's, bit for bit (the handle's order against the caller's)
    psis = MC.psis_loo(cm, xd)["pointwise"]["pareto_k"]
    assert psis[MC._datum_order(cm, want.shape[1])].tobytes() == np.ascontiguousarray(fused[3]).tobytes()


@pytest.mark.parametrize("kind", PI.KINDS)
def test_hostile_rows(kind, hip):
    """a trace no sampler would write: the call returns, a datum with a non-finite term is NaN in all four
    rows and no other is, and the numbers are the checker's on the device's own terms and replicates"""
    x = PI.hostile(kind)
    cm = TP.comp(kind)
    xd = torch.from_numpy(x).cuda()
    ll = MC.pointwise_log_likelihood(cm, xd)[0].cpu().numpy()
    yrep, _ = TP.device_call(cm, x, PI.SEED, PI.CHAIN_LO)
    want = LC.run(ll, yrep, observed(kind))
    got = device_call(cm, x, PI.SEED, PI.CHAIN_LO)
    affected = ~np.isfinite(ll).all(axis=(0, 2))
    assert np.isnan(got[:, affected]).all() and not np.isnan(got[:3, ~affected]).any()
    assert_same(got, want)
    rc, free = from_ll_call(ll, yrep, observed(kind))
    assert rc == _lib.OK
    assert_same(free, want)


def test_a_hostile_dimension_voids_its_datums_alone(hip):
    """eight_schools: theta_3 NaN in one sample and theta_5 +inf in another (second wavefront) void datums
    3 and 5; a NaN replicate of datum 1 (a scale no sampler would write is not needed: the model-free
    route takes it) counts in neither set"""
    kind = models.EIGHT_SCHOOLS
    x = PI.draws(kind, 3, 70)
    x[1, 2 + 3, 7] = np.nan
    x[0, 2 + 5, 66] = np.inf
    cm = TP.comp(kind)
    xd = torch.from_numpy(x).cuda()
    ll = MC.pointwise_log_likelihood(cm, xd)[0].cpu().numpy()
    yrep, _ = TP.device_call(cm, x, 11, 0)
    want = LC.run(ll, yrep, observed(kind))
    got = device_call(cm, x, 11, 0)
    assert_same(got, want)
    bad = np.isnan(got).all(axis=0)
    assert list(np.nonzero(bad)[0]) == [3, 5] and np.isfinite(got[:, ~bad]).all()
    clean = [0, 1, 2, 4, 6, 7]
    holes = yrep.copy()
    holes[:, 1, 10:50] = np.nan
    rc, free = from_ll_call(ll[:, clean], holes[:, clean], observed(kind)[clean])
    assert rc == _lib.OK and np.isfinite(free).all()
    assert_same(free, LC.run(ll[:, clean], holes[:, clean], observed(kind)[clean]))
    assert free[0, 1] + free[1, 1] < 0.8 and free[:, 0].tobytes() == got[:, 0].tobytes()


def test_refusals(hip):
    cm = TP.comp(models.SIMPLE)
    x = PI.draws(models.SIMPLE, S=2, Cn=3)
    S, d, Cn = x.shape
    N = 10
    xd = torch.from_numpy(x).cuda()
    out = torch.zeros((4, N), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L, O = cm.L, _lib.PredictiveOpts
    f, X, OUT = L.exmc_hip_loo_pit, xd.data_ptr(), out.data_ptr()
    assert f(cm.h, O(1, 0, 0), X, S, d, Cn, 0, OUT) == _lib.OK
    bad = [(cm.h, O(1, 0, 0), None, S, d, Cn, 0, OUT),        # no trace
           (cm.h, O(1, 0, 0), X, S, d, Cn, 0, None),          # no output
           (cm.h, O(1, 0, 0), X, S, d + 1, Cn, 0, OUT),
           (cm.h, O(1, 0, 0), X, 0, d, Cn, 0, OUT),
           (cm.h, O(1, 0, 0), X, S, d, 0, 0, OUT),
           (cm.h, O(1, -1, 0), X, S, d, Cn, 0, OUT),
           (cm.h, O(1, 0, 1), X, S, d, Cn, 0, OUT),           # there is no resume
           (cm.h, O(1, 0, 0), X, 1, d, 1, 0, OUT),            # n < 2
           (cm.h, O(1, 0, 0), X, 65536, d, 32768, 0, OUT),    # n = 2^31 (refused before anything is read)
           (None, O(1, 0, 0), X, S, d, Cn, 0, OUT)]
    for args in bad:
        assert f(*args) == _lib.ERR_BADARG, args[1:]
    hin, hout = np.zeros((Cn, S, d)), np.zeros((4, N))
    H, HO = hin.ctypes.data_as(DP), hout.ctypes.data_as(DP)
    g = L.exmc_hip_loo_pit_host
    assert g(cm.h, O(1, 0, 0), H, S, d, Cn, 0, HO) == _lib.OK
    for args in [(cm.h, O(1, 0, 0), None, S, d, Cn, 0, HO), (cm.h, O(1, 0, 0), H, S, d, Cn, 0, None),
                 (cm.h, O(1, 0, 0), H, S, d - 1, Cn, 0, HO), (cm.h, O(1, 0, 0), H, 0, d, Cn, 0, HO),
                 (cm.h, O(1, 0, 0), H, S, d, -1, 0, HO), (cm.h, O(1, -3, 0), H, S, d, Cn, 0, HO),
                 (cm.h, O(1, 0, 1), H, S, d, Cn, 0, HO), (cm.h, O(1, 0, 0), H, 1, d, 1, 0, HO),
                 (None, O(1, 0, 0), H, S, d, Cn, 0, HO)]:
        assert g(*args) == _lib.ERR_BADARG, args[1:]
    # the model-free call
    ll = torch.zeros((S, N, Cn), dtype=torch.float64, device="cuda")
    y = torch.zeros(N, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    k, A, Y = L.exmc_hip_loo_pit_from_ll, ll.data_ptr(), y.data_ptr()
    assert k(0, A, A, Y, S, N, Cn, OUT) == _lib.OK
    for args in [(0, None, A, Y, S, N, Cn, OUT), (0, A, None, Y, S, N, Cn, OUT), (0, A, A, None, S, N, Cn, OUT),
                 (0, A, A, Y, S, N, Cn, None), (0, A, A, Y, 0, N, Cn, OUT), (0, A, A, Y, S, 0, Cn, OUT),
                 (0, A, A, Y, S, N, 0, OUT), (0, A, A, Y, 1, N, 1, OUT), (0, A, A, Y, 65536, N, 32768, OUT)]:
        assert k(*args) == _lib.ERR_BADARG, args
    with pytest.raises(ValueError):
        PP.loo_pit(cm, xd.float())
    with pytest.raises(ValueError):
        PP.loo_pit_from_pointwise(ll, ll[:, :5], y)
    with pytest.raises(ValueError):
        PP.loo_pit_from_pointwise(ll, ll, y[:5])


def test_unsupported_models(hip):
    from exmc_amd import codegen, sampler
    # EXMC_MODEL_STD_NORMAL has no data: the library makes no handle of it, and a null handle is a bad argument
    h = C.c_void_p()
    assert hip.exmc_hip_model_create(models.STD_NORMAL, 2, None, 0, 0, C.byref(h)) == _lib.ERR_UNSUPPORTED
    # a generated model, compiled WITH its per-datum terms: it has datums for model comparison, none here
    gen = sampler.compile(codegen.compile_ir(codegen.eight_schools_ir(), pointwise=True))
    try:
        assert gen.L.exmc_hip_model_n_data(gen.h) == 8
        for name in _lib.LOO_PIT_EXPORTS:
            getattr(gen.L, name)
        xd = torch.zeros((2, gen.d, 3), dtype=torch.float64, device="cuda")
        out = torch.zeros((4, 8), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert gen.L.exmc_hip_loo_pit(gen.h, _lib.PredictiveOpts(1, 0, 0), xd.data_ptr(), 2, gen.d, 3, 0,
                                      out.data_ptr()) == _lib.ERR_UNSUPPORTED
        assert b"loo-pit" in gen.L.exmc_hip_last_error()
        hin, hout = np.zeros((3, 2, gen.d)), np.zeros((4, 8))
        assert gen.L.exmc_hip_loo_pit_host(gen.h, _lib.PredictiveOpts(1, 0, 0), hin.ctypes.data_as(DP), 2, gen.d, 3, 0,
                                           hout.ctypes.data_as(DP)) == _lib.ERR_UNSUPPORTED
        with pytest.raises(_lib.ExmcHipError):
            PP.loo_pit(gen, xd)
        # the plug-in's model-free entry point answers as its PSIS one does; libexmc_hip.so serves the call,
        # with the generated model's own terms
        ll = MC.pointwise_log_likelihood(gen, xd)[0]
        yrep = torch.zeros_like(ll)
        y = np.zeros(8)
        assert from_ll_call(ll, yrep, y, L=gen.L)[0] == _lib.ERR_UNSUPPORTED
        assert ll.shape == (2, 8, 3)
        rc, free = from_ll_call(ll, yrep, y)
        assert rc == _lib.OK and np.isfinite(free[:3]).all()
    finally:
        gen.close()
