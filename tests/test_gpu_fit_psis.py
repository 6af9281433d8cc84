"""The smoothing and the resampling of log importance ratios on the GPU (exmc_amd/csrc/exmc_psis_ratio.hpp,
include/exmc_hip_fit_psis.h): exmc_hip_ratio_psis_from_lr and exmc_hip_ratio_gather byte for byte against the
host checker (tests/host/fit_psis_host_checker.c) per fit and pooled; weight-zero samples and NaN groups;
exmc_hip_fit_psis_host and importance.psis_fit end to end on real Pathfinder and ADVI fits of eight_schools
against the statement run on the same raw arrays; every refusal; the plug-in library's answers."""
import ctypes as C

import numpy as np
import pytest
import torch

import fit_psis_checker as FC
import fit_psis_statement as FS
import oracle as O
from exmc_amd import _lib, advi, codegen as cg, importance, models, pathfinder, sampler
from test_fit_psis_statement import ratios

pytestmark = pytest.mark.gpu

D = 3       # dimensions of the draws the gather moves


def device(lr, pooled, R, seed, want_lw=True, draws=None):
    """exmc_hip_ratio_psis_from_lr (and the gather of `draws` [S][D][F]) -> out, lw, idx, gathered"""
    L = _lib.load()
    S, F = lr.shape
    G = 1 if pooled else F
    x = torch.from_numpy(np.ascontiguousarray(lr)).cuda()
    out = torch.full((5, G), 7.0, dtype=torch.float64, device="cuda")
    lw = torch.full((S, F), 7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((max(R, 1), G), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.exmc_hip_ratio_psis_from_lr(0, x.data_ptr(), S, F, int(pooled), R, seed, out.data_ptr(),
                                             lw.data_ptr() if want_lw else None, idx.data_ptr() if R else None), L)
    got = None
    if draws is not None and R:
        dd = torch.from_numpy(np.ascontiguousarray(draws)).cuda()
        res = torch.full((R, draws.shape[1], G), 7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.exmc_hip_ratio_gather(0, dd.data_ptr(), idx.data_ptr(), S, draws.shape[1], F, int(pooled), R,
                                           res.data_ptr()), L)
        got = res.cpu().numpy()
    torch.cuda.synchronize()
    return out.cpu().numpy(), lw.cpu().numpy(), idx.cpu().numpy()[:R], got


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got != want)[:6], got.reshape(-1)[:6], want.reshape(-1)[:6])


def check(lr, pooled, R, seed, draws=None):
    out, lw, idx, res = device(lr, pooled, R, seed, draws=draws)
    wout, wlw, widx = FC.groups(lr, pooled, R, seed)
    same(out, wout, "out")
    same(lw, wlw, "lw")
    same(idx, widx, "idx")
    if res is not None:
        same(res, FC.gather(draws, widx, pooled), "gathered")
    return out, lw, idx


# (S, n_fits, pooled): per fit at a tail of 8 and of 95 samples (1000 draws: sixteen chunks to merge), pooled at
# 2100 samples (one block of the cumulative sum) and at 9100 (more than two blocks, chunks of 64), and 8 samples
# in either view: T <= 4, khat = +inf, nothing smoothed
SHAPES = [(40, 3, False), (1000, 70, False), (30, 70, True), (130, 70, True), (8, 1, False), (8, 1, True)]


@pytest.mark.parametrize("S,F,pooled", SHAPES)
def test_from_lr_bit_exact(hip, S, F, pooled):
    lr = ratios(S, F, 100 + S + F)
    n = S * F if pooled else S
    draws = np.random.default_rng(S).normal(size=(S, D, F))
    for R in (0, 1, 64, 1000, n + 37):
        out, lw, idx = check(lr, pooled, R, seed=2 ** 33 + R, draws=draws)
        assert idx.shape[0] == R and (R == 0 or (idx.min() >= 0 and idx.max() < n))
    if S == 8:
        assert np.all(np.isposinf(out[0])) and np.all(out[4] <= 4)
    else:
        assert np.all(np.isfinite(out)) and np.all(out[4] == FS.PS.tail_len(n))
    # without the caller's lw the weights live in scratch of the call: the same indices
    o2, lw2, idx2, _ = device(lr, pooled, 64, 2 ** 33 + 64, want_lw=False)
    same(idx2, FC.groups(lr, pooled, 64, 2 ** 33 + 64)[2], "idx without lw")
    assert np.all(lw2 == 7.0)
    o3, lw3, _, _ = device(lr, pooled, 0, 0, want_lw=False)      # the diagnostics alone
    same(o3, out, "out alone")


@pytest.mark.parametrize("pooled", [False, True])
def test_weight_zero_samples_and_nan_groups(hip, pooled):
    """the groups of tests/test_fit_psis_statement.py: 30 % weight-zero samples; all weights zero, a NaN, a
    +inf"""
    S, F = 500, 4
    lr = ratios(S, F, 23)
    zero = np.random.default_rng(5).random((S, F)) < 0.3
    a = np.where(zero, -np.inf, lr)
    draws = np.random.default_rng(1).normal(size=(S, D, F))
    out, lw, idx = check(a, pooled, 2000, 9, draws=draws)
    ob, _, ib = check(np.where(zero, -1e300, lr), pooled, 2000, 9)
    same(out[[0, 1, 2, 4]], ob[[0, 1, 2, 4]], "khat, log_mean_ratio, ess, T")
    same(idx, ib, "idx")
    picked = zero.reshape(-1)[idx[:, 0]] if pooled else np.stack([zero[idx[:, g], g] for g in range(F)])
    assert not picked.any() and np.all(out[3] == (zero.sum() if pooled else zero.sum(axis=0)))
    bad = ratios(60, 5, 31)
    bad[:, 1] = -np.inf
    bad[7, 2] = np.nan
    bad[9, 4] = np.inf
    d2 = np.random.default_rng(2).normal(size=(60, D, 5))
    out, lw, idx = check(bad, pooled, 33, 1, draws=d2)
    groups = [0] if pooled else [1, 2, 4]
    assert np.all(np.isnan(out[:, groups])) and np.all(idx[:, groups] == -1)
    if not pooled:
        assert np.all(np.isfinite(out[:, [0, 3]])) and np.all(np.isnan(lw[:, groups]))


# ---- end to end on real fits ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def es(hip):
    spec = models.eight_schools()
    comp = sampler.compile(spec)
    yield comp, O.model_for(spec)
    comp.close()


def _raws(comp):
    return (pathfinder.fit_raw(comp, dict(num_draws=64, max_iters=5, seed=3), 16),
            advi.fit_raw(comp, dict(num_draws=64, max_iters=50, seed=3), 16))


@pytest.mark.parametrize("which", ["pathfinder", "advi"])
@pytest.mark.parametrize("pooled", [False, True])
def test_end_to_end_on_real_fits(es, which, pooled):
    comp, om = es
    raw = _raws(comp)[0 if which == "pathfinder" else 1]
    scale, kind = (raw["sigma"], FS.SIGMA) if which == "pathfinder" else (raw["log_sigma"], FS.LOG_SIGMA)
    Cn, S, d = raw["draws"].shape
    assert (Cn, S) == (16, 64) and np.all(np.isfinite(raw["mu"])) and np.all(np.isfinite(scale))
    R, seed = 200, 77
    # the statement on the same raw arrays: the log ratios in lane mode, then the checker's orders and the
    # estimator from the papers
    cols = [FS.log_ratio_lane(om, 16, raw["draws"][c], raw["mu"][c], scale[c], kind) for c in range(Cn)]
    wlr = np.stack([c[0] for c in cols], axis=1)                  # [S][C]
    wlp = np.stack([c[1] for c in cols], axis=1)
    wout, wlw, widx = FC.groups(wlr, pooled, R, seed)
    sout, slw, sidx = FS.groups(wlr, pooled, R, seed)
    G = 1 if pooled else Cn
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    out, lw, lr, lp = np.zeros((5, G)), np.zeros((Cn, S)), np.zeros((Cn, S)), np.zeros((Cn, S))
    idx, res = np.zeros((G, R), np.int32), np.zeros((G, R, d))
    x, mu, sc = (np.ascontiguousarray(a) for a in (raw["draws"], raw["mu"], scale))
    comp.check(comp.L.exmc_hip_fit_psis_host(comp.h, x.ctypes.data_as(dp), mu.ctypes.data_as(dp), sc.ctypes.data_as(dp),
                                             kind, S, d, Cn, 0, int(pooled), R, seed, out.ctypes.data_as(dp),
                                             lw.ctypes.data_as(dp), idx.ctypes.data_as(ip), res.ctypes.data_as(dp),
                                             lr.ctypes.data_as(dp), lp.ctypes.data_as(dp)))
    assert comp.last_kernel_ms > 0
    same(lr, np.ascontiguousarray(wlr.T), "lr")
    same(lp, np.ascontiguousarray(wlp.T), "logp")
    same(out, wout, "out")
    same(lw, np.ascontiguousarray(wlw.T), "lw")
    same(idx, np.ascontiguousarray(widx.T), "idx")
    want_res = FC.gather(np.ascontiguousarray(x.transpose(1, 2, 0)), widx, pooled)       # [R][d][G]
    same(res, np.ascontiguousarray(want_res.transpose(2, 0, 1)), "resampled")
    np.testing.assert_allclose(out[:3], sout[:3], rtol=1e-9)
    np.testing.assert_array_equal(out[3:], sout[3:])
    np.testing.assert_array_equal(idx.T, sidx)
    # the Python layer over the same call
    r = importance.psis_fit(comp, raw, pooled=pooled, num_resample=R, seed=seed)
    assert set(r) >= {"khat", "log_mean_ratio", "ess", "n_zero", "tail", "log_weights", "indices", "draws", "trace"}
    same(r["log_weights"], lw, "log_weights")
    if pooled:
        assert [r[k] for k in _lib.FIT_PSIS_ROWS] == list(out[:, 0]) and r["dropped"].size == 0
        same(r["indices"], idx[0], "indices")
        same(r["draws"], res[0], "draws")
        tr = r["trace"]
    else:
        same(np.stack([r[k] for k in _lib.FIT_PSIS_ROWS]), out, "rows")
        same(r["indices"], idx, "indices")
        same(r["draws"], res, "draws")
        tr = r["trace"][5]
    ref = sampler._build_trace(comp.spec, res[0] if pooled else res[5])
    assert set(tr) == set(ref) and all(np.array_equal(tr[k], ref[k]) for k in ref)


def test_fit_psis_of_the_fit_modules_and_pooled_dropping(es):
    comp, _ = es
    raw, r = pathfinder.fit_psis(comp, dict(num_draws=64, max_iters=5, seed=3), num_paths=16, num_resample=10)
    want = importance.psis_fit(comp, raw, num_resample=10)
    assert all(np.array_equal(r[k], want[k], equal_nan=True) for k in ("khat", "ess", "indices", "log_weights"))
    raw2, r2 = advi.fit_psis(comp, dict(num_draws=64, max_iters=50, seed=3), num_fits=16, pooled=True)
    assert np.isfinite(r2["khat"]) and r2["trace"] is None and r2["indices"].shape == (0,)
    # a failed path (status 1, NaN mu) and a fit with an infinite scale are left out of the pool, and named
    bad = {k: np.array(v, copy=True) for k, v in raw.items() if k != "kernel_ms"}
    bad["status"][2] = 1
    bad["mu"][2] = np.nan
    bad["sigma"][9, 0] = np.inf
    rp = importance.psis_fit(comp, bad, pooled=True, num_resample=50, seed=4)
    assert list(rp["dropped"]) == [2, 9] and list(rp["kept"]) == [c for c in range(16) if c not in (2, 9)]
    keep = {k: (v[rp["kept"]] if isinstance(v, np.ndarray) else v) for k, v in raw.items()}
    rk = importance.psis_fit(comp, keep, pooled=True, num_resample=50, seed=4)
    assert rk["khat"] == rp["khat"] and np.array_equal(rk["indices"], rp["indices"]) and rp["log_weights"].shape == (14, 64)
    # per fit the failed path is a NaN group and its neighbours are what they were
    rf = importance.psis_fit(comp, bad, num_resample=5)
    assert np.isnan(rf["khat"][2]) and np.all(rf["indices"][2] == -1) and rf["trace"][2] is None
    assert np.all(np.isnan(rf["draws"][2])) and rf["khat"][3] == r["khat"][3]
    with pytest.raises(ValueError):
        importance.psis_fit(comp, dict(draws=raw["draws"], mu=raw["mu"]))
    with pytest.raises(ValueError):
        importance.psis_fit(comp, raw, num_resample=-1)


def test_generated_model_goes_through_its_plugin_and_the_main_library(hip):
    spec = cg.compile_ir(cg.eight_schools_ir())
    comp = sampler.compile(spec)
    try:
        raw = pathfinder.fit_raw(comp, dict(num_draws=40, max_iters=5, seed=3), 5)
        r = importance.psis_fit(comp, raw, num_resample=9, seed=2)
        x = np.ascontiguousarray(raw["draws"].transpose(1, 2, 0))
        lr = torch.zeros((40, 5), dtype=torch.float64, device="cuda")
        xd, m, s = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, raw["mu"].T, raw["sigma"].T))
        torch.cuda.synchronize()
        comp.check(comp.L.exmc_hip_fit_log_ratio(comp.h, xd.data_ptr(), m.data_ptr(), s.data_ptr(), 0, 40, 10, 5, 0,
                                                 lr.data_ptr(), None))
        wout, wlw, widx = FC.groups(lr.cpu().numpy(), False, 9, 2)
        same(np.stack([r[k] for k in _lib.FIT_PSIS_ROWS]), wout, "rows")
        same(r["log_weights"], np.ascontiguousarray(wlw.T), "lw")
        same(r["indices"], np.ascontiguousarray(widx.T), "idx")
        same(r["draws"], np.ascontiguousarray(FC.gather(x, widx, False).transpose(2, 0, 1)), "draws")
        # the plug-in carries the log ratio alone
        P = comp.L
        out = torch.zeros((5, 5), dtype=torch.float64, device="cuda")
        idx = torch.zeros((9, 5), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert P.exmc_hip_ratio_psis_from_lr(0, lr.data_ptr(), 40, 5, 0, 0, 0, out.data_ptr(), None, None) == _lib.ERR_UNSUPPORTED
        assert P.exmc_hip_ratio_gather(0, xd.data_ptr(), idx.data_ptr(), 40, 10, 5, 0, 9, xd.data_ptr()) == _lib.ERR_UNSUPPORTED
        assert P.exmc_hip_fit_psis(comp.h, xd.data_ptr(), m.data_ptr(), s.data_ptr(), 0, 40, 10, 5, 0, 0, 0, 0,
                                   out.data_ptr(), None, None, None, None, None) == _lib.ERR_UNSUPPORTED
        dp = C.POINTER(C.c_double)
        h = np.zeros((5, 5))
        assert P.exmc_hip_fit_psis_host(comp.h, raw["draws"].ctypes.data_as(dp), raw["mu"].ctypes.data_as(dp),
                                        raw["sigma"].ctypes.data_as(dp), 0, 40, 10, 5, 0, 0, 0, 0, h.ctypes.data_as(dp),
                                        None, None, None, None, None) == _lib.ERR_UNSUPPORTED
    finally:
        comp.close()


def test_refusals(es):
    comp, om = es
    L = comp.L
    S, F, d, R = 6, 3, om.d, 4
    lr = torch.zeros((S, F), dtype=torch.float64, device="cuda")
    out = torch.zeros((5, F), dtype=torch.float64, device="cuda")
    idx = torch.zeros((R, F), dtype=torch.int32, device="cuda")
    x = torch.zeros((S, d, F), dtype=torch.float64, device="cuda")
    m = torch.ones((d, F), dtype=torch.float64, device="cuda")
    res = torch.zeros((R, d, F), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()      # noqa: E731

    def refused(f, args, cases):
        assert f(*args) == _lib.OK
        for at, bad in cases:
            a = list(args)
            a[at] = bad
            assert f(*a) == _lib.ERR_BADARG, (f.__name__, at)

    refused(L.exmc_hip_ratio_psis_from_lr, [0, p(lr), S, F, 0, R, 1, p(out), None, p(idx)],
            [(1, None), (2, 0), (3, 0), (5, -1), (7, None), (9, None), (0, 99)])
    # a pooled n above 2^31 - 1 (refused before anything is read)
    assert L.exmc_hip_ratio_psis_from_lr(0, p(lr), 1 << 16, 1 << 15, 1, 0, 1, p(out), None, None) == _lib.ERR_BADARG
    refused(L.exmc_hip_ratio_gather, [0, p(x), p(idx), S, d, F, 0, R, p(res)],
            [(1, None), (2, None), (3, 0), (4, 0), (5, 0), (7, 0), (8, None), (0, 99)])
    assert L.exmc_hip_ratio_gather(0, p(x), p(idx), 1 << 16, d, 1 << 15, 1, R, p(res)) == _lib.ERR_BADARG
    args = [comp.h, p(x), p(m), p(m), 0, S, d, F, 0, 0, R, 1, p(out), None, None, None, None, None]
    cases = [(0, None), (1, None), (2, None), (3, None), (4, 7), (5, 0), (6, d - 1), (7, 0), (10, -1), (12, None)]
    refused(L.exmc_hip_fit_psis, args, cases)
    a = list(args)
    a[8] = 5        # no row of eight_schools has five lanes
    assert L.exmc_hip_fit_psis(*a) == _lib.ERR_UNSUPPORTED
    a = list(args)
    a[5], a[7], a[9] = 1 << 16, 1 << 15, 1
    assert L.exmc_hip_fit_psis(*a) == _lib.ERR_BADARG
    dp = C.POINTER(C.c_double)
    hx, hm, ho = np.zeros((F, S, d)), np.ones((F, d)), np.zeros((5, F))
    hargs = [comp.h, hx.ctypes.data_as(dp), hm.ctypes.data_as(dp), hm.ctypes.data_as(dp), 0, S, d, F, 0, 0, 0, 1,
             ho.ctypes.data_as(dp), None, None, None, None, None]
    refused(L.exmc_hip_fit_psis_host, hargs, cases)
