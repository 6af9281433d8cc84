"""ADVI on the GPU (include/exmc_hip_advi.h, advi_kernel) against the statement of advi.ex in lane
mode (tests/advi_statement.py): mu, log_sigma, the ELBO history (NaN where the statement has none),
num_iters, converged and the draws bit for bit, for every model kind's layout family and for
generated models; the branches of the convergence test, each asserted on the statement's own run."""
import ctypes as C
import math

import numpy as np
import pytest

import advi_statement as AS
import gen_checker as GC
import oracle as O
import pathfinder_statement as PS
import sv_ncp_checker as SN
from exmc_amd import _lib, advi, codegen as cg, models, sampler

pytestmark = pytest.mark.gpu

KEYS = ("mu", "log_sigma", "elbo_history", "num_iters", "converged", "draws")
# (kind, lanes): the test that fits in that layout -- each kind's default row; every other row of
# exmc_layouts.inc is run by test_gpu_fit_layouts.py (test_fit_layouts_catalogue.py holds the two to the table)
FIT_LAYOUTS = {("simple", 1): "test_simple_one_lane", ("eight_schools", 16): "test_eight_schools_16_lanes",
               ("sv", 64): "test_sv_64_lanes", ("sv_ncp", 64): "test_sv_ncp_64_lanes",
               ("logistic", 16): "test_logistic_16_lanes_small_design", ("radon", 64): "test_radon_64_lanes"}


def _statement(om, lanes, seed, n_fits, chain_lo=0, **kw):
    rs = [AS.fit_lane(om, lanes, seed + 7919 * (chain_lo + c), **kw) for c in range(n_fits)]
    out = {k: np.stack([np.asarray(r[k]) for r in rs]) for k in ("mu", "log_sigma", "draws")}
    hist = np.full((n_fits, kw["max_iters"]), np.nan)
    for c, r in enumerate(rs):
        assert len(r.elbo_history) == r.num_iters
        hist[c, :r.num_iters] = r.elbo_history
    out["elbo_history"] = hist
    out["num_iters"] = np.array([r.num_iters for r in rs], np.int32)
    out["converged"] = np.array([1 if r.converged else 0 for r in rs], np.int32)
    out["non_finite"] = [r.non_finite for r in rs]
    return out


def _assert_same(got, want, what=""):
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        # a NaN carries no payload contract: NaN where the statement has NaN, bytes elsewhere
        nan = np.isnan(b) if b.dtype == np.float64 else np.zeros(b.shape, bool)
        assert np.array_equal(np.isnan(a) if a.dtype == np.float64 else nan, nan), (what, k)
        assert a[~nan].tobytes() == b[~nan].tobytes(), (what, k, a, b)


def _check(comp, om, lanes, seed, n_fits, **kw):
    got = advi.fit_raw(comp, dict(kw, seed=seed, lanes_per_chain=lanes), n_fits)
    want = _statement(om, lanes, seed, n_fits, **kw)
    _assert_same(got, want, (lanes, seed, kw))
    return got, want


@pytest.fixture(scope="module")
def handles(hip):
    made = {}

    def get(name, spec_fn):
        if name not in made:
            spec = spec_fn()
            made[name] = (spec, sampler.compile(spec))
        return made[name]
    yield get
    for _, comp in made.values():
        comp.close()


def test_simple_one_lane(handles):
    spec, comp = handles("simple", models.simple)
    _check(comp, O.model_for(spec), 1, 3, 3, max_iters=12, num_draws=5, window_size=6)


@pytest.mark.parametrize("n_mc", [1, 3])
def test_eight_schools_16_lanes(handles, n_mc):
    """five fits: the second wavefront is partial; the sequential-sum group"""
    spec, comp = handles("es", models.eight_schools)
    _check(comp, O.model_for(spec), 16, 11, 5, max_iters=14, num_draws=4, num_mc_samples=n_mc, window_size=8)


def test_sv_64_lanes(handles):
    """DPL = 2 with invalid slots (d = 102), the butterfly, a flat order that is not the kernel order"""
    spec, comp = handles("sv", lambda: models.sv(models.sv_returns()))
    _check(comp, O.model_for(spec), 64, 5, 3, max_iters=10, num_draws=3, window_size=4, learning_rate=1.0e-3)


def test_sv_ncp_64_lanes(handles):
    r = models.sv_returns()
    spec, comp = handles("sv_ncp", lambda: models.sv_ncp(r))
    _, want = _check(comp, SN.model(r, True), 64, 0, 3, max_iters=10, num_draws=3, window_size=4,
                     learning_rate=1.0e-3, num_mc_samples=2)
    assert sum(want["non_finite"]) == 0


def test_logistic_16_lanes_small_design(handles):
    """16 lanes: DPL = 2 (d = 21), the butterfly sum, not wave-cooperative: lane groups without a fit
    return at once. The wave-cooperative model (kCoop) is Logistic<4>:
    test_gpu_fit_layouts.py::test_logistic_advi at 4 lanes."""
    X, y = models.logistic_data(seed=140, n=40, k=20)
    spec, comp = handles("logistic", lambda: models.logistic(X, y))
    _check(comp, O.model_for(spec), 16, 2, 2, max_iters=8, num_draws=2, window_size=4)


def test_radon_64_lanes(handles):
    from test_radon_chunks import _survey_like
    spec, comp = handles("radon", lambda: models.radon(_survey_like()))
    _check(comp, O.model_for(spec), 64, 4, 2, max_iters=6, num_draws=2, window_size=4)
    # at the default rate the density is not finite in the first iterations and mu goes to -inf, which
    # compares little; at 1e-3 everything stays finite
    got, want = _check(comp, O.model_for(spec), 64, 4, 2, max_iters=6, num_draws=2, window_size=4,
                       learning_rate=1.0e-3)
    assert sum(want["non_finite"]) == 0
    assert all(np.isfinite(want[k]).all() and np.isfinite(got[k]).all() for k in KEYS)


@pytest.fixture(scope="module")
def generated(hip):
    made = {}

    def get(name):
        if name not in made:
            if name == "simple":
                spec = cg.compile_ir(cg.simple_ir())
            elif name == "es":
                spec = cg.compile_ir(cg.eight_schools_ir())
            elif name == "sv_ncp":
                r = np.asarray(models.sv_returns())
                spec = cg.compile_ir(cg.sv_ir(r), ncp=True, name="gen_sv_ncp",
                                     default_init=models.sv_ncp(r).default_init, lanes=64, waves_per_simd=2)
            else:
                ir = cg.IR()
                ir.rv("x", "normal", dict(mu=float(name), sigma=1.0))
                spec = cg.compile_ir(ir)
            made[name] = (spec, sampler.compile(spec))
        return made[name]
    yield get
    for _, comp in made.values():
        comp.close()


@pytest.mark.parametrize("name,lanes", [("simple", 1), ("es", 16), ("sv_ncp", 64)])
def test_generated_models(generated, name, lanes):
    """a one-lane layout, the plate layout of eight_schools, the 64-lane scan chain of non-centred sv"""
    spec, comp = generated(name)
    _check(comp, GC.model(spec.gen, lanes), lanes, 9, 2, max_iters=6, num_draws=2, window_size=4,
           learning_rate=1.0e-3)


# ---- the branches of the convergence test --------------------------------------------------------------
# Settings chosen on the CPU by reading the statement's run on eight_schools, seeds 11 + 7919 c, rate 0.05,
# tolerance 0.02: with a window of 10 the fits would stop at 23, 13, 20, 25, 23; with 9 at 12, 10, 19, 13, 22.
@pytest.mark.parametrize("window,max_iters,stops", [(10, 22, [22, 13, 20, 22, 22]), (9, 15, [12, 10, 15, 13, 15])])
def test_mixed_convergence_in_one_wavefront(handles, window, max_iters, stops):
    """Fits 0..3 share a wavefront: some converge before max_iters and are predicated off (their
    generators stay put, so their draws depend on their own halt), others run to the end. An odd
    window drops its oldest value."""
    spec, comp = handles("es", models.eight_schools)
    got, want = _check(comp, O.model_for(spec), 16, 11, 5, max_iters=max_iters, num_draws=3, window_size=window,
                       learning_rate=0.05, convergence_tol=0.02)
    assert want["num_iters"].tolist() == stops
    assert want["converged"].tolist() == [1 if s < max_iters else 0 for s in stops]
    assert 0 < want["converged"][:4].sum() < 4
    assert np.isnan(got["elbo_history"][1, stops[1]:]).all() and not np.isnan(got["elbo_history"][1, :stops[1]]).any()


def test_early_exit_when_every_fit_converges_at_the_window(handles):
    """a tolerance so large that every fit converges as soon as the window is full: the wavefronts leave
    the loop there, and the draws continue each generator from iteration window_size"""
    spec, comp = handles("es", models.eight_schools)
    got, want = _check(comp, O.model_for(spec), 16, 11, 5, max_iters=60, num_draws=3, window_size=10,
                       convergence_tol=1.0e9)
    assert (want["num_iters"] == 10).all() and (want["converged"] == 1).all()
    assert (got["num_iters"] == 10).all()


def test_non_finite_logp_takes_the_constant_branch(handles):
    """At the default rate sv_ncp's density stops being finite after a few iterations (found by reading
    the statement's run; NaN arithmetic, nothing faults): the ELBO is -1.0e10 from there on, mu goes
    NaN through the unrepaired gradient, and the fit converges on equal means once the window holds
    only the constant."""
    r = models.sv_returns()
    spec, comp = handles("sv_ncp", lambda: models.sv_ncp(r))
    got, want = _check(comp, SN.model(r, True), 64, 0, 2, max_iters=40, num_draws=2, window_size=10)
    assert min(want["non_finite"]) >= 10 and (want["converged"] == 1).all() and (want["num_iters"] < 40).all()
    n0 = int(want["num_iters"][0])
    assert (want["elbo_history"][0, n0 - 10:n0] == -1.0e10).all()
    assert np.isnan(want["mu"]).any() and np.isnan(got["mu"]).any()


def test_flat_order_moves_the_variates(hip):
    """with the two entries of simple swapped in the flat vector, variate r goes to kernel dimension
    perm[r], in every sample and in every draw"""
    spec = models.simple()
    comp = sampler.compile(spec)
    try:
        perm = np.array([1, 0], dtype=np.int32)
        comp.check(comp.L.exmc_hip_model_set_flat_order(comp.h, perm.ctypes.data_as(C.POINTER(C.c_int32)), 2))
        om = O.model_for(spec)
        om.set_flat_order([1, 0])
        kw = dict(max_iters=5, num_draws=3, num_mc_samples=2, window_size=4)
        got, want = _check(comp, om, 1, 21, 2, **kw)
        plain = _statement(O.model_for(spec), 1, 21, 2, **kw)
        assert not np.array_equal(plain["draws"], want["draws"]) and not np.array_equal(plain["mu"], want["mu"])
        # independent of the statement's loop: the variates numbered num_iters * n_mc * d + r of the seeded
        # generator, swapped, are the z of draw 0 of fit 0
        n = int(got["num_iters"][0])
        f = PS.rng_factory(21, 1)()
        v = np.array([f() for _ in range(n * 2 * 2 + 2)])[n * 2 * 2:]
        zk = v[::-1]                                          # kernel dimension i takes variate rank[i]
        sigma = np.array([O.lib().exo_det_exp(float(x)) for x in got["log_sigma"][0]])
        assert np.array_equal(got["draws"][0, 0], got["mu"][0] + sigma * zk)
        assert not np.array_equal(got["draws"][0, 0], got["mu"][0] + sigma * zk[::-1])
    finally:
        comp.close()


def test_batch_is_the_seeds_and_chain_lo_shards(handles):
    spec, comp = handles("es", models.eight_schools)
    kw = dict(max_iters=15, num_draws=2, lanes_per_chain=16, window_size=9, learning_rate=0.05, convergence_tol=0.02)
    whole = advi.fit_raw(comp, dict(kw, seed=11), 6)
    assert 0 < whole["converged"].sum() < 6
    for c in (0, 3, 5):
        one = advi.fit_raw(comp, dict(kw, seed=11 + 7919 * c), 1)
        for k in KEYS:
            assert one[k][0].tobytes() == whole[k][c].tobytes(), (c, k)
    part = advi.fit_raw(comp, dict(kw, seed=11, chain_lo=2), 4)
    for k in KEYS:
        assert part[k].tobytes() == np.ascontiguousarray(whole[k][2:]).tobytes(), k


def test_device_form_null_outputs_and_refusals(handles):
    import torch
    spec, comp = handles("es", models.eight_schools)
    S, Cn, d, iters = 3, 5, spec.d, 15
    host = advi.fit_raw(comp, dict(max_iters=iters, num_draws=S, seed=11, lanes_per_chain=16, window_size=9,
                                   learning_rate=0.05, convergence_tol=0.02), Cn)
    dev = torch.device("cuda", 0)
    draws = torch.zeros((S, d, Cn), dtype=torch.float64, device=dev)
    mu = torch.zeros((d, Cn), dtype=torch.float64, device=dev)
    hist = torch.zeros((iters, Cn), dtype=torch.float64, device=dev)
    ni = torch.zeros(Cn, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ao = _lib.AdviOpts(S, iters, 1, 9, 0.05, 0.02, 11, 16)
    comp.check(comp.L.exmc_hip_advi(comp.h, ao, Cn, 0, draws.data_ptr(), mu.data_ptr(), None, hist.data_ptr(),
                                    ni.data_ptr(), None))
    assert np.array_equal(draws.cpu().numpy().transpose(2, 0, 1), host["draws"])
    assert np.array_equal(mu.cpu().numpy().T, host["mu"])
    assert np.array_equal(hist.cpu().numpy().T, host["elbo_history"], equal_nan=True)
    assert np.array_equal(ni.cpu().numpy(), host["num_iters"])
    # no history asked for: the window lives in scratch of the call, the results are the same
    comp.check(comp.L.exmc_hip_advi(comp.h, ao, Cn, 0, draws.data_ptr(), None, None, None, ni.data_ptr(), None))
    assert np.array_equal(draws.cpu().numpy().transpose(2, 0, 1), host["draws"])
    assert np.array_equal(ni.cpu().numpy(), host["num_iters"])
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    cv = np.zeros(Cn, np.int32)
    comp.check(comp.L.exmc_hip_advi_host(comp.h, ao, Cn, 0, dp(), dp(), dp(), dp(), ip(), cv.ctypes.data_as(ip)))
    assert np.array_equal(cv, host["converged"])

    def call(o, n=Cn, lo=0):
        return comp.L.exmc_hip_advi_host(comp.h, o, n, lo, dp(), dp(), dp(), dp(), ip(), cv.ctypes.data_as(ip))
    for bad in (_lib.AdviOpts(0, iters, 1, 9, 0.05, 0.02, 11, 16), _lib.AdviOpts(S, 0, 1, 9, 0.05, 0.02, 11, 16),
                _lib.AdviOpts(S, iters, 0, 9, 0.05, 0.02, 11, 16), _lib.AdviOpts(S, iters, 1, 1, 0.05, 0.02, 11, 16),
                _lib.AdviOpts(S, iters, 1, 0, 0.05, 0.02, 11, 16), _lib.AdviOpts(S, -1, 1, 9, 0.05, 0.02, 11, 16)):
        assert call(bad) == _lib.ERR_BADARG
        assert comp.L.exmc_hip_advi(comp.h, bad, Cn, 0, None, None, None, None, None, None) == _lib.ERR_BADARG
    assert call(ao, n=0) == _lib.ERR_BADARG and call(ao, lo=-1) == _lib.ERR_BADARG
    assert call(_lib.AdviOpts(S, iters, 1, 2, 0.05, 0.02, 11, 16)) == 0          # the smallest window
    assert call(_lib.AdviOpts(S, iters, 1, 9, 0.05, 0.02, 11, 5)) == _lib.ERR_UNSUPPORTED


def test_reference_tests_restated(generated):
    """advi_test.exs with its literals: Normal(5, 1), 200 draws, 500 iterations, rate 0.05, seed 42: the
    mean within 2.0 of 5.0; Normal(0, 1), 50 draws, 100 iterations, seed 42: a history of numbers;
    seed 123 twice: equal draws. Each equal to the statement."""
    spec, comp = generated("5.0")
    opts = dict(num_draws=200, max_iters=500, learning_rate=0.05, seed=42)
    draws, info = advi.fit(comp, opts)
    assert set(draws) == {"x"} and draws["x"].shape[0] == 200
    assert abs(float(np.mean(draws["x"])) - 5.0) < 2.0
    assert isinstance(info["elbo_history"], list) and len(info["elbo_history"]) == info["num_iters"] > 0
    want = AS.fit_lane(GC.model(spec.gen, 1), 1, 42, num_draws=200, max_iters=500, learning_rate=0.05)
    assert np.array_equal(draws["x"].reshape(-1), want.draws.reshape(-1))
    assert info["elbo_history"] == want.elbo_history and info["converged"] == want.converged
    assert info["num_iters"] == want.num_iters
    spec0, comp0 = generated("0.0")
    _, i0 = advi.fit(comp0, dict(num_draws=50, max_iters=100, seed=42))
    assert len(i0["elbo_history"]) == i0["num_iters"] and all(math.isfinite(e) for e in i0["elbo_history"])
    a, _ = advi.fit(comp0, dict(num_draws=50, max_iters=100, seed=123))
    b, _ = advi.fit(comp0, dict(num_draws=50, max_iters=100, seed=123))
    assert a["x"].tobytes() == b["x"].tobytes()
    many, infos, best = advi.fit(comp0, dict(num_draws=5, max_iters=100, seed=123), num_fits=3)
    assert len(many) == 3 and many[0]["x"].tobytes() != many[1]["x"].tobytes()
    assert best == int(np.argmax([np.mean(i["elbo_history"][-50:]) for i in infos]))
