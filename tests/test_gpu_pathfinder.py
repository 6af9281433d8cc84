"""Pathfinder on the GPU (include/exmc_hip_pathfinder.h, pathfinder_kernel) against the statement of
pathfinder.ex in lane mode (tests/pathfinder_statement.py): mu, sigma, elbo, num_iters, best_index,
status and the draws bit for bit, for every model kind's layout family and for generated models."""
import ctypes as C
import math

import numpy as np
import pytest

import gen_checker as GC
import oracle as O
import pathfinder_statement as PS
import sv_ncp_checker as SN
from exmc_amd import codegen as cg, models, pathfinder, sampler

pytestmark = pytest.mark.gpu

KEYS = ("mu", "sigma", "elbo", "num_iters", "best_index", "status", "draws")
# (kind, lanes): the test that fits in that layout -- each kind's default row; every other row of
# exmc_layouts.inc is run by test_gpu_fit_layouts.py (test_fit_layouts_catalogue.py holds the two to the table)
FIT_LAYOUTS = {("simple", 1): "test_simple_one_lane", ("eight_schools", 16): "test_eight_schools_16_lanes",
               ("sv", 64): "test_sv_64_lanes", ("sv_ncp", 64): "test_sv_ncp_64_lanes_and_the_halt",
               ("logistic", 16): "test_logistic_16_lanes_small_design", ("radon", 64): "test_radon_64_lanes"}


def _statement(om, lanes, seed, n_paths, chain_lo=0, **kw):
    rs = [PS.fit_lane(om, lanes, seed + 7919 * (chain_lo + c), **kw) for c in range(n_paths)]
    out = {k: np.stack([np.asarray(r[k]) for r in rs]) for k in KEYS}
    out["num_iters"] = out["num_iters"].astype(np.int32)
    out["best_index"] = out["best_index"].astype(np.int32)
    out["status"] = out["status"].astype(np.int32)
    out["pushes"] = [r.pushes for r in rs]
    return out


def _assert_same(got, want, what=""):
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        # NaN results (status 1) carry no payload contract: NaN where the statement has NaN, bytes elsewhere
        nan = np.isnan(b) if b.dtype == np.float64 else np.zeros(b.shape, bool)
        assert np.array_equal(np.isnan(a) if a.dtype == np.float64 else nan, nan), (what, k)
        assert a[~nan].tobytes() == b[~nan].tobytes(), (what, k, a, b)


def _check(comp, om, lanes, seed, n_paths, **kw):
    opts = dict(kw, seed=seed, lanes_per_chain=lanes)
    got = pathfinder.fit_raw(comp, opts, n_paths)
    want = _statement(om, lanes, seed, n_paths, **kw)
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
    _check(comp, O.model_for(spec), 1, 3, 3, max_iters=8, num_draws=5)


@pytest.mark.parametrize("history_size", [6, 2])
def test_eight_schools_16_lanes(handles, history_size):
    """five paths: the second wavefront is partial; the sequential-sum group"""
    spec, comp = handles("es", models.eight_schools)
    _check(comp, O.model_for(spec), 16, 11, 5, max_iters=12, num_draws=4, history_size=history_size)


@pytest.mark.parametrize("history_size", [6, 2, 1])
def test_eight_schools_history_fills_and_wraps(handles, history_size):
    """With sharp likelihoods the path crosses non-concave ground and pairs are pushed (none is with the
    benchmark data: y.s < 0 wherever the density is concave): the two-loop recursion, the push in
    front and the truncation at history_size."""
    def sharp():
        return models.eight_schools([3.0 * v for v in O.EIGHT_SCHOOLS_Y], [0.1 * v for v in O.EIGHT_SCHOOLS_SIGMA])
    spec, comp = handles("es_sharp", sharp)
    _, want = _check(comp, O.model_for(spec), 16, 11, 5, max_iters=12, num_draws=2, history_size=history_size)
    assert max(want["pushes"]) > 2 and min(want["pushes"]) >= 2


def test_sv_64_lanes(handles):
    """DPL = 2 with invalid slots (d = 102), the butterfly, a flat order that is not the kernel order"""
    spec, comp = handles("sv", lambda: models.sv(models.sv_returns()))
    _, want = _check(comp, O.model_for(spec), 64, 5, 3, max_iters=10, num_draws=3)
    assert sum(want["pushes"]) > 0


def test_sv_ncp_64_lanes_and_the_halt(handles):
    """From the seeded start the fixed step 0.01 g soon leaves the region where sv_ncp's density is
    finite: the path halts there (found by reading the statement's run, nothing is provoked), the
    failing point is no path point, and the lanes of a halted path keep taking part in the sums."""
    r = models.sv_returns()
    spec, comp = handles("sv_ncp", lambda: models.sv_ncp(r))
    got, want = _check(comp, SN.model(r, True), 64, 0, 3, max_iters=10, num_draws=3)
    assert (want["num_iters"] < 11).all() and (got["num_iters"] >= 1).all()


def test_logistic_16_lanes_small_design(handles):
    """16 lanes: DPL = 2 (d = 21), the butterfly sum, not wave-cooperative: lane groups without a path
    return at once. The wave-cooperative model (kCoop) is Logistic<4>:
    test_gpu_fit_layouts.py::test_logistic_pathfinder at 4 lanes."""
    X, y = models.logistic_data(seed=140, n=40, k=20)
    spec, comp = handles("logistic", lambda: models.logistic(X, y))
    _check(comp, O.model_for(spec), 16, 2, 2, max_iters=8, num_draws=2)


def test_radon_64_lanes(handles):
    from test_radon_chunks import _survey_like
    spec, comp = handles("radon", lambda: models.radon(_survey_like()))
    _check(comp, O.model_for(spec), 64, 4, 2, max_iters=6, num_draws=2)


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
    _check(comp, GC.model(spec.gen, lanes), lanes, 9, 2, max_iters=6, num_draws=2)


def test_flat_order_moves_the_start_and_the_draws(hip):
    """with the two entries of simple swapped in the flat vector, variate r goes to kernel dimension
    perm[r], in the start and in every draw"""
    spec = models.simple()
    comp = sampler.compile(spec)
    try:
        perm = np.array([1, 0], dtype=np.int32)
        comp.check(comp.L.exmc_hip_model_set_flat_order(comp.h, perm.ctypes.data_as(C.POINTER(C.c_int32)), 2))
        om = O.model_for(spec)
        om.set_flat_order([1, 0])
        got, want = _check(comp, om, 1, 21, 2, max_iters=1, num_draws=3)
        plain = _statement(O.model_for(spec), 1, 21, 2, max_iters=1, num_draws=3)
        assert not np.array_equal(plain["draws"], want["draws"])
        # independent of the statement: the first d variates of the seeded generator, swapped, are the z of
        # draw 0 of path 0, whatever point is best
        f = PS.rng_factory(21, 1)()
        zk = np.array([f() for _ in range(2)])[::-1]         # kernel dimension i takes variate rank[i]
        assert np.array_equal(got["draws"][0, 0], got["mu"][0] + got["sigma"][0] * zk)
        assert not np.array_equal(got["draws"][0, 0], got["mu"][0] + got["sigma"][0] * zk[::-1])
    finally:
        comp.close()


def test_batch_is_the_seeds_and_chain_lo_shards(handles):
    spec, comp = handles("es", models.eight_schools)
    kw = dict(max_iters=5, num_draws=2, lanes_per_chain=16)
    whole = pathfinder.fit_raw(comp, dict(kw, seed=77), 6)
    for c in (0, 3, 5):
        one = pathfinder.fit_raw(comp, dict(kw, seed=77 + 7919 * c), 1)
        for k in KEYS:
            assert one[k][0].tobytes() == whole[k][c].tobytes(), (c, k)
    part = pathfinder.fit_raw(comp, dict(kw, seed=77, chain_lo=2), 4)
    for k in KEYS:
        assert part[k].tobytes() == np.ascontiguousarray(whole[k][2:]).tobytes(), k


def test_device_form_and_null_outputs(handles):
    import torch
    from exmc_amd import _lib
    spec, comp = handles("es", models.eight_schools)
    S, Cn, d = 3, 5, spec.d
    host = pathfinder.fit_raw(comp, dict(max_iters=4, num_draws=S, seed=8, lanes_per_chain=16), Cn)
    dev = torch.device("cuda", 0)
    draws = torch.zeros((S, d, Cn), dtype=torch.float64, device=dev)
    mu = torch.zeros((d, Cn), dtype=torch.float64, device=dev)
    ni = torch.zeros(Cn, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    po = _lib.PfOpts(S, 4, 6, 8, 16)
    comp.check(comp.L.exmc_hip_pathfinder(comp.h, po, Cn, 0, draws.data_ptr(), mu.data_ptr(), None, None,
                                          ni.data_ptr(), None, None))
    assert np.array_equal(draws.cpu().numpy().transpose(2, 0, 1), host["draws"])
    assert np.array_equal(mu.cpu().numpy().T, host["mu"])
    assert np.array_equal(ni.cpu().numpy(), host["num_iters"])
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    elbo = np.zeros(Cn)
    comp.check(comp.L.exmc_hip_pathfinder_host(comp.h, po, Cn, 0, dp(), dp(), dp(), elbo.ctypes.data_as(dp),
                                               ip(), ip(), ip()))
    assert np.array_equal(elbo, host["elbo"])
    for bad in (_lib.PfOpts(0, 4, 6, 8, 16), _lib.PfOpts(3, 0, 6, 8, 16), _lib.PfOpts(3, 4, 0, 8, 16),
                _lib.PfOpts(3, 4, 7, 8, 16)):
        assert comp.L.exmc_hip_pathfinder_host(comp.h, bad, Cn, 0, dp(), dp(), dp(), elbo.ctypes.data_as(dp),
                                               ip(), ip(), ip()) == _lib.ERR_BADARG
    assert comp.L.exmc_hip_pathfinder_host(comp.h, _lib.PfOpts(3, 4, 6, 8, 5), Cn, 0, dp(), dp(), dp(),
                                           elbo.ctypes.data_as(dp), ip(), ip(), ip()) == _lib.ERR_UNSUPPORTED


def test_reference_tests_restated(generated):
    """pathfinder_test.exs with its literals: Normal(3, 1), 500 draws, 50 iterations, seed 42: the mean
    within 2.5 of 3.0, num_iters > 0, a finite ELBO; Normal(0, 1), seed 123 twice: equal draws."""
    spec, comp = generated("3.0")
    draws, info = pathfinder.fit(comp, dict(num_draws=500, max_iters=50, seed=42))
    assert set(draws) == {"x"} and draws["x"].shape[0] == 500
    assert abs(float(np.mean(draws["x"])) - 3.0) < 2.5
    assert info["num_iters"] > 0 and math.isfinite(info["elbo"]) and info["status"] == 0
    want = PS.fit_lane(GC.model(spec.gen, 1), 1, 42, num_draws=500, max_iters=50)
    assert np.array_equal(draws["x"].reshape(-1), want.draws.reshape(-1)) and info["elbo"] == want.elbo
    spec0, comp0 = generated("0.0")
    a, ia = pathfinder.fit(comp0, dict(num_draws=50, max_iters=20, seed=123))
    b, _ = pathfinder.fit(comp0, dict(num_draws=50, max_iters=20, seed=123))
    assert a["x"].tobytes() == b["x"].tobytes() and math.isfinite(ia["elbo"])
    many, infos, best = pathfinder.fit(comp0, dict(num_draws=5, max_iters=20, seed=123), num_paths=3)
    assert len(many) == 3 and best == int(np.argmax([i["elbo"] for i in infos]))
    assert many[0]["x"].tobytes() == a["x"][:5].tobytes()
