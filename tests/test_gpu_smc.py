"""SMC on the GPU (include/exmc_hip_smc.h, exmc_smc.hpp) against the statement of smc.ex in lane mode
(tests/smc_statement.py): particles, logps, the three histories (NaN where the statement has none),
num_stages and status bit for bit, for every model kind's default layout, eight_schools' other rows and
generated models; forced and suppressed resampling, batches, the non-finite branch, the flat order and
the refusals."""
import ctypes as C

import numpy as np
import pytest

import gen_checker as GC
import oracle as O
import smc_statement as SS
import sv_ncp_checker as SN
from exmc_amd import _lib, codegen as cg, models, sampler, smc

pytestmark = pytest.mark.gpu

KEYS = ("particles", "logp", "betas", "ess_history", "acceptance_rates", "num_stages", "status")


def _statement(om, lanes, seed, n_runs, n, run_lo=0, max_stages=SS.DEFAULT_MAX_STAGES, **kw):
    rs = [SS.sample_lane(om, lanes, seed, num_particles=n, run=run_lo + r, max_stages=max_stages, **kw)
          for r in range(n_runs)]
    out = SS.padded(rs, max_stages)
    out["runs"] = rs
    return out


def _assert_same(got, want, what=""):
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        # a NaN carries no payload contract: NaN where the statement has NaN, bytes elsewhere
        nan = np.isnan(b) if b.dtype == np.float64 else np.zeros(b.shape, bool)
        assert np.array_equal(np.isnan(a) if a.dtype == np.float64 else nan, nan), (what, k)
        assert a[~nan].tobytes() == b[~nan].tobytes(), (what, k, a, b)


def _check(comp, om, lanes, seed, n_runs, n, **kw):
    got = smc.sample_raw(comp, dict(kw, seed=seed, num_particles=n, lanes_per_chain=lanes), n_runs)
    kw.pop("run_lo", None)
    want = _statement(om, lanes, seed, n_runs, n, **kw)
    _assert_same(got, want, (lanes, seed, n, kw))
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


# ---- each kind's default row: N = 3 (a wavefront with empty lane groups, two runs) and N = 70 (more than
# one wavefront at every G), 2 MH steps; max_stages = 4 for the wide kinds ---------------------------------
def _both(comp, om, lanes, seed, **kw):
    _check(comp, om, lanes, seed, 2, 3, num_mh_steps=2, **kw)
    return _check(comp, om, lanes, seed, 1, 70, num_mh_steps=2, **kw)


def test_simple_one_lane(handles):
    spec, comp = handles("simple", models.simple)
    _, want = _both(comp, O.model_for(spec), 1, 3, max_stages=12)
    assert any(i is not None for i in want["runs"][0].indices)


def test_eight_schools_16_lanes(handles):
    spec, comp = handles("es", models.eight_schools)
    _both(comp, O.model_for(spec), 16, 11, max_stages=8)


def test_sv_64_lanes(handles):
    spec, comp = handles("sv", lambda: models.sv(models.sv_returns()))
    _both(comp, O.model_for(spec), 64, 5, max_stages=4)


def test_sv_ncp_64_lanes(handles):
    r = models.sv_returns()
    spec, comp = handles("sv_ncp", lambda: models.sv_ncp(r))
    _both(comp, SN.model(r, True), 64, 0, max_stages=4)


def test_logistic_16_lanes_small_design(handles):
    X, y = models.logistic_data(seed=140, n=40, k=20)
    spec, comp = handles("logistic", lambda: models.logistic(X, y))
    _both(comp, O.model_for(spec), 16, 2, max_stages=4)


def test_radon_64_lanes(handles):
    from test_radon_chunks import _survey_like
    spec, comp = handles("radon", lambda: models.radon(_survey_like()))
    _both(comp, O.model_for(spec), 64, 4, max_stages=4)


# ---- to the end at the defaults: N = 300 crosses the 256 stride of particle_sum ------------------------
def test_simple_to_the_end(handles):
    spec, comp = handles("simple", models.simple)
    got, want = _check(comp, O.model_for(spec), 1, 7, 1, 300)
    assert want["status"].tolist() == [0] and want["runs"][0].betas[-1] == 1.0
    assert got["betas"][0, want["num_stages"][0] - 1] == 1.0


def test_eight_schools_to_the_end(handles):
    spec, comp = handles("es", models.eight_schools)
    got, want = _check(comp, O.model_for(spec), 16, 7, 1, 300)
    # from the N(0, 0.25) start the ESS of eight_schools stays above N / 2 up to beta = 1: no resampling, and
    # the first bisection runs out at 1 - 2^-52 (the stage that does not move is the second)
    assert want["status"].tolist() == [0] and want["num_stages"][0] >= 1
    assert got["betas"][0, want["num_stages"][0] - 1] == 1.0


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_eight_schools_other_rows(handles, lanes):
    spec, comp = handles("es", models.eight_schools)
    _check(comp, O.model_for(spec), lanes, 13, 2, 5, max_stages=2)


# ---- resampling ---------------------------------------------------------------------------------------------
def test_forced_and_suppressed_resampling(handles):
    """threshold_ratio = 1.0: the threshold is N, a resampling in nearly every stage, the indices seen through
    the gathered particles; 0.0: none"""
    spec, comp = handles("es", models.eight_schools)
    om = O.model_for(spec)
    _, want = _check(comp, om, 16, 21, 2, 40, threshold_ratio=1.0, max_stages=5, num_mh_steps=1)
    idx = [i for r in want["runs"] for i in r.indices]
    assert sum(i is not None for i in idx) >= len(idx) - 2
    assert any(i is not None and i != list(range(40)) for i in idx)
    _, none = _check(comp, om, 16, 21, 2, 40, threshold_ratio=0.0, max_stages=5, num_mh_steps=1)
    assert all(i is None for r in none["runs"] for i in r.indices)
    assert none["status"].tolist() == [0, 0]


def test_batch_is_the_seeds_and_run_lo_shards(handles):
    spec, comp = handles("es", models.eight_schools)
    kw = dict(num_particles=20, num_mh_steps=2, lanes_per_chain=16, max_stages=6, seed=11)
    whole = smc.sample_raw(comp, kw, 3)
    for r in range(3):
        one = smc.sample_raw(comp, dict(kw, run_lo=r), 1)
        for k in KEYS:
            assert one[k][0].tobytes() == whole[k][r].tobytes(), (r, k)
    alias = smc.sample_raw(comp, dict(kw, seed=11 + 7919 * 2), 1)
    for k in KEYS:
        assert alias[k][0].tobytes() == whole[k][2].tobytes(), k
    assert whole["particles"][0].tobytes() != whole["particles"][1].tobytes()


def test_flat_order_moves_the_variates(hip):
    spec = models.simple()
    comp = sampler.compile(spec)
    try:
        perm = np.array([1, 0], dtype=np.int32)
        comp.check(comp.L.exmc_hip_model_set_flat_order(comp.h, perm.ctypes.data_as(C.POINTER(C.c_int32)), 2))
        om = O.model_for(spec)
        om.set_flat_order([1, 0])
        got, want = _check(comp, om, 1, 21, 1, 6, max_stages=3, num_mh_steps=2)
        plain = _statement(O.model_for(spec), 1, 21, 1, 6, max_stages=3, num_mh_steps=2)
        assert not np.array_equal(plain["particles"], want["particles"])
    finally:
        comp.close()


# ---- generated models: the plug-in's init and mutate, libexmc_hip.so's reweight, the Python stage loop ----
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
            elif name == "signed_log":
                # s ~ N(0, 1) on the whole line and a Custom term log(s): NaN for every s < 0
                ir = cg.IR()
                ir.rv("s", "normal", dict(mu=0.0, sigma=1.0))
                ir.rv("y", "custom", dict(s="s", logpdf=lambda o, _x, p: o.log(p["s"])))
                ir.obs("y_obs", "y", 0.0)
                spec = cg.compile_ir(ir)
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
    spec, comp = generated(name)
    _check(comp, GC.model(spec.gen, lanes), lanes, 9, 2, 5, max_stages=3, num_mh_steps=2)


def test_non_finite_logp_takes_the_constant(generated):
    """starts and proposals with s < 0 have a NaN density: -1.0e10, in the start and in the mutation (the
    statement counts 58 such evaluations). sv_ncp, the input of ADVI's constant branch, stays finite under
    SMC's short proposals: test_sv_ncp_64_lanes runs it."""
    spec, comp = generated("signed_log")
    got, want = _check(comp, GC.model(spec.gen, 1), 1, 3, 1, 24, max_stages=4, num_mh_steps=3)
    run = want["runs"][0]
    assert run.non_finite > 24 // 4
    assert np.isfinite(got["logp"]).all()


def test_reference_tests_restated(generated):
    """smc_test.exs with its literals, each equal to the statement"""
    spec, comp = generated("2.0")
    trace, info = smc.sample(comp, dict(num_particles=200, num_mh_steps=3, seed=42))
    assert set(trace) == {"x"} and trace["x"].shape[0] == 200
    assert abs(float(np.mean(trace["x"])) - 2.0) < 2.0
    assert info["betas"][-1] == 1.0 and info["status"] == 0 and info["num_stages"] == len(info["betas"])
    want = SS.sample_lane(GC.model(spec.gen, 1), 1, 42, num_particles=200, num_mh_steps=3)
    assert np.array_equal(trace["x"].reshape(-1), want.particles.reshape(-1))
    assert info["betas"] == want.betas and info["ess_history"] == want.ess_history
    assert info["acceptance_rates"] == want.acceptance_rates
    spec0, comp0 = generated("0.0")
    _, i0 = smc.sample(comp0, dict(num_particles=100, num_mh_steps=2, seed=42))
    assert all(b1 >= b0 for b0, b1 in zip(i0["betas"], i0["betas"][1:]))
    assert all(0.0 <= a <= 1.0 for a in i0["acceptance_rates"]) and all(e > 0.0 for e in i0["ess_history"])
    traces, infos = smc.sample(comp0, dict(num_particles=20, num_mh_steps=2, seed=42), num_runs=2)
    assert len(traces) == len(infos) == 2 and traces[0]["x"].tobytes() != traces[1]["x"].tobytes()


# ---- the device form -----------------------------------------------------------------------------------------
def test_device_form_null_outputs_and_refusals(handles, generated):
    import torch
    spec, comp = handles("es", models.eight_schools)
    R, N, d, S = 2, 20, spec.d, 6
    host = smc.sample_raw(comp, dict(num_particles=N, num_mh_steps=2, seed=11, lanes_per_chain=16, max_stages=S), R)
    dev = torch.device("cuda", 0)
    q = torch.zeros((d, R * N), dtype=torch.float64, device=dev)
    betas = torch.zeros((S, R), dtype=torch.float64, device=dev)
    ns = torch.zeros(R, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    so = _lib.SmcOpts(N, 0.5, 2, 11, S, 16)
    comp.check(comp.L.exmc_hip_smc(comp.h, so, R, 0, q.data_ptr(), None, betas.data_ptr(), None, None, ns.data_ptr(), None))
    assert comp.last_kernel_ms > 0.0
    assert np.array_equal(q.cpu().numpy().T.reshape(R, N, d), host["particles"])
    assert np.array_equal(betas.cpu().numpy().T, host["betas"], equal_nan=True)
    assert np.array_equal(ns.cpu().numpy(), host["num_stages"])
    comp.check(comp.L.exmc_hip_smc(comp.h, so, R, 0, None, None, None, None, None, None, None))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    st = np.zeros(R, np.int32)
    comp.check(comp.L.exmc_hip_smc_host(comp.h, so, R, 0, dp(), dp(), dp(), dp(), dp(), ip(), st.ctypes.data_as(ip)))
    assert np.array_equal(st, host["status"])

    def call(o, n=R, lo=0):
        return comp.L.exmc_hip_smc_host(comp.h, o, n, lo, dp(), dp(), dp(), dp(), dp(), ip(), st.ctypes.data_as(ip))
    for bad in (_lib.SmcOpts(0, 0.5, 2, 11, S, 16), _lib.SmcOpts(N, 0.5, 0, 11, S, 16),
                _lib.SmcOpts(N, float("nan"), 2, 11, S, 16), _lib.SmcOpts(N, float("inf"), 2, 11, S, 16),
                _lib.SmcOpts(N, 0.5, 2, 11, -1, 16), _lib.SmcOpts(-3, 0.5, 2, 11, S, 16)):
        assert call(bad) == _lib.ERR_BADARG
        assert comp.L.exmc_hip_smc(comp.h, bad, R, 0, None, None, None, None, None, None, None) == _lib.ERR_BADARG
    assert call(so, n=0) == _lib.ERR_BADARG and call(so, lo=-1) == _lib.ERR_BADARG
    assert call(_lib.SmcOpts(1, 0.5, 1, 11, 1, 16)) == 0                          # the smallest of everything
    assert call(_lib.SmcOpts(N, 0.5, 2, 11, S, 5)) == _lib.ERR_UNSUPPORTED        # a lane count not compiled in
    # a plug-in carries init and mutate; the whole run and the model-free front are libexmc_hip.so's
    gspec, gcomp = generated("simple")
    go = _lib.SmcOpts(N, 0.5, 2, 11, S, 1)
    assert gcomp.L.exmc_hip_smc(gcomp.h, go, R, 0, None, None, None, None, None, None, None) == _lib.ERR_UNSUPPORTED
    t = {k: torch.zeros(max(S * R, 2 * R, R * N, gspec.d * R), dtype=torch.float64, device=dev)
         for k, _ in _lib.SmcState._fields_}
    state = _lib.SmcState(*[t[k].data_ptr() for k, _ in _lib.SmcState._fields_])
    gq = torch.zeros((gspec.d, R * N), dtype=torch.float64, device=dev)
    glp = torch.zeros(R * N, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    assert gcomp.L.exmc_hip_smc_reweight(0, go, R, gspec.d, 0, gq.data_ptr(), glp.data_ptr(), state) == _lib.ERR_UNSUPPORTED
    main = _lib.load()
    assert main.exmc_hip_smc_reweight(0, go, R, gspec.d, S + 1, gq.data_ptr(), glp.data_ptr(), state) == _lib.ERR_BADARG
    assert main.exmc_hip_smc_reweight(0, go, R, gspec.d, 0, None, glp.data_ptr(), state) == _lib.ERR_BADARG
    assert main.exmc_hip_smc_reweight(0, go, R, gspec.d, 0, gq.data_ptr(), glp.data_ptr(), _lib.SmcState()) == _lib.ERR_BADARG
