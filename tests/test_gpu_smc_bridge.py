"""Bridged SMC on the GPU (include/exmc_hip_smc_bridge.h, exmc_smc.hpp) against its statement in lane mode
(tests/smc_bridge_statement.py): particles, logp, logb, the three histories, log_evidence_steps (NaN where
the statement has none), log_evidence, num_stages and status bit for bit, for every model kind's default
layout, eight_schools' other rows and generated models; both weights paths, the threshold's ends, a base
from a fit, batches, the non-finite branch, the flat order, NULL outputs and the refusals."""
import ctypes as C

import numpy as np
import pytest

import gen_checker as GC
import oracle as O
import smc_bridge_statement as SB
import smc_statement as SS
import sv_ncp_checker as SN
from exmc_amd import _lib, models, sampler, smc
from test_gpu_smc import generated, handles  # noqa: F401  (module-scoped fixtures: the compiled handles)

pytestmark = pytest.mark.gpu

KEYS = ("particles", "logp", "logb", "betas", "ess_history", "acceptance_rates", "log_evidence_steps", "log_evidence",
        "num_stages", "status")


def _statement(om, lanes, seed, n_runs, n, run_lo=0, max_stages=SS.DEFAULT_MAX_STAGES, **kw):
    rs = [SB.sample_lane(om, lanes, seed, num_particles=n, run=run_lo + r, max_stages=max_stages, **kw)
          for r in range(n_runs)]
    out = SB.padded(rs, max_stages)
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


def _check(comp, om, lanes, seed, n_runs, n, base=None, **kw):
    got = smc.sample_bridged_raw(comp, dict(kw, seed=seed, num_particles=n, lanes_per_chain=lanes), n_runs, base=base)
    kw.pop("run_lo", None)
    if base is not None:
        kw["mu"], kw["sigma"] = smc._base(base, om.d)
    want = _statement(om, lanes, seed, n_runs, n, **kw)
    _assert_same(got, want, (lanes, seed, n, kw))
    return got, want


# ---- each kind's default row: N = 3 (a wavefront with empty lane groups, two runs) and N = 70 (more than
# one wavefront at every G), 2 MH steps; max_stages = 4 for the wide kinds ---------------------------------
def _both(comp, om, lanes, seed, **kw):
    _check(comp, om, lanes, seed, 2, 3, num_mh_steps=2, **kw)
    return _check(comp, om, lanes, seed, 1, 70, num_mh_steps=2, **kw)


def test_simple_one_lane(handles):
    spec, comp = handles("simple", models.simple)
    _, want = _both(comp, O.model_for(spec), 1, 3, max_stages=12)
    run = want["runs"][0]
    assert run.status == 0 and run.num_stages >= 2 and not run.bisect[0][2] and run.bisect[-1][2]


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
    got, want = _check(comp, O.model_for(spec), 1, 31, 1, 300)
    n = want["num_stages"][0]
    assert want["status"].tolist() == [0] and got["betas"][0, n - 1] == 1.0
    assert got["log_evidence"][0] == want["runs"][0].log_evidence
    # the estimator end to end: tests/test_smc_bridge_statement.py holds these runs to a quadrature of log p(y)
    assert -8.8 < got["log_evidence"][0] < -6.8


def test_eight_schools_to_the_end(handles):
    spec, comp = handles("es", models.eight_schools)
    got, want = _check(comp, O.model_for(spec), 16, 7, 1, 300)
    n = want["num_stages"][0]
    assert want["status"].tolist() == [0] and got["betas"][0, n - 1] == 1.0
    # with the start divided out the temper of eight_schools has real stages, each one resampled
    assert n >= 3 and all(i is not None for i in want["runs"][0].indices)
    betas = want["runs"][0].betas
    assert all(b1 - b0 > 1e-6 for b0, b1 in zip([0.0] + betas, betas))


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_eight_schools_other_rows(handles, lanes):
    spec, comp = handles("es", models.eight_schools)
    _check(comp, O.model_for(spec), lanes, 13, 2, 5, max_stages=2)


def test_weights_from_l2_above_4096_particles(handles):
    """N = 4100: the run's log ratios do not fit the LDS array of the weights kernel, and the cumulative sums
    have a second block"""
    spec, comp = handles("simple", models.simple)
    _, want = _check(comp, O.model_for(spec), 1, 5, 1, 4100, num_mh_steps=1, max_stages=2)
    assert not want["runs"][0].bisect[0][2]          # the first stage went through the bisection


def test_threshold_ratio_zero_and_one(handles):
    """0.0: the ESS at 1.0 - beta is always at or above the threshold: one stage. 1.0: the threshold is N, the
    evaluation at 1.0 is (nearly) never enough and the bisection ends within 1.0 of N"""
    spec, comp = handles("es", models.eight_schools)
    om = O.model_for(spec)
    _, zero = _check(comp, om, 16, 21, 2, 40, threshold_ratio=0.0, max_stages=5, num_mh_steps=1)
    assert zero["num_stages"].tolist() == [1, 1] and zero["status"].tolist() == [0, 0]
    assert all(r.bisect == [(0, False, True)] for r in zero["runs"])
    _, one = _check(comp, om, 16, 21, 2, 40, threshold_ratio=1.0, max_stages=5, num_mh_steps=1)
    assert all(not b[2] for r in one["runs"] for b in r.bisect)
    assert any(i != list(range(40)) for r in one["runs"] for i in r.indices)


def test_base_from_a_fit(handles):
    """an ADVI-shaped base: mu and log_sigma per dimension in kernel order"""
    spec, comp = handles("es", models.eight_schools)
    rng = np.random.default_rng(4)
    base = dict(mu=rng.normal(size=spec.d) * 0.3, log_sigma=rng.normal(size=spec.d) * 0.2 - 0.1, elbo=-40.0)
    got, want = _check(comp, O.model_for(spec), 16, 9, 2, 40, base=base, max_stages=6, num_mh_steps=2)
    plain = smc.sample_bridged_raw(comp, dict(seed=9, num_particles=40, lanes_per_chain=16, max_stages=6, num_mh_steps=2), 2)
    assert not np.array_equal(plain["particles"], got["particles"])
    # (mu, sigma) is the same base
    mu, sigma = smc._base(base, spec.d)
    pair = smc.sample_bridged_raw(comp, dict(seed=9, num_particles=40, lanes_per_chain=16, max_stages=6, num_mh_steps=2), 2,
                                  base=(mu, sigma))
    for k in KEYS:
        assert pair[k].tobytes() == got[k].tobytes(), k


def test_batch_is_the_seeds_and_run_lo_shards(handles):
    spec, comp = handles("es", models.eight_schools)
    kw = dict(num_particles=20, num_mh_steps=2, lanes_per_chain=16, max_stages=6, seed=11)
    whole = smc.sample_bridged_raw(comp, kw, 3)
    for r in range(3):
        one = smc.sample_bridged_raw(comp, dict(kw, run_lo=r), 1)
        for k in KEYS:
            assert one[k][0].tobytes() == whole[k][r].tobytes(), (r, k)
    alias = smc.sample_bridged_raw(comp, dict(kw, seed=11 + 7919 * 2), 1)
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
        base = (np.array([0.5, -0.25]), np.array([0.75, 1.25]))       # the base stays in kernel order
        got, want = _check(comp, om, 1, 21, 1, 6, base=base, max_stages=3, num_mh_steps=2)
        plain = _statement(O.model_for(spec), 1, 21, 1, 6, max_stages=3, num_mh_steps=2, mu=base[0], sigma=base[1])
        assert not np.array_equal(plain["particles"], want["particles"])
    finally:
        comp.close()


# ---- generated models: the plug-in's init and mutate, libexmc_hip.so's reweight, the Python stage loop ----
@pytest.mark.parametrize("name,lanes", [("simple", 1), ("es", 16), ("sv_ncp", 64)])
def test_generated_models(generated, name, lanes):
    spec, comp = generated(name)
    _check(comp, GC.model(spec.gen, lanes), lanes, 9, 2, 5, max_stages=3, num_mh_steps=2)


def test_generated_model_with_a_base(generated):
    spec, comp = generated("es")
    rng = np.random.default_rng(6)
    base = (rng.normal(size=spec.d) * 0.2, np.exp(rng.normal(size=spec.d) * 0.2))
    _check(comp, GC.model(spec.gen, 16), 16, 9, 2, 5, base=base, max_stages=3, num_mh_steps=2)


def test_non_finite_logp_takes_the_constant(generated):
    """starts and proposals with s < 0 have a NaN density: -1.0e10 in the start and in the mutation; their
    weights are zero against the finite half's and the evidence stays finite"""
    spec, comp = generated("signed_log")
    got, want = _check(comp, GC.model(spec.gen, 1), 1, 3, 1, 24, max_stages=4, num_mh_steps=3)
    run = want["runs"][0]
    assert run.non_finite > 24 // 4
    assert np.isfinite(got["logp"]).all() and np.isfinite(got["log_evidence"]).all()


def test_sample_bridged_and_the_pooled_evidence(generated):
    spec, comp = generated("2.0")
    trace, info = smc.sample_bridged(comp, dict(num_particles=200, num_mh_steps=3, seed=42))
    assert set(trace) == {"x"} and trace["x"].shape[0] == 200
    want = SB.sample_lane(GC.model(spec.gen, 1), 1, 42, num_particles=200, num_mh_steps=3)
    assert np.array_equal(trace["x"].reshape(-1), want.particles.reshape(-1))
    assert info["betas"] == want.betas and info["ess_history"] == want.ess_history
    assert info["acceptance_rates"] == want.acceptance_rates and info["status"] == 0
    assert info["log_evidence"] == want.log_evidence and info["log_evidence_steps"] == want.log_evidence_steps
    assert set(info) == {"num_stages", "betas", "ess_history", "acceptance_rates", "status", "log_evidence",
                         "log_evidence_steps"}
    # x ~ N(2, 1) alone is a normalised density: log Z = 0, and a base equal to it gives 0 to rounding
    assert abs(info["log_evidence"]) < 0.5
    _, exact = smc.sample_bridged(comp, dict(num_particles=50, num_mh_steps=1, seed=1), base=([2.0], [1.0]))
    assert exact["num_stages"] == 1 and abs(exact["log_evidence"]) < 1e-6
    traces, infos = smc.sample_bridged(comp, dict(num_particles=20, num_mh_steps=2, seed=42), num_runs=2)
    assert len(traces) == len(infos) == 2 and traces[0]["x"].tobytes() != traces[1]["x"].tobytes()
    pooled = smc.pooled_log_evidence(infos)
    assert min(i["log_evidence"] for i in infos) <= pooled <= max(i["log_evidence"] for i in infos)
    assert pooled == SB.pooled_log_evidence([i["log_evidence"] for i in infos])


# ---- the device form -----------------------------------------------------------------------------------------
def test_device_form_null_outputs_and_refusals(handles, generated):
    import torch
    spec, comp = handles("es", models.eight_schools)
    R, N, d, S = 2, 20, spec.d, 6
    opts = dict(num_particles=N, num_mh_steps=2, seed=11, lanes_per_chain=16, max_stages=S)
    host = smc.sample_bridged_raw(comp, opts, R)
    dev = torch.device("cuda", 0)
    f8 = dict(dtype=torch.float64, device=dev)
    q, lb, le, les = torch.zeros((d, R * N), **f8), torch.zeros(R * N, **f8), torch.zeros(R, **f8), torch.zeros((S, R), **f8)
    ns = torch.zeros(R, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    so = _lib.SmcOpts(N, 0.5, 2, 11, S, 16)
    Lb = comp.L.exmc_hip_smc_bridge
    comp.check(Lb(comp.h, so, R, 0, None, None, q.data_ptr(), None, lb.data_ptr(), None, None, None, ns.data_ptr(), None,
                  le.data_ptr(), les.data_ptr()))
    assert comp.last_kernel_ms > 0.0
    assert np.array_equal(q.cpu().numpy().T.reshape(R, N, d), host["particles"])
    assert np.array_equal(lb.cpu().numpy().reshape(R, N), host["logb"])
    assert np.array_equal(le.cpu().numpy(), host["log_evidence"])
    assert np.array_equal(les.cpu().numpy().T, host["log_evidence_steps"], equal_nan=True)
    assert np.array_equal(ns.cpu().numpy(), host["num_stages"])
    nulls = [None] * 10
    comp.check(Lb(comp.h, so, R, 0, None, None, *nulls))
    # a device base: the default's values given explicitly are the default
    mu_d, sg_d = torch.zeros(d, **f8), torch.full((d,), 0.5, **f8)
    torch.cuda.synchronize()
    comp.check(Lb(comp.h, so, R, 0, mu_d.data_ptr(), sg_d.data_ptr(), q.data_ptr(), *nulls[:7], le.data_ptr(), None))
    assert np.array_equal(q.cpu().numpy().T.reshape(R, N, d), host["particles"])
    assert np.array_equal(le.cpu().numpy(), host["log_evidence"])
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ev = np.zeros(R)

    def call(o, n=R, lo=0, mu=None, sigma=None):
        return comp.L.exmc_hip_smc_bridge_host(
            comp.h, o, n, lo, mu.ctypes.data_as(dp) if mu is not None else dp(),
            sigma.ctypes.data_as(dp) if sigma is not None else dp(), dp(), dp(), dp(), dp(), dp(), dp(), ip(), ip(),
            ev.ctypes.data_as(dp), dp())
    assert call(so) == 0 and np.array_equal(ev, host["log_evidence"])
    for bad in (_lib.SmcOpts(0, 0.5, 2, 11, S, 16), _lib.SmcOpts(N, 0.5, 0, 11, S, 16),
                _lib.SmcOpts(N, float("nan"), 2, 11, S, 16), _lib.SmcOpts(N, float("inf"), 2, 11, S, 16),
                _lib.SmcOpts(N, 0.5, 2, 11, -1, 16), _lib.SmcOpts(-3, 0.5, 2, 11, S, 16)):
        assert call(bad) == _lib.ERR_BADARG
        assert Lb(comp.h, bad, R, 0, None, None, *nulls) == _lib.ERR_BADARG
    assert call(so, n=0) == _lib.ERR_BADARG and call(so, lo=-1) == _lib.ERR_BADARG
    assert call(_lib.SmcOpts(1, 0.5, 1, 11, 1, 16)) == 0                          # the smallest of everything
    assert call(_lib.SmcOpts(N, 0.5, 2, 11, S, 5)) == _lib.ERR_UNSUPPORTED        # a lane count not compiled in
    # the base: finite, sigma > 0
    ok_mu, ok_sg = np.zeros(d), np.full(d, 0.5)
    assert call(so, mu=ok_mu, sigma=ok_sg) == 0 and np.array_equal(ev, host["log_evidence"])
    for i, v in ((0, 0.0), (d - 1, -1.0), (3, float("nan")), (3, float("inf"))):
        sg = ok_sg.copy()
        sg[i] = v
        assert call(so, sigma=sg) == _lib.ERR_BADARG and b"base" in comp.L.exmc_hip_last_error()
    for v in (float("nan"), float("-inf")):
        mu = ok_mu.copy()
        mu[d - 1] = v
        assert call(so, mu=mu) == _lib.ERR_BADARG
    bad_sg = torch.full((d,), -0.5, **f8)
    torch.cuda.synchronize()
    assert Lb(comp.h, so, R, 0, None, bad_sg.data_ptr(), *nulls) == _lib.ERR_BADARG
    # a plug-in carries init and mutate; the whole run and the model-free front are libexmc_hip.so's
    gspec, gcomp = generated("simple")
    go = _lib.SmcOpts(N, 0.5, 2, 11, S, 1)
    assert gcomp.L.exmc_hip_smc_bridge(gcomp.h, go, R, 0, None, None, *nulls) == _lib.ERR_UNSUPPORTED
    assert gcomp.L.exmc_hip_smc_bridge_host(gcomp.h, go, R, 0, dp(), dp(), dp(), dp(), dp(), dp(), dp(), dp(), ip(), ip(),
                                            ev.ctypes.data_as(dp), dp()) == _lib.ERR_UNSUPPORTED
    t = {k: torch.zeros(max(S * R, 2 * R, R * N, gspec.d * R), **f8) for k, _ in _lib.SmcState._fields_}
    state = _lib.SmcState(*[t[k].data_ptr() for k, _ in _lib.SmcState._fields_])
    gq, glp, glb = torch.zeros((gspec.d, R * N), **f8), torch.zeros(R * N, **f8), torch.zeros(R * N, **f8)
    gle, gles = torch.zeros(R, **f8), torch.zeros((S, R), **f8)
    words = torch.zeros((2, R * N), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    rw = (gq.data_ptr(), glp.data_ptr(), glb.data_ptr(), state, gle.data_ptr(), gles.data_ptr())
    assert gcomp.L.exmc_hip_smc_bridge_reweight(0, go, R, gspec.d, 0, *rw) == _lib.ERR_UNSUPPORTED
    main = _lib.load()
    assert main.exmc_hip_smc_bridge_reweight(0, go, R, gspec.d, S + 1, *rw) == _lib.ERR_BADARG
    assert main.exmc_hip_smc_bridge_reweight(0, go, R, gspec.d, 0, None, *rw[1:]) == _lib.ERR_BADARG
    assert main.exmc_hip_smc_bridge_reweight(0, go, R, gspec.d, 0, gq.data_ptr(), glp.data_ptr(), None, *rw[3:]) == _lib.ERR_BADARG
    assert main.exmc_hip_smc_bridge_reweight(0, go, R, gspec.d, 0, *rw[:4], None, gles.data_ptr()) == _lib.ERR_BADARG
    assert main.exmc_hip_smc_bridge_reweight(0, go, R, gspec.d, 0, *rw[:3], _lib.SmcState(), *rw[4:]) == _lib.ERR_BADARG
    init = gcomp.L.exmc_hip_smc_bridge_init
    args = (gq.data_ptr(), glp.data_ptr(), glb.data_ptr(), words.data_ptr(), state, gle.data_ptr(), gles.data_ptr())
    gbad = torch.zeros(gspec.d, **f8)
    torch.cuda.synchronize()
    assert init(gcomp.h, go, R, 0, None, gbad.data_ptr(), *args) == _lib.ERR_BADARG        # sigma = 0
    assert init(gcomp.h, go, R, 0, None, None, gq.data_ptr(), glp.data_ptr(), None, *args[3:]) == _lib.ERR_BADARG
    assert init(gcomp.h, go, R, 0, None, None, *args[:5], None, gles.data_ptr()) == _lib.ERR_BADARG
    assert gcomp.L.exmc_hip_smc_bridge_mutate(gcomp.h, go, R, None, None, gq.data_ptr(), glp.data_ptr(), None,
                                              words.data_ptr(), state) == _lib.ERR_BADARG
