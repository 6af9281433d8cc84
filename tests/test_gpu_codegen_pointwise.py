"""The per-datum terms of generated models on the device: gen_pointwise_kernel against the same text
compiled for the host (tests/gen_pointwise_checker.py) bit for bit, the range entry point of both
libraries, waic / loo / psis_loo of a generated handle composed across the two libraries, the reference's
integration tests 17-19 without a host likelihood, and the handle-state rules of the new entry point."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gen_models as GM
import gen_pointwise_checker as PC
import pw_models as PM
import test_gpu_handle_state as HS
import test_gpu_model_comparison as TM
from exmc_amd import _lib, models, sampler
from exmc_amd import codegen as cg
from exmc_amd import model_comparison as MC

pytestmark = pytest.mark.gpu

SHAPES = [(7, 3), (5, 67), (40, 64)]   # one ragged wavefront; chains straddle a wavefront; full blocks
MODELS = {
    "simple": lambda: cg.simple_ir(),
    "long": PM.long_ir,                        # 37 datums: two generated functions and a partial third
    "eight_schools": lambda: cg.eight_schools_ir(),
    "survival": GM.survival_ir,                # weighted, masked, censored, mean, logsumexp
    "walk24": lambda: PM.walk_ir(22),          # the lane layout only (d = 24)
}
_comps = {}


def comp_of(name):
    if name not in _comps:
        _comps[name] = sampler.compile(cg.compile_ir(MODELS[name](), name="pw_" + name, pointwise=True))
    return _comps[name]


# values that leave the fast ranges of exp / log, put into some samples of a wavefront and not others
HOSTILE = [np.nan, np.inf, -np.inf, 745.2, -745.2, 1e308, -1e308, 5e-324, -1e-310, 0.0, -0.0, 200.5, -200.5]


def trace(d, S, Cn, seed=0, hostile=True):
    rng = np.random.default_rng(1000 * S + Cn + seed)
    x = rng.normal(size=(S, d, Cn)) * 0.7
    if hostile:
        n = S * Cn
        for k, v in enumerate(HOSTILE):
            kk = (5 * k + 2) % n
            x[kk // Cn, (3 * k) % d, kk % Cn] = v
        for j in range(d):                       # a NaN in every dimension (a clamped one swallows it)
            kk = (7 * j + 1) % n
            x[kk // Cn, j, kk % Cn] = np.nan
    return np.ascontiguousarray(x)


def host_matrix(gen, x, i0=0, i1=None):
    """ll [S][nb][C] by the host-compiled text"""
    return np.ascontiguousarray(PC.terms(gen, x.transpose(0, 2, 1), i0, i1).transpose(0, 2, 1))


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def dev_range(comp, xd, i0, nb):
    S, d, Cn = xd.shape
    ll = torch.full((S, max(nb, 1), Cn), -7.0, dtype=torch.float64, device="cuda")   # (a refused nb < 1 writes nothing)
    torch.cuda.synchronize()
    rc = comp.L.exmc_hip_pointwise_loglik_range(comp.h, xd.data_ptr(), S, d, Cn, i0, nb, ll.data_ptr())
    return rc, ll.cpu().numpy()


@pytest.mark.parametrize("S,Cn", SHAPES)
@pytest.mark.parametrize("name", list(MODELS))
def test_matrix_equals_the_host_compiled_text(name, S, Cn, hip):
    comp = comp_of(name)
    gen = comp.spec.gen
    x = trace(gen.d, S, Cn)
    ll, names = MC.pointwise_log_likelihood(comp, torch.from_numpy(x).cuda())
    assert names == gen.datum_names == MC.datum_names(comp) and len(names) == MC.n_data(comp) == gen.n_datums
    got, want = ll.cpu().numpy(), host_matrix(gen, x)
    assert got.shape == (S, gen.n_datums, Cn)
    assert np.isnan(want).any() and np.isfinite(want).any()      # (the test's own inputs do what they are for)
    assert same(got, want), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]


@pytest.mark.parametrize("name", ["long", "survival"])
def test_ranges_are_the_matching_columns(name, hip):
    comp = comp_of(name)
    N = comp.spec.gen.n_datums
    x = trace(comp.d, 5, 67)
    xd = torch.from_numpy(x).cuda()
    rc, full = dev_range(comp, xd, 0, N)
    assert rc == 0 and same(full, host_matrix(comp.spec.gen, x))
    for i0, nb in [(3, N - 3), (0, 1), (N - 1, 1), (15, 2), (16, 1), (5, 13), (N // 2, N - N // 2)]:
        rc, part = dev_range(comp, xd, i0, nb)
        assert rc == 0 and same(part, full[:, i0:i0 + nb, :]), (i0, nb)
    for i0, nb in [(-1, 2), (0, 0), (0, N + 1), (N, 1), (3, N - 2), (2, -1)]:
        assert dev_range(comp, xd, i0, nb)[0] == _lib.ERR_BADARG, (i0, nb)
    assert comp.L.exmc_hip_pointwise_loglik_range(comp.h, 0, 5, comp.d, 67, 0, 1, xd.data_ptr()) == _lib.ERR_BADARG
    assert dev_range(comp, torch.zeros((5, comp.d + 1, 67), dtype=torch.float64, device="cuda"), 0, 1)[0] == _lib.ERR_BADARG


def _pointwise_arrays_equal(a, b):
    assert a["pointwise"]["names"] == b["pointwise"]["names"]
    for k, v in a["pointwise"].items():
        if k != "names":
            assert same(v, b["pointwise"][k]), k
    for k in a:
        if k != "pointwise":
            assert same(a[k], b[k]) if isinstance(a[k], float) else a[k] == b[k], k


@pytest.mark.parametrize("S,Cn", SHAPES)
def test_waic_loo_psis_equal_the_full_matrix_whatever_the_blocking(S, Cn, hip):
    comp = comp_of("long")
    N = comp.spec.gen.n_datums
    x = trace(comp.d, S, Cn, hostile=False)
    xd = torch.from_numpy(x).cuda()
    ll, names = MC.pointwise_log_likelihood(comp, xd)
    assert names == comp.spec.datum_names
    want = (MC.waic_from_pointwise(ll, names), MC.loo_from_pointwise(ll, names), MC.psis_loo_from_pointwise(ll, names))
    per = 8 * S * Cn
    for scratch in (1, per, per * 16 + 8, per * N, 0):   # one datum per block (twice), 16 + 16 + 5, one block, default
        _pointwise_arrays_equal(MC.waic(comp, xd, scratch_bytes=scratch), want[0])
        _pointwise_arrays_equal(MC.loo(comp, xd, scratch_bytes=scratch), want[1])
        _pointwise_arrays_equal(MC.psis_loo(comp, xd, scratch_bytes=scratch), want[2])
    st = MC.pointwise_stats(comp, xd, scratch_bytes=per * 16)
    assert st.shape == (4, N) and same(st, MC._stats_from_ll(ll))
    # the reductions themselves stay with libexmc_hip.so
    out = torch.empty((4, N), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L = comp.L
    assert L.exmc_hip_ic_stats(comp.h, xd.data_ptr(), S, comp.d, Cn, out.data_ptr()) == _lib.ERR_UNSUPPORTED
    assert b"exmc_hip_pointwise_loglik_range" in L.exmc_hip_last_error()
    assert L.exmc_hip_psis_stats(comp.h, xd.data_ptr(), S, comp.d, Cn, 0, out.data_ptr()) == _lib.ERR_UNSUPPORTED
    assert L.exmc_hip_ic_stats_from_ll(0, ll.data_ptr(), S, N, Cn, out.data_ptr()) == _lib.ERR_UNSUPPORTED


# ---- integration_test.exs 17-19 (:513-607): literals and assertions, no host likelihood ----------------
OPTS = dict(num_warmup=300, num_samples=300, seed=42)


def _sampled(ir, name):
    comp = sampler.compile(cg.compile_ir(ir, name=name, pointwise=True))
    trace_, _ = sampler.sample(comp, {}, OPTS)
    mu = np.asarray(trace_["mu"], dtype=np.float64)
    return comp, np.ascontiguousarray(mu.reshape(1, -1, 1))       # host [C][S][d]


def test_17_waic_on_normal_normal(hip):
    comp, tr = _sampled(PM.ref_ir(0.0, 10.0, [("x", 5.0)]), "pw_ref17")
    ll, names = MC.pointwise_log_likelihood(comp, tr)
    assert tuple(ll.shape) == (300, 1, 1) and names == ["x_obs"]
    llh = ll.cpu().numpy()
    assert np.all(np.isfinite(llh)) and np.all(llh < 0.0)
    r = MC.waic(comp, tr)
    for k in ("waic", "elpd_waic", "p_waic", "se"):
        assert isinstance(r[k], float)
    assert r["n_obs"] == 1
    assert r["waic"] > 0.0
    assert 0.0 < r["p_waic"] < 5.0


def test_18_better_model_has_lower_waic(hip):
    good = MC.waic(*_sampled(PM.ref_ir(5.0, 1.0, [("x", 5.0)]), "pw_ref18_good"))
    bad = MC.waic(*_sampled(PM.ref_ir(0.0, 1.0, [("x", 5.0)]), "pw_ref18_bad"))
    assert good["elpd_waic"] > bad["elpd_waic"], (good["elpd_waic"], bad["elpd_waic"])
    assert MC.compare([("good", good), ("bad", bad)])[0]["label"] == "good"


def test_19_loo_over_two_observations(hip):
    comp, tr = _sampled(PM.ref_ir(0.0, 10.0, [("x1", 4.0), ("x2", 5.0)]), "pw_ref19")
    r = MC.loo(comp, tr)
    assert r["pointwise"]["names"] == ["x1_obs", "x2_obs"]
    for k in ("loo", "elpd_loo", "p_loo", "se"):
        assert isinstance(r[k], float)
    assert r["n_obs"] == 2
    assert r["loo"] > 0.0


# ---- against the hand-written kind ------------------------------------------------------------------
def test_generated_eight_schools_agrees_with_the_kind(hip):
    """One trace, the kind's fused pass against the generated terms reduced through the model-free entry
    points. DESIGN.md holds the kind's terms to 1e-11 of logp's (other exp / log forms, the same
    -1/2 log 2 pi); lppd_i and elpd_loo_i are log-mean-exps of n = 400 such terms, a mean of
    perturbations of that size: 1e-10 relative."""
    spec = models.eight_schools()
    kind = sampler.compile(spec)
    _, stats = sampler.sample_chains_compiled(kind, 8, dict(num_warmup=60, num_samples=50, seed=7))
    xk = np.ascontiguousarray(np.asarray(stats[0]["extra"]["raw"]["draws"]).transpose(1, 2, 0))   # [S][d][C]
    comp = comp_of("eight_schools")
    # the kind's theta_trans_j is the generated model's non-centred theta_j: one flat order
    assert [n.replace("theta_trans_", "theta_") for n in spec.var_names] == comp.spec.var_names
    xg = xk
    a = MC.pointwise_stats(kind, torch.from_numpy(xk).cuda())
    b = MC.pointwise_stats(comp, torch.from_numpy(xg).cuda())
    assert MC.datum_names(kind) == MC.datum_names(comp)
    for row, nm in ((0, "lppd"), (2, "elpd_loo")):
        gap = np.max(np.abs(a[row] - b[row]) / np.abs(a[row]))
        print("eight schools, generated against kind: max relative gap of %s = %.3g" % (nm, gap))
        assert gap <= 1e-10, (nm, gap)


# ---- libexmc_hip.so's range entry point -----------------------------------------------------------
@pytest.mark.parametrize("kind", [models.SIMPLE, models.RADON])
def test_kinds_ranges_are_the_matching_columns(kind, hip):
    comp, x = TM.small_trace(kind)
    xd = torch.from_numpy(x).cuda()
    S, d, Cn = x.shape
    N = MC.n_data(comp)
    full = torch.empty((S, N, Cn), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    comp.check(comp.L.exmc_hip_pointwise_loglik(comp.h, xd.data_ptr(), S, d, Cn, full.data_ptr()))
    full = full.cpu().numpy()
    for i0, nb in [(0, N), (3, N - 3), (N - 1, 1), (1, 2), (N // 3, N // 2)]:
        rc, part = dev_range(comp, xd, i0, nb)
        assert rc == 0 and same(part, full[:, i0:i0 + nb, :]), (i0, nb)
    for i0, nb in [(-1, 1), (0, 0), (0, N + 1), (N, 1)]:
        assert dev_range(comp, xd, i0, nb)[0] == _lib.ERR_BADARG


def test_default_built_plugin_has_no_per_datum_terms(hip):
    comp = sampler.compile(cg.compile_ir(cg.simple_ir(), name="pw_plain"))
    for name in _lib.POINTWISE_EXPORTS:
        getattr(comp.L, name)
    xd = torch.zeros((4, comp.d, 2), dtype=torch.float64, device="cuda")
    assert comp.L.exmc_hip_model_n_data(comp.h) < 0
    assert dev_range(comp, xd, 0, 1)[0] == _lib.ERR_UNSUPPORTED
    assert comp.spec.datum_names is None
    with pytest.raises(_lib.ExmcHipError, match="from_pointwise"):
        MC.waic(comp, xd)


# ---- the three build forms --------------------------------------------------------------------------
def test_build_forms_give_identical_matrices(hip, monkeypatch):
    gen = cg.generate(cg.simple_ir(), pointwise=True)
    x = trace(gen.d, 5, 67)
    xd = torch.from_numpy(x).cuda()
    want = host_matrix(gen, x)
    for env in (None, "EXMC_PLUGIN_STUBS", "EXMC_PLUGIN_ONE_TU"):
        with monkeypatch.context() as mp:
            if env:
                mp.setenv(env, "1")
            so = cg.build_plugin(gen)
        comp = sampler.compile(cg.GeneratedSpec(gen, so, name="pw_forms"))
        rc, got = dev_range(comp, xd, 0, gen.n_datums)
        assert rc == 0 and same(got, want), env


# ---- handle state -----------------------------------------------------------------------------------
def op_range(cx, h):
    """the new entry point as an op of test_gpu_handle_state's catalogue: all datums, and a block"""
    S, Cn = cx.diag_shape
    x = cx.diag_trace
    N = cx.L.exmc_hip_model_n_data(h)
    out = {}
    for key, i0, nb in (("all", 0, N), ("block", 1, N - 2)):
        ll = torch.zeros((S, nb, Cn), dtype=torch.float64, device=cx.dev)
        torch.cuda.synchronize()
        rc = cx.L.exmc_hip_pointwise_loglik_range(h, x.data_ptr(), S, cx.d, Cn, i0, nb, ll.data_ptr())
        if rc:
            return {"rc": rc}
        out[key] = ll.cpu().numpy()
    return out


_ctxs, _fresh = {}, {}


def state_ctx(cfg):
    """es16: a kind on libexmc_hip.so; pw_walk16: test_gpu_handle_state's generated configuration built
    with per-datum terms (its Ctx compiles through codegen.compile_ir)"""
    if cfg not in _ctxs:
        if cfg == "es16":
            _ctxs[cfg] = HS.ctx("es16")
        else:
            orig = cg.compile_ir
            cg.compile_ir = lambda *a, **k: orig(*a, pointwise=True, **k)
            try:
                _ctxs[cfg] = HS.Ctx("walk16")
            finally:
                cg.compile_ir = orig
            # the swap took effect: the spec, the text and the library of THIS context carry the terms
            cx = _ctxs[cfg]
            assert cx.spec.n_datums == 7 and "#define EXMC_GEN_POINTWISE 1" in cx.spec.gen.header
            assert cx.spec.lib_path == cg.plugin_paths(cx.spec.gen)[2]
            with cx.handle() as h:
                assert cx.L.exmc_hip_model_n_data(h) == 7
    return _ctxs[cfg]


def _fresh_range(cx, cfg):
    if cfg not in _fresh:
        with cx.handle() as h:
            _fresh[cfg] = op_range(cx, h)
    return _fresh[cfg]


@pytest.mark.parametrize("a", list(HS.OPS))
@pytest.mark.parametrize("cfg", ["es16", "pw_walk16"])
def test_range_after_and_before_every_op(cfg, a, hip):
    """the pair rule: after every op of the catalogue the entry point answers as on a fresh handle, and
    the op after it answers as on a fresh handle"""
    cx = state_ctx(cfg)
    want = _fresh_range(cx, cfg)
    assert "rc" not in want and same(want["block"], want["all"][:, 1:-1, :])
    with cx.handle() as h:
        HS.OPS[a](cx, h)
        got = op_range(cx, h)
    assert HS.same(got, want), a
    with cx.handle() as h:
        op_range(cx, h)
        got = HS.OPS[a](cx, h)
    assert HS.same(got, HS.expected(cx, a)), HS.diff(got, HS.expected(cx, a))


@pytest.mark.parametrize("cfg", ["es16", "pw_walk16"])
def test_resident_chains_continue_across_the_range_call(cfg, hip):
    """the continuation rule: resident chains advance to the same bits with the call in between"""
    cx = state_ctx(cfg)

    def run(between):
        with cx.handle() as h:
            _lib.check(cx.L.exmc_hip_chains_init(h, C.byref(cx.tun_s), HS._dp(cx.q0), 1, 0, 1,
                                                 cx.opts(0, 0, 31, cx.lanes)), cx.L)
            trd, tr = cx.dev_trace(cx.ns, 1)
            n1 = cx.ns // 2
            rc, lf1, dv1 = HS._advance(cx, h, n1, 0, trd, tr)
            assert rc == 0
            if between:
                assert "rc" not in op_range(cx, h)
            rc, lf2, dv2 = HS._advance(cx, h, cx.ns - n1, n1, trd, tr)
            assert rc == 0
            return dict(lf=np.array([lf1, lf2]), dv=np.array([dv1, dv2]), **HS._devd(trd))

    assert HS.same(run(True), run(False))
