"""EXMC_MODEL_SV_NCP on the GPU: SVNcp<64> (exmc_models.hpp) against the checker's statement in the
kernel's order (tests/sv_ncp_checker.py, O.Cfg(1, 64)), bit for bit -- value and gradient, leapfrog
rows, whole transitions, the shared warmup, the bench protocol at full size -- and every public
route of the Python API and of the NIF shim with the kind."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import sv_ncp_checker as S
from exmc_amd import _lib, models, sampler

pytestmark = pytest.mark.gpu

T, D = 100, 102
CFG = O.Cfg(1, 64)
R = np.asarray(models.sv_returns())


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def nc(hip):
    spec = models.sv_ncp(R)
    comp = sampler.compile(spec)
    yield spec, comp, S.model(R)
    comp.close()


def _points(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, D))
    q[:, 0] *= 0.5
    q[:, T] = rng.uniform(-4.0, 0.0, size=n)
    q[:, T + 1] = rng.uniform(0.5, 4.0, size=n)
    return np.ascontiguousarray(q)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _logp_grad_device(comp, q):
    q = np.ascontiguousarray(q)
    lp = np.zeros(q.shape[0])
    g = np.zeros_like(q)
    _lib.check(comp.L.exmc_hip_logp_grad_host(comp.h, _dp(q), q.shape[0], 64, _dp(lp), _dp(g)))
    return lp, g


def test_logp_grad_random_points_bit_exact(nc):
    spec, comp, om = nc
    q = _points(97, 1)
    q[0] = spec.to_unconstrained(spec.default_init)
    lp, g = _logp_grad_device(comp, q)
    for c in range(q.shape[0]):
        olp, og = om.logp_grad(q[c], CFG)
        assert olp == lp[c], (c, olp, lp[c])
        assert np.array_equal(og, g[c]), c


def _hostile():
    base = _points(1, 2)[0]
    rows = []
    for v in (np.nan, np.inf, -np.inf, 1e308, -1e308, 5e-324, -5e-324, 2.2e-308, 0.0, -0.0):
        for i in (0, 1, 37, 63, 64, 99, T, T + 1):
            r = base.copy()
            r[i] = v
            rows.append(r)
    for ls in (-200.0, 200.0, -250.0, 250.0, -199.999, 199.999):   # both ends of the :log clamp
        r = base.copy()
        r[T] = ls
        rows.append(r)
        r = base.copy()
        r[T + 1] = ls
        rows.append(r)
    for scale in (40.0, 400.0, 1e4):                                 # walks out of the fast window
        r = base.copy()
        r[1:T] = scale
        r[T] = 0.0
        rows.append(r)
        r = base.copy()
        r[1:T] = -scale
        rows.append(r)
    r = base.copy()
    r[0] = 1e-300                                                    # s_1 below 2^-380
    rows.append(r)
    r = base.copy()
    r[:T] = 0.0                                                      # the default init: every s_t = 0
    rows.append(r)
    return np.ascontiguousarray(rows)


def test_logp_grad_hostile_operands_bit_exact(nc):
    spec, comp, om = nc
    q = _hostile()
    lp, g = _logp_grad_device(comp, q)
    for c in range(q.shape[0]):
        olp, og = om.logp_grad(q[c], CFG)
        assert _same(olp, lp[c]), (c, olp, lp[c])
        assert _same(og, g[c]), c


@pytest.mark.parametrize("eps", [0.05, -0.05])
def test_multi_step_bit_exact(nc, eps):
    spec, comp, om = nc
    rng = np.random.default_rng(3)
    C_, n = 40, 25
    q = _points(C_, 4)
    p = np.ascontiguousarray(rng.normal(size=(C_, D)))
    im = np.ascontiguousarray(rng.uniform(0.5, 2.0, size=D))
    g = np.array([om.logp_grad(q[c], CFG)[1] for c in range(C_)])
    aq, ap, ag = (np.zeros((C_, n, D)) for _ in range(3))
    alp = np.zeros((C_, n))
    _lib.check(comp.L.exmc_hip_multi_step_host(comp.h, _dp(q), _dp(p), _dp(g), eps, _dp(im), n, C_, 64,
                                               _dp(aq), _dp(ap), _dp(alp), _dp(ag)))
    for c in range(0, C_, 3):
        oq, op, olp, og = om.multi_step(q[c], p[c], g[c], eps, im, n, CFG)
        # steps from a small sigma at unit mass leave the stable range of s_1: NaN rows are expected
        assert _same(oq, aq[c]) and _same(op, ap[c])
        assert _same(olp, alp[c]) and _same(og, ag[c])


def _oracle_transitions(om, flat, q, logp, g, rngs, n_draws, eps, im, max_depth):
    """n_draws NUTS transitions per chain with the checker (sampler.ex:854-925); the momentum is drawn
    in the flat order (sample_momentum_fast, sampler.ex:393-403), which for sv is not the kernel order."""
    L = O.lib()
    C_, d = q.shape
    out = dict(draws=np.zeros((C_, n_draws, d)), logp=np.zeros((C_, n_draws)),
               tree_depth=np.zeros((C_, n_draws), np.int32), n_steps=np.zeros((C_, n_draws), np.int32),
               divergent=np.zeros((C_, n_draws), np.int32), accept_prob=np.zeros((C_, n_draws)),
               energy=np.zeros((C_, n_draws)))
    for c in range(C_):
        r = O.Rng(int(rngs[c, 0]), int(rngs[c, 1]))
        qc, gc, lpc = q[c].copy(), g[c].copy(), float(logp[c])
        for s in range(n_draws):
            p = np.zeros(d)
            for i in flat:
                p[i] = L.exo_rng_normal(C.byref(r), CFG.math_mode) / np.sqrt(im[i])
            jlp0 = lpc - L.exo_kinetic_energy(_dp(p), _dp(im), d, CFG)
            qo, go, res = om.tree_build(qc, p, lpc, gc, eps, im, max_depth, r, jlp0, CFG)
            L.exo_rng_uniform(C.byref(r))
            qc, gc, lpc = qo, go, res.logp
            out["draws"][c, s] = qc
            out["logp"][c, s] = lpc
            out["tree_depth"][c, s] = res.depth
            out["n_steps"][c, s] = res.n_steps
            out["divergent"][c, s] = res.divergent
            out["accept_prob"][c, s] = res.accept_sum / res.n_steps if res.n_steps else 0.0
            out["energy"][c, s] = -jlp0
        rngs[c, 0], rngs[c, 1] = r.a, r.b
        q[c], g[c], logp[c] = qc, gc, lpc
    return out


@pytest.mark.parametrize("eps,max_depth", [(0.08, 10), (0.6, 10), (0.01, 5)])
def test_transitions_bit_exact(nc, eps, max_depth):
    spec, comp, om = nc
    rng = np.random.default_rng(9)
    C_, n_draws = 21, 8
    q = _points(C_, 10)
    im = np.ascontiguousarray(rng.uniform(0.3, 3.0, size=D))
    g = np.zeros((C_, D))
    logp = np.zeros(C_)
    for c in range(C_):
        logp[c], g[c] = om.logp_grad(q[c], CFG)
    rngs = np.zeros((C_, 2), dtype=np.uint64)
    for c in range(C_):
        r = O.Rng()
        O.lib().exo_rng_seed(C.byref(r), 500 + c)
        rngs[c] = (r.a, r.b)
    hq, hg, hl, hr = q.copy(), g.copy(), logp.copy(), rngs.copy()
    t, tr = sampler._host_trace(C_, n_draws, D)
    _lib.check(comp.L.exmc_hip_transitions_host(comp.h, _dp(hq), _dp(hl), _dp(hg),
                                                hr.ctypes.data_as(C.POINTER(C.c_uint64)), C_, n_draws,
                                                eps, _dp(im), max_depth, 64, tr))
    o = _oracle_transitions(om, spec.flat_order(), q, logp, g, rngs, n_draws, eps, im, max_depth)
    for k in ("tree_depth", "n_steps", "divergent", "draws", "logp", "accept_prob", "energy"):
        assert _same(o[k], t[k]), k
    assert np.array_equal(hq, q) and np.array_equal(hg, g) and np.array_equal(hr, rngs)


def test_bench_protocol_full_size_bit_exact(nc):
    """2048 chains x (1000 + 1000) in the bench's protocol: the shared warmup's step size and inverse
    mass, then the first, a middle and the last wavefront's chain, every per-draw output."""
    spec, comp, om = nc
    opts = dict(num_warmup=1000, num_samples=1000, seed=42, lanes_per_chain=64)
    tuning = sampler.warmup(comp, spec.default_init, opts)
    q0 = spec.to_unconstrained(spec.default_init)
    st = O.warmup(om, q0, num_warmup=1000, seed=42, cfg=CFG)
    assert st.step_size == tuning["epsilon"]
    assert np.array_equal(np.array(st.inv_mass[:D]), tuning["inv_mass"])
    _, _, extra = sampler.sample_compiled_tuned(comp, tuning, spec.default_init, opts, num_chains=2048)
    raw = extra["raw"]
    for c in (0, 1023, 2047):
        t, _ = O.sample_tuned(om, st.step_size, np.array(st.inv_mass[:D]), q0, num_samples=1000,
                              seed=42 + 7919 * c, cfg=CFG)
        for k in ("tree_depth", "n_steps", "divergent", "draws", "logp", "accept_prob", "energy"):
            assert np.array_equal(t[k], raw[k][c]), (c, k)


def test_single_chain_sample_and_warm_start_bit_exact(nc):
    spec, comp, om = nc
    q0 = spec.to_unconstrained(spec.default_init)
    trace, st1 = sampler.sample(spec, spec.default_init, dict(num_warmup=300, num_samples=60, seed=3))
    t, st = O.sample(om, q0, num_warmup=300, num_samples=60, seed=3, cfg=CFG)
    assert st.step_size == st1["step_size"]
    assert np.array_equal(t["draws"], st1["raw"]["draws"][0])
    assert st.divergences == st1["divergences"]
    # the trace speaks of s_t: the walk the spec reconstructs from the draws
    x = spec.constrain(st1["raw"]["draws"][0])
    for i, name in enumerate(spec.var_names):
        assert np.array_equal(trace[name], x[:, i]), name
    assert not np.array_equal(trace["s_50"], st1["raw"]["draws"][0][:, 49])
    ws = dict(inv_mass_diag=st1["inv_mass_diag"], step_size=st1["step_size"])
    _, st2 = sampler.sample(spec, spec.default_init, dict(num_warmup=40, num_samples=30, seed=5, warm_start=ws))
    t2, o2 = O.sample_warm(om, ws["step_size"], ws["inv_mass_diag"], q0, num_warmup=40, num_samples=30, seed=5,
                           cfg=CFG)
    assert o2.step_size == st2["step_size"]
    assert np.array_equal(np.array(o2.inv_mass[:D]), st2["inv_mass_diag"])
    assert np.array_equal(t2["draws"], st2["raw"]["draws"][0])


def test_independent_chains_bit_exact(nc):
    """sample_chains(..., vectorized: false): each chain adapts on its own (indep_kernel)."""
    spec, comp, om = nc
    opts = dict(num_warmup=150, num_samples=40, seed=11, lanes_per_chain=64, vectorized=False)
    traces, stats = sampler.sample_chains_independent_compiled(comp, 3, opts)
    raw = stats[0]["extra"]["raw"]
    for c in range(3):
        t, st = O.sample(om, num_warmup=150, num_samples=40, seed=11 + 7919 * c, cfg=CFG)
        assert stats[c]["step_size"] == st.step_size
        assert np.array_equal(raw["draws"][c], t["draws"]), c


def test_sample_stream_equals_sample(nc):
    spec, comp, om = nc
    opts = dict(num_warmup=100, num_samples=25, seed=8, stream_chunk=7)
    trace, stats = sampler.sample(spec, spec.default_init, opts)
    msgs = []
    assert sampler.sample_stream(spec, msgs.append, spec.default_init, opts) == "ok"
    assert msgs[-1] == ("exmc_done", 25) and len(msgs) == 26
    for i, (tag, idx, point, stat) in enumerate(msgs[:-1]):
        assert tag == "exmc_sample" and idx == i + 1
        assert all(point[k] == float(trace[k][i]) for k in trace)


def test_dense_mass_bit_exact(nc):
    spec, comp, om = nc
    opts = dict(num_warmup=300, num_samples=15, seed=13, lanes_per_chain=64, dense_mass=True)
    tuning = sampler.warmup(comp, spec.default_init, opts)
    q0 = spec.to_unconstrained(spec.default_init)
    st, cov, chol = O.warmup_dense(om, q0, num_warmup=300, seed=13, cfg=CFG)
    assert st.step_size == tuning["epsilon"]
    assert np.array_equal(cov, tuning["cov"]) and np.array_equal(chol, tuning["chol_cov"])
    _, _, extra = sampler.sample_compiled_tuned(comp, tuning, spec.default_init, opts, num_chains=2)
    for c in range(2):
        t, _ = O.sample_tuned_dense(om, st.step_size, cov, chol, q0, num_samples=15, seed=13 + 7919 * c, cfg=CFG)
        for k in ("draws", "n_steps", "divergent", "energy"):
            assert np.array_equal(t[k], extra["raw"][k][c]), (c, k)


def test_other_lane_counts_are_unsupported(nc):
    spec, comp, om = nc
    q = _points(2, 5)
    lp = np.zeros(2)
    g = np.zeros_like(q)
    for lanes in (1, 16, 32):
        assert comp.L.exmc_hip_logp_grad_host(comp.h, _dp(q), 2, lanes, _dp(lp), _dp(g)) == 4   # EXMC_ERR_UNSUPPORTED
    assert comp.default_lanes == comp.default_warmup_lanes == comp.default_dense_lanes == 64


def test_nif_model_create_kind_7_equals_the_c_abi(nc, tmp_path_factory):
    import nif_harness as H
    spec, comp, om = nc
    hn = H.build(str(tmp_path_factory.mktemp("nif_ncp")))[1]["HipNative"]
    ok, ref = hn.call("model_create", 7, spec.data)
    assert ok == H.Atom("ok")
    assert hn.call("model_set_flat_order", ref, spec.flat_order()) == H.Atom("ok")
    q = _points(3, 6)
    lp, g = hn.call("logp_grad", ref, q.ravel(), 3)
    dlp, dg = _logp_grad_device(comp, q)
    assert np.array_equal(H.f64(lp), dlp) and np.array_equal(H.f64(g), dg.ravel())
    q0 = spec.to_unconstrained(spec.default_init)
    tun = hn.call("warmup", ref, q0, 100, 10, 0.8, 42)
    t2 = sampler.warmup(comp, spec.default_init, dict(num_warmup=100, seed=42))
    assert tun["epsilon"] == t2["epsilon"] and np.array_equal(H.f64(tun["inv_mass"]), t2["inv_mass"])
    tr, lf, dv = hn.call("sample_chains", ref, tun["epsilon"], H.f64(tun["inv_mass"]), q0, 4, 0, 4, 20, 10, 42)
    _, _, extra = sampler.sample_compiled_tuned(comp, t2, spec.default_init, dict(num_samples=20, seed=42),
                                                num_chains=4)
    assert np.array_equal(H.f64(tr["draws"]).reshape(4, 20, D), extra["raw"]["draws"])
    assert lf == extra["total_leapfrogs"]


def test_sample_chains_vectorized_and_sharded(nc):
    """sample_chains (vectorized) equals the checker's chains, and the two-rank fan-out equals it."""
    spec, comp, om = nc
    opts = dict(num_warmup=120, num_samples=20, seed=21, init_values=spec.default_init)
    t1, s1 = sampler.sample_chains(spec, 3, opts)
    t, st = O.sample_chains(om, 3, init_q=spec.to_unconstrained(spec.default_init), num_warmup=120,
                            num_samples=20, seed=21, cfg=CFG)
    assert st.step_size == s1[0]["step_size"]
    assert np.array_equal(t["draws"], s1[0]["extra"]["raw"]["draws"])
    x = spec.constrain(t["draws"][2])
    assert np.array_equal(t1[2]["s_77"], x[:, 76])
    t2, s2 = sampler.sample_chains(spec, 3, dict(opts, devices=[0, 0]))
    assert np.array_equal(s1[0]["extra"]["raw"]["draws"], s2[0]["extra"]["raw"]["draws"])
    assert all(np.array_equal(t1[c]["s_100"], t2[c]["s_100"]) for c in range(3))
