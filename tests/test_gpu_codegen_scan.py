"""Scan chains of the generated 64-lane layout on the GPU: the plug-ins of non-centred sv and of two
random-walk models, their walks evaluated by wave_scan_fwd / wave_scan_bwd (exmc_models.hpp
EXMC_GEN_SCAN_FWD / _BWD), against the same generated text on the CPU (tests/gen_checker.py, whose
scans are the host statement of include/exmc_scan.h) -- bit for bit: value and gradient at ordinary
and hostile points, single transitions, the shared warmup and a batch of chains, the traced walk."""
import ctypes as C

import numpy as np
import pytest

import chain_models as CM
import gen_checker as GC
import oracle as O
import test_gpu_sv_ncp as TN
from exmc_amd import codegen as cg, models, sampler

pytestmark = pytest.mark.gpu

T = 100
CFG = O.Cfg(1, 64)
R = np.asarray(models.sv_returns())


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.fixture(scope="module")
def gsv(hip):
    """non-centred sv from its node list, compiled as the drop-in path compiles it (ncp, scan) for two
    resident waves per SIMD, like the hand-written kind and the bench's gen_sv"""
    hand = models.sv_ncp(R)
    spec = cg.compile_ir(cg.sv_ir(R), ncp=True, name="gen_sv_ncp", default_init=hand.default_init, lanes=64,
                         waves_per_simd=2)
    assert [c["increments"] for c in spec.gen.scan_chains] == [T - 1]
    comp = sampler.compile(spec)
    perm = [hand.var_names.index(n) for n in spec.gen.var_names]   # kind order -> generated order
    yield spec, comp, GC.model(spec.gen, 64), perm
    comp.close()


def _device(comp, q):
    q = np.ascontiguousarray(q)
    lp, g = np.zeros(q.shape[0]), np.zeros_like(q)
    comp.check(comp.L.exmc_hip_logp_grad_host(comp.h, _dp(q), q.shape[0], 64, _dp(lp), _dp(g)))
    return lp, g


def _check_points(comp, om, q):
    lp, g = _device(comp, q)
    for c in range(q.shape[0]):
        olp, og = om.logp_grad(q[c], CFG)
        assert _same(olp, lp[c]), (c, olp, lp[c])
        assert _same(og, g[c]), c


def test_sv_logp_grad_bit_exact(gsv):
    spec, comp, om, perm = gsv
    q = TN._points(97, 1)[:, perm]
    q[0] = spec.to_unconstrained(spec.default_init)
    _check_points(comp, om, np.ascontiguousarray(q))


def test_sv_logp_grad_hostile_operands_bit_exact(gsv):
    """NaN, +-inf, 1e308, denormals in s_1, in z and in log sigma / log nu, both ends of the clamps,
    walks out of the fast window (tests/test_gpu_sv_ncp.py's rows, in the generated order)"""
    spec, comp, om, perm = gsv
    _check_points(comp, om, np.ascontiguousarray(TN._hostile()[:, perm]))


@pytest.mark.parametrize("eps,max_depth", [(0.08, 10), (0.6, 10)])
def test_sv_transitions_bit_exact(gsv, eps, max_depth):
    spec, comp, om, perm = gsv
    rng = np.random.default_rng(9)
    C_, n_draws, D = 13, 6, spec.d
    q = np.ascontiguousarray(TN._points(C_, 10)[:, perm])
    im = np.ascontiguousarray(rng.uniform(0.3, 3.0, size=D))
    g, logp = np.zeros((C_, D)), np.zeros(C_)
    for c in range(C_):
        logp[c], g[c] = om.logp_grad(q[c], CFG)
    rngs = np.zeros((C_, 2), dtype=np.uint64)
    for c in range(C_):
        r = O.Rng()
        O.lib().exo_rng_seed(C.byref(r), 700 + c)
        rngs[c] = (r.a, r.b)
    hq, hg, hl, hr = q.copy(), g.copy(), logp.copy(), rngs.copy()
    t, tr = sampler._host_trace(C_, n_draws, D)
    comp.check(comp.L.exmc_hip_transitions_host(comp.h, _dp(hq), _dp(hl), _dp(hg),
                                               hr.ctypes.data_as(C.POINTER(C.c_uint64)), C_, n_draws,
                                               eps, _dp(im), max_depth, 64, tr))
    o = TN._oracle_transitions(om, spec.flat_order(), q, logp, g, rngs, n_draws, eps, im, max_depth)
    for k in ("tree_depth", "n_steps", "divergent", "draws", "logp", "accept_prob", "energy"):
        assert _same(o[k], t[k]), k


def test_sv_shared_warmup_and_chains_bit_exact(gsv):
    """the bench's protocol at 256 chains x (200 + 200): the shared warmup's step size and inverse
    mass, then the first, a middle and the last chain, every per-draw output"""
    spec, comp, om, _ = gsv
    nw, ns, D = 200, 200, spec.d
    opts = dict(num_warmup=nw, num_samples=ns, seed=42, lanes_per_chain=64)
    tuning = sampler.warmup(comp, spec.default_init, opts)
    q0 = spec.to_unconstrained(spec.default_init)
    st = O.warmup(om, q0, num_warmup=nw, seed=42, cfg=CFG)
    assert st.step_size == tuning["epsilon"]
    assert np.array_equal(np.array(st.inv_mass[:D]), tuning["inv_mass"])
    _, _, extra = sampler.sample_compiled_tuned(comp, tuning, spec.default_init, opts, num_chains=256)
    raw = extra["raw"]
    for c in (0, 131, 255):
        t, _ = O.sample_tuned(om, st.step_size, np.array(st.inv_mass[:D]), q0, num_samples=ns,
                              seed=42 + 7919 * c, cfg=CFG)
        for k in ("tree_depth", "n_steps", "divergent", "draws", "logp", "accept_prob", "energy"):
            assert np.array_equal(t[k], raw[k][c]), (c, k)


def test_sv_traced_walk_is_the_reconstructed_walk(gsv):
    spec, comp, om, _ = gsv
    opts = dict(num_warmup=100, num_samples=30, seed=3)
    trace, st = sampler.sample(spec, spec.default_init, opts)
    t, ost = O.sample(om, spec.to_unconstrained(spec.default_init), num_warmup=100, num_samples=30, seed=3,
                      cfg=CFG)
    raw = st["raw"]["draws"][0]
    assert ost.step_size == st["step_size"] and np.array_equal(t["draws"], raw)
    # Transform.apply per entry, then reconstruct_ncp (sampler.ex:1281-1313), written out here
    x = np.array(raw, dtype=np.float64, copy=True)
    for i, name in enumerate(spec.var_names):
        if spec.gen.transforms.get(name) == "log":
            x[:, i] = np.exp(np.clip(x[:, i], -200.0, 200.0))
    ref = models.reconstruct_ncp(x, spec.var_names, spec.gen.ncp_info)
    for i, name in enumerate(spec.var_names):
        assert np.array_equal(trace[name], ref[:, i]), name
    i50 = spec.var_names.index("s_50")
    assert not np.array_equal(trace["s_50"], raw[:, i50])          # the walk, not z_50


@pytest.mark.parametrize("lengths", [[40, 70], [129]])
def test_random_walk_models_bit_exact(hip, lengths):
    ir = CM.chain_ir(lengths, seed=len(lengths))
    gen = cg.generate(ir, lanes=64)
    assert [c["increments"] for c in gen.scan_chains] == lengths
    spec = cg.GeneratedSpec(gen, cg.build_plugin(gen), name="gen_walk_%d" % len(lengths))
    comp = sampler.compile(spec)
    try:
        om = GC.model(gen, 64)
        rng = np.random.default_rng(5)
        q = np.ascontiguousarray(rng.normal(size=(64, gen.d)) * 0.7)
        q[1] = 40.0
        q[2] = -40.0
        q[3, ::7] = np.nan
        q[4, ::5] = 1e308
        q[5, ::3] = 5e-324
        _check_points(comp, om, q)
        q0 = np.ascontiguousarray(rng.normal(size=gen.d) * 0.1)
        opts = dict(num_warmup=80, num_samples=30, seed=5, lanes_per_chain=64)
        tun = sampler._lib.Tuning()
        tr, t = sampler._host_trace(1, 30, gen.d)
        dv = C.c_int32()
        comp.check(comp.L.exmc_hip_sample_host(comp.h, _dp(q0), sampler._c_opts(sampler._merge_opts(opts)), t,
                                              C.byref(tun), C.byref(dv)))
        ot, ost = O.sample(om, init_q=q0, num_warmup=80, num_samples=30, seed=5, cfg=CFG)
        assert tun.epsilon == ost.step_size
        for k in ("draws", "n_steps", "tree_depth", "divergent", "energy"):
            assert np.array_equal(tr[k][0], ot[k]), k
    finally:
        comp.close()
