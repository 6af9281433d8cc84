"""Model comparison on the device (exmc_amd/csrc/exmc_ic.hpp, include/exmc_hip_compare.h): the pointwise
matrix and the fused statistics of every built-in kind bit for bit against the host statement
(tests/host/ic_host_checker.c); the datum terms tied to the log-density the sampler runs; the model-free
reduction on hostile matrices; argument errors."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ic_checker as IC
from exmc_amd import _lib, models, sampler
from exmc_amd import model_comparison as MC

pytestmark = pytest.mark.gpu

F32 = lambda x: float(np.float32(x))  # noqa: E731
L2P = F32(math.log(F32(2 * math.pi)))


def _spec(kind):
    return {models.SIMPLE: models.simple, models.EIGHT_SCHOOLS: models.eight_schools,
            models.SV: lambda: models.sv(models.sv_returns()),
            models.SV_NCP: lambda: models.sv_ncp(models.sv_returns()),
            models.LOGISTIC: models.logistic, models.RADON: models.radon}[kind]()


KINDS = [models.SIMPLE, models.EIGHT_SCHOOLS, models.SV, models.SV_NCP, models.LOGISTIC, models.RADON]
_traces = {}


def small_trace(kind):
    """8 chains x 50 draws of the kind, then 3 draws of wide random positions (outside the kinds'
    fast windows): a device tensor [S][d][C]"""
    if kind not in _traces:
        spec = _spec(kind)
        comp = sampler.compile(spec)
        opts = dict(num_warmup=60, num_samples=50, seed=7)
        _, stats = sampler.sample_chains_compiled(comp, 8, opts)
        raw = np.asarray(stats[0]["extra"]["raw"]["draws"])          # [C][S][d]
        x = raw.transpose(1, 2, 0)
        rng = np.random.default_rng(kind)
        wide = rng.normal(0.0, 1.0, size=(3, spec.d, 8)) * np.array([1.0, 8.0, 60.0])[:, None, None]
        x = np.concatenate([x, wide], axis=0)
        _traces[kind] = (comp, np.ascontiguousarray(x))
    return _traces[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_pointwise_and_stats_bit_exact(kind, hip):
    comp, x = small_trace(kind)
    blob = comp.spec.data
    xd = torch.from_numpy(x).cuda()
    S, d, Cn = x.shape
    N = MC.n_data(comp)
    ll = torch.empty((S, N, Cn), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    comp.check(comp.L.exmc_hip_pointwise_loglik(comp.h, xd.data_ptr(), S, d, Cn, ll.data_ptr()))
    llh = ll.cpu().numpy()
    want = IC.pointwise(kind, blob, x)
    assert llh.tobytes() == want.tobytes(), np.argwhere(llh != want)[:5]
    # the fused pass == pointwise -> ic_stats_from_ll == the host statement, every call the same bits
    st = MC.pointwise_stats(comp, xd)
    st2 = MC.pointwise_stats(comp, xd)
    assert st.tobytes() == st2.tobytes()
    order = MC._datum_order(comp, N)
    fused = st[:, order]                     # back to the handle's order
    via_ll = MC._stats_from_ll(ll)
    assert fused.tobytes() == via_ll.tobytes()
    assert fused.tobytes() == IC.stats_kind(kind, blob, x).tobytes()
    # the host entry point
    sh = np.zeros((4, N))
    host = np.ascontiguousarray(x.transpose(2, 0, 1))
    comp.check(comp.L.exmc_hip_ic_stats_host(comp.h, host.ctypes.data_as(C.POINTER(C.c_double)), S, d, Cn,
                                             sh.ctypes.data_as(C.POINTER(C.c_double))))
    assert sh.tobytes() == fused.tobytes()


def _prior(kind, spec, q):
    """the non-datum terms of each kind's logp (exmc_models.hpp / oracle/exmc_oracle.c), numpy"""
    c = lambda s: L2P + 2 * math.log(s)  # noqa: E731
    nrm = lambda x, s: -0.5 * ((x / s) ** 2 + c(s))  # noqa: E731
    hc = lambda x, s: (F32(math.log(2 / math.pi)) - math.log(s)) - math.log(1 + (x / s) ** 2)  # noqa: E731
    if kind == models.SIMPLE:
        return nrm(q[0], 5.0) + (-math.exp(q[1]) + q[1])
    if kind == models.EIGHT_SCHOOLS:
        # the kind folds each observation's -0.5 log(2 pi) out of its likelihood (exmc_models.hpp)
        return (nrm(q[0], 5.0) + hc(math.exp(q[1]), 5.0) + q[1] + sum(nrm(t, 1.0) for t in q[2:10])
                - 8 * (-0.5 * L2P))
    if kind in (models.SV, models.SV_NCP):
        sig, nu = math.exp(q[100]), math.exp(q[101])
        p = (F32(math.log(50.0)) - 50.0 * sig + q[100]) + (F32(math.log(F32(0.1))) - F32(0.1) * nu + q[101])
        if kind == models.SV:
            s = q[:100]
            return p + nrm(s[0], sig) + sum(nrm(s[t] - s[t - 1], sig) for t in range(1, 100))
        return p + nrm(q[0], sig) + sum(nrm(z, 1.0) for z in q[1:100])
    if kind == models.LOGISTIC:
        return sum(nrm(v, 10.0) for v in q)
    J = 85
    sa, sy = math.exp(q[J + 2]), math.exp(q[J + 3])
    return (sum(nrm(v, 1.0) for v in q[:J]) + nrm(q[J], 10.0) + nrm(q[J + 1], 5.0) + hc(sa, 2.5) + q[J + 2]
            + hc(sy, 2.5) + q[J + 3] + nrm(q[J + 4], 5.0))


@pytest.mark.parametrize("kind", KINDS)
def test_datum_terms_tie_to_the_samplers_logp(kind, hip):
    comp, x = small_trace(kind)
    q = np.ascontiguousarray(x[10].T[:4])          # 4 sampled positions [4][d]
    lp, g = np.zeros(4), np.zeros((4, comp.d))
    comp.check(comp.L.exmc_hip_logp_grad_host(comp.h, q.ctypes.data_as(C.POINTER(C.c_double)), 4,
                                              comp.default_lanes, lp.ctypes.data_as(C.POINTER(C.c_double)),
                                              g.ctypes.data_as(C.POINTER(C.c_double))))
    for c in range(4):
        total = math.fsum(IC.terms(kind, comp.spec.data, q[c])) + _prior(kind, comp.spec, q[c])
        assert abs(total - lp[c]) <= 1e-11 * abs(lp[c]), (c, total, lp[c])


def test_from_ll_on_hostile_matrices(hip):
    import test_ic_host as H
    ll = H.hostile()
    got = MC._stats_from_ll(torch.from_numpy(ll).cuda())
    assert got.tobytes() == IC.stats_from_ll(ll).tobytes()
    # host arrays are uploaded; the result is the same
    assert MC._stats_from_ll(ll).tobytes() == got.tobytes()


def test_waic_loo_results(hip):
    comp, x = small_trace(models.RADON)
    w, lo = MC.waic(comp, torch.from_numpy(x).cuda()), MC.loo(comp, np.ascontiguousarray(x.transpose(2, 0, 1)))
    st = MC.pointwise_stats(comp, torch.from_numpy(x).cuda())
    assert w["n_obs"] == lo["n_obs"] == st.shape[1]
    assert w == MC.waic_totals(st[0], st[1]) | {"pointwise": w["pointwise"]}
    assert lo["elpd_loo"] == MC.loo_totals(st[2], st[3])["elpd_loo"]
    assert w["pointwise"]["names"][:2] == [("radon", 0), ("radon", 1)]
    # the caller's order: datum k of the handle is observation datum_order[k]
    ll, names = MC.pointwise_log_likelihood(comp, torch.from_numpy(x).cuda())
    order = comp.spec.datum_order
    assert names[0] == ("radon", int(order[0]))
    np.testing.assert_array_equal(st[:, order], MC._stats_from_ll(ll))


def test_errors(hip):
    comp, x = small_trace(models.SIMPLE)
    xd = torch.from_numpy(x).cuda()
    S, d, Cn = x.shape
    out = torch.empty((4, MC.n_data(comp)), dtype=torch.float64, device="cuda")
    L = comp.L
    assert L.exmc_hip_ic_stats(comp.h, xd.data_ptr(), S, d + 1, Cn, out.data_ptr()) == _lib.ERR_BADARG
    assert L.exmc_hip_ic_stats(comp.h, xd.data_ptr(), 1, d, 1, out.data_ptr()) == _lib.ERR_BADARG
    assert L.exmc_hip_ic_stats(comp.h, None, S, d, Cn, out.data_ptr()) == _lib.ERR_BADARG
    assert L.exmc_hip_pointwise_loglik(comp.h, xd.data_ptr(), S, d, Cn, None) == _lib.ERR_BADARG
    assert L.exmc_hip_ic_stats_from_ll(0, None, S, 3, Cn, out.data_ptr()) == _lib.ERR_BADARG
    assert L.exmc_hip_model_n_data(None) < 0
    with pytest.raises(ValueError):
        MC.waic(comp, xd.float())
    with pytest.raises(ValueError):
        MC.waic(comp, xd[0])
    with pytest.raises(ValueError):
        MC.pointwise_log_likelihood(comp, xd, max_bytes=64)
    with pytest.raises(ValueError):
        MC.waic_from_pointwise(torch.zeros((2, 2), dtype=torch.float64, device="cuda"))


def test_plugin_library_refers_to_the_main_library(hip):
    """a generated model's plug-in exports the entry points but carries no comparison kernels: its
    handles have no per-datum terms, and the model-free reduction is libexmc_hip.so's"""
    from exmc_amd import codegen
    P = _lib.bind(codegen.build_plugin(codegen.generate(codegen.simple_ir())))
    for name in _lib.COMPARE_EXPORTS:
        getattr(P, name)
    ll = np.random.default_rng(3).normal(size=(4, 3, 2))
    lld = torch.from_numpy(ll).cuda()
    out = torch.empty((4, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert P.exmc_hip_ic_stats_from_ll(0, lld.data_ptr(), 4, 3, 2, out.data_ptr()) == _lib.ERR_UNSUPPORTED
    assert MC.waic_from_pointwise(lld)["n_obs"] == 3
    assert MC._stats_from_ll(lld).tobytes() == IC.stats_from_ll(ll).tobytes()
