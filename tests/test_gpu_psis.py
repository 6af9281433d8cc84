"""PSIS-LOO on the device (exmc_amd/csrc/exmc_psis.hpp, include/exmc_hip_compare.h): out [3][N] (elpd_loo,
p_loo, Pareto k) bit for bit against the host statement (tests/host/psis_host_checker.c) on matrices that
take every branch of the kernels and through every built-in kind, whatever the datum blocking; hostile
matrices; errors and handle state; the psis_loo results."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ic_checker as IC
import psis_checker as PC
import test_gpu_handle_state as HS
import test_gpu_model_comparison as TM
import test_psis_host as H
from exmc_amd import _lib, models
from exmc_amd import model_comparison as MC

pytestmark = pytest.mark.gpu


def _dev(ll):
    out, _ = MC._psis_from_ll(torch.from_numpy(np.ascontiguousarray(ll)).cuda())
    return out


def _same(got, want):
    assert got.shape == want.shape
    assert got.tobytes() == want.tobytes(), (np.argwhere(got != want)[:6], got[:, :4], want[:, :4])


# n = 20: M = 4, nothing smoothed; 200: the n / 5 branch, M = 40; 4096: 3 sqrt n, M = 192, 64 chunks to
# merge; 2590: C no multiple of the wavefront, M = 153; 70 000: the chunk grows to 128 samples and
# M = 794 is more than the lanes of a workgroup would hold one each
SIZES = {"n20": (5, 4, 3, 4), "n200": (25, 8, 6, 1), "n4096": (64, 64, 6, 2), "n2590": (37, 70, 5, 3),
         "n70000": (70, 1000, 8, 6)}


@pytest.mark.parametrize("name", list(SIZES))
def test_from_ll_bit_exact(name, hip):
    S, Cn, N, seed = SIZES[name]
    assert PC.tail_len(S * Cn) == {"n20": 4, "n200": 40, "n4096": 192, "n2590": 153, "n70000": 794}[name]
    ll = H.matrix(S, Cn, N, seed)
    want = PC.stats_from_ll(ll)
    got = _dev(ll)
    _same(got, want)
    if name == "n20":
        assert np.all(np.isposinf(got[2]))
    else:
        assert np.all(np.isfinite(got)) and got[2].min() < 0.5 < 0.7 < got[2].max()
    assert _dev(ll).tobytes() == got.tobytes()


def test_tail_sorted_in_global_memory(hip):
    """n = 7.5e6 gives M = 8216 pairs, more than one workgroup sorts in LDS (8192): the tail is sorted in
    the table rows in global memory"""
    S, Cn = 750, 10000
    assert PC.tail_len(S * Cn) == 8216
    ll = H.matrix(S, Cn, 1, 8)
    _same(_dev(ll), PC.stats_from_ll(ll))


def test_ties(hip):
    ll = H.ties()
    want, T = PC.stats_from_ll(ll, tails=True)
    assert list(T) == [100, 130, 192]
    got = _dev(ll)
    _same(got, want)
    assert np.isnan(got[2, 0]) and np.all(np.isfinite(got[2, 1:]))
    # a degenerate fit is a warning too: the NaN datum counts in n_high_k
    r = MC.psis_loo_from_pointwise(ll)
    assert r["n_high_k"] == 1 + int(np.sum(got[2, 1:] > r["k_threshold"]))


def test_hostile_matrix(hip):
    """NaN, +inf, -inf in one datum each void that datum alone; the neighbours are what they are without
    them; the cutoff floor log DBL_MIN applies in datums 2 and 6"""
    ll = H.hostile()
    got = _dev(ll)
    _same(got, PC.stats_from_ll(ll))
    assert np.all(np.isnan(got[:, [1, 3, 5]]))
    ok = [0, 2, 4, 6]
    assert np.all(np.isfinite(got[:2, ok]))
    _same(_dev(ll[:, ok, :]), np.ascontiguousarray(got[:, ok]))
    # host arrays are uploaded; the result is the same
    assert MC._psis_from_ll(ll)[0].tobytes() == got.tobytes()


def _kind_stats(comp, xd, scratch=0):
    S, d, Cn = xd.shape
    N = MC.n_data(comp)
    out = torch.empty((3, N), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    comp.check(comp.L.exmc_hip_psis_stats(comp.h, xd.data_ptr(), S, d, Cn, scratch, out.data_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", TM.KINDS)
def test_kinds_bit_exact_whatever_the_blocking(kind, hip):
    comp, x = TM.small_trace(kind)
    S, d, Cn = x.shape
    N = MC.n_data(comp)
    xd = torch.from_numpy(x).cuda()
    want = PC.stats_from_ll(IC.pointwise(kind, comp.spec.data, x))
    got = _kind_stats(comp, xd)
    _same(got, want)
    # a budget of Nb datums' matrices: at least three blocks, the last one partial
    Nb = max(1, int(N / 2.5))
    assert N % Nb != 0 and -(-N // Nb) >= 3
    _same(_kind_stats(comp, xd, Nb * S * Cn * 8 + 17), got)
    _same(_kind_stats(comp, xd, 1), got)          # below one datum's matrix: one datum per block
    # the model-free form over the device's own matrix, and the host entry point
    ll, _ = MC.pointwise_log_likelihood(comp, xd)
    _same(MC._psis_from_ll(ll)[0], got)
    oh = np.zeros((3, N))
    host = np.ascontiguousarray(x.transpose(2, 0, 1))
    comp.check(comp.L.exmc_hip_psis_stats_host(comp.h, host.ctypes.data_as(C.POINTER(C.c_double)), S, d, Cn, 0,
                                               oh.ctypes.data_as(C.POINTER(C.c_double))))
    _same(oh, got)


def test_logistic_clipped_probabilities_tie_in_the_tail(hip):
    """draws far out: p clips at 1e-7 / 1 - 1e-7, so the largest lr of many datums are exactly equal and
    the order of the tail is decided by the sample index"""
    comp, x = TM.small_trace(models.LOGISTIC)
    rng = np.random.default_rng(21)
    wide = rng.normal(0.0, 60.0, size=(23, x.shape[1], x.shape[2]))
    x2 = np.ascontiguousarray(np.concatenate([x[:30], wide], axis=0))
    ll = IC.pointwise(models.LOGISTIC, comp.spec.data, x2)
    M = PC.tail_len(x2.shape[0] * x2.shape[2])
    top = np.sort(-ll.transpose(1, 0, 2).reshape(ll.shape[1], -1), axis=1)[:, -(M + 1):]
    assert np.mean([len(np.unique(r)) < M // 2 for r in top]) > 0.5     # most datums: ties among the largest
    want, T = PC.stats_from_ll(ll, tails=True)
    assert T.min() < M
    _same(_kind_stats(comp, torch.from_numpy(x2).cuda()), want)


def test_errors(hip):
    comp, x = TM.small_trace(models.SIMPLE)
    xd = torch.from_numpy(x).cuda()
    S, d, Cn = x.shape
    out = torch.empty((3, MC.n_data(comp)), dtype=torch.float64, device="cuda")
    L = comp.L
    assert L.exmc_hip_psis_stats(comp.h, xd.data_ptr(), S, d + 1, Cn, 0, out.data_ptr()) == _lib.ERR_BADARG
    assert L.exmc_hip_psis_stats(comp.h, xd.data_ptr(), 1, d, 1, 0, out.data_ptr()) == _lib.ERR_BADARG
    assert L.exmc_hip_psis_stats(comp.h, None, S, d, Cn, 0, out.data_ptr()) == _lib.ERR_BADARG
    assert L.exmc_hip_psis_stats(comp.h, xd.data_ptr(), S, d, Cn, 0, None) == _lib.ERR_BADARG
    assert L.exmc_hip_psis_stats(None, xd.data_ptr(), S, d, Cn, 0, out.data_ptr()) == _lib.ERR_BADARG
    assert L.exmc_hip_psis_stats_from_ll(0, None, S, 3, Cn, out.data_ptr()) == _lib.ERR_BADARG
    assert L.exmc_hip_psis_stats_from_ll(0, xd.data_ptr(), 1, 3, 1, out.data_ptr()) == _lib.ERR_BADARG
    assert L.exmc_hip_psis_stats_from_ll(0, xd.data_ptr(), 1 << 16, 1, 1 << 15, out.data_ptr()) == _lib.ERR_BADARG
    with pytest.raises(ValueError):
        MC.psis_loo(comp, xd.float())
    with pytest.raises(ValueError):
        MC.psis_loo_from_pointwise(torch.zeros((2, 2), dtype=torch.float64, device="cuda"))


def test_plugin_library_answers_unsupported(hip):
    from exmc_amd import codegen
    P = _lib.bind(codegen.build_plugin(codegen.generate(codegen.simple_ir())))
    for name in _lib.PSIS_EXPORTS:
        getattr(P, name)
    ll = np.random.default_rng(3).normal(size=(4, 3, 2))
    lld = torch.from_numpy(ll).cuda()
    out = torch.empty((3, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert P.exmc_hip_psis_stats_from_ll(0, lld.data_ptr(), 4, 3, 2, out.data_ptr()) == _lib.ERR_UNSUPPORTED
    assert MC.psis_loo_from_pointwise(lld)["n_obs"] == 3


def op_psis(cx, h):
    S, Cn = cx.diag_shape
    x = cx.diag_trace
    L = cx.L
    N = L.exmc_hip_model_n_data(h)
    st = torch.zeros((3, N), dtype=torch.float64, device=cx.dev)
    torch.cuda.synchronize()
    rc = L.exmc_hip_psis_stats(h, x.data_ptr(), S, cx.d, Cn, 0, st.data_ptr())
    if rc:
        return {"rc": rc}
    host = np.ascontiguousarray(x.cpu().numpy().transpose(2, 0, 1))
    sh = np.zeros((3, N))
    rc = L.exmc_hip_psis_stats_host(h, host.ctypes.data_as(C.POINTER(C.c_double)), S, cx.d, Cn, 0,
                                    sh.ctypes.data_as(C.POINTER(C.c_double)))
    if rc:
        return {"rc": rc}
    torch.cuda.synchronize()
    return dict(st=st.cpu().numpy(), sh=sh)


_fresh = {}


def _fresh_psis(cx, cfg):
    if cfg not in _fresh:
        with cx.handle() as h:
            _fresh[cfg] = op_psis(cx, h)
    return _fresh[cfg]


@pytest.mark.parametrize("a", list(HS.OPS))
@pytest.mark.parametrize("cfg", ["es16", "sv64"])
def test_psis_after_and_before_every_op(cfg, a, hip):
    """exmc_hip_psis_stats reads no handle state and leaves none, as test_gpu_ic_handle_state.py holds
    exmc_hip_ic_stats to: after every op of test_gpu_handle_state's catalogue it answers as on a fresh
    handle, and the op after it answers as on a fresh handle"""
    cx = HS.ctx(cfg)
    want = _fresh_psis(cx, cfg)
    assert "rc" not in want and want["st"].tobytes() == want["sh"].tobytes()
    with cx.handle() as h:
        HS.OPS[a](cx, h)
        got = op_psis(cx, h)
    assert HS.same(got, want), a
    with cx.handle() as h:
        op_psis(cx, h)
        got = HS.OPS[a](cx, h)
    assert HS.same(got, HS.expected(cx, a)), HS.diff(got, HS.expected(cx, a))


@pytest.mark.parametrize("cfg", ["es16", "sv64"])
def test_resident_chains_continue_across_psis_stats(cfg, hip):
    cx = HS.ctx(cfg)

    def run(between):
        with cx.handle() as h:
            _lib.check(cx.L.exmc_hip_chains_init(h, C.byref(cx.tun_s), HS._dp(cx.q0), 1, 0, 1,
                                                 cx.opts(0, 0, 31, cx.lanes)), cx.L)
            trd, tr = cx.dev_trace(cx.ns, 1)
            n1 = cx.ns // 2
            rc, lf1, dv1 = HS._advance(cx, h, n1, 0, trd, tr)
            assert rc == 0
            if between:
                assert "rc" not in op_psis(cx, h)
            rc, lf2, dv2 = HS._advance(cx, h, cx.ns - n1, n1, trd, tr)
            assert rc == 0
            return dict(lf=np.array([lf1, lf2]), dv=np.array([dv1, dv2]), **HS._devd(trd))

    assert HS.same(run(True), run(False))


def test_psis_loo_results(hip):
    comp, x = TM.small_trace(models.RADON)
    xd = torch.from_numpy(x).cuda()
    S, d, Cn = x.shape
    r = MC.psis_loo(comp, xd)
    r2 = MC.psis_loo(comp, np.ascontiguousarray(x.transpose(2, 0, 1)), scratch_bytes=100 * S * Cn * 8)
    st, n = MC.psis_pointwise_stats(comp, xd)
    assert n == S * Cn
    assert set(r) == {"loo", "elpd_loo", "p_loo", "se", "n_obs", "pointwise", "k_threshold", "n_high_k"}
    tot = MC.loo_totals(st[0], st[1])
    assert all(r[k] == tot[k] == r2[k] for k in tot)
    assert r["k_threshold"] == min(1 - 1 / math.log10(n), 0.7)
    assert r["n_high_k"] == int(np.sum(~(st[2] <= r["k_threshold"]))) == r2["n_high_k"]
    pw = r["pointwise"]
    assert pw["names"][:2] == [("radon", 0), ("radon", 1)]
    np.testing.assert_array_equal(pw["pareto_k"], st[2])
    np.testing.assert_array_equal(pw["elpd_loo"], st[0])
    # the caller's order: datum k of the handle is observation datum_order[k]
    ll, names = MC.pointwise_log_likelihood(comp, xd)
    order = comp.spec.datum_order
    rf = MC.psis_loo_from_pointwise(ll, names=names)
    np.testing.assert_array_equal(st[:, order], np.stack([rf["pointwise"][k] for k in ("elpd_loo", "p_loo", "pareto_k")]))
    # over the sampled draws alone (the wide ones leave one sample with all the weight, smoothed or not)
    # the smoothed estimate is not the raw one
    xs = xd[:50].contiguous()
    assert np.any(MC.psis_pointwise_stats(comp, xs)[0][0] != MC.pointwise_stats(comp, xs)[2])
    # compare() takes a WAIC and a PSIS result
    ranked = MC.compare([("w", MC.waic(comp, xd)), ("p", r)])
    assert {e["label"] for e in ranked} == {"w", "p"} and ranked[0]["d_elpd"] == 0.0
    assert [e for e in ranked if e["label"] == "p"][0]["elpd"] == r["elpd_loo"]
