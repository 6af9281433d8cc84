"""Prior and prior predictive samples on the device (exmc_amd/csrc/exmc_prior.hpp, include/exmc_hip_prior.h,
exmc_amd/predictive.py) against the statement of predictive.ex's prior_samples and the sample/2 callbacks
(tests/prior_statement.py), bit for bit: every built-in kind on two wavefronts (the second partial) and on
one chain; continuation through the carried generators; sharding by chain_lo; no replicates; the host form
and the block form; refusals; a generated handle; the tangent on the device against the host build of the
same header; posterior_predictive on the positions. tests/test_prior_statement.py shows on the CPU that
these inputs never reach the gamma cap."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import predictive_inputs as PI
import prior_statement as PR
import test_detmath_tan as DT
from exmc_amd import _lib, models, sampler
from exmc_amd import predictive as PP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_comp = {}


def comp(kind):
    if kind not in _comp:
        _comp[kind] = sampler.compile(PI.spec(kind))
    return _comp[kind]


def device_call(cm, S, Cn, seed, chain_lo, resume=False, state=None, want_state=True, replicates=True):
    """exmc_hip_prior_samples -> (x [S][d][C], q [S][d][C], yrep [S][N][C] or None, state [2][C] uint64 or None)"""
    N = cm.L.exmc_hip_model_n_data(cm.h)
    x = torch.full((S, cm.d, Cn), np.nan, dtype=torch.float64, device="cuda")
    q = torch.full((S, cm.d, Cn), np.nan, dtype=torch.float64, device="cuda")
    out = torch.full((S, N, Cn), np.nan, dtype=torch.float64, device="cuda") if replicates else None
    st = None
    if want_state or state is not None:
        st = torch.from_numpy((np.zeros((2, Cn), np.uint64) if state is None else state).view(np.int64)).cuda()
    torch.cuda.synchronize()
    cm.check(cm.L.exmc_hip_prior_samples(cm.h, _lib.PredictiveOpts(seed, chain_lo, 1 if resume else 0), S, Cn,
                                         None if st is None else st.data_ptr(), x.data_ptr(), q.data_ptr(),
                                         None if out is None else out.data_ptr()))
    return (x.cpu().numpy(), q.cpu().numpy(), None if out is None else out.cpu().numpy(),
            None if st is None else st.cpu().numpy().view(np.uint64))


def _same(got, want):
    return all((g is None and w is None) or g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("Cn", [PR.C_PAR, 1])
@pytest.mark.parametrize("kind", PI.KINDS)
def test_parity_with_the_statement(kind, Cn, hip):
    wx, wq, wy, wstate, n = PR.expected(kind, Cn)
    assert wx.shape[0] == 3 and wx.shape[2] == Cn and n["cap"] == 0
    cm = comp(kind)
    x, q, yrep, state = device_call(cm, PR.S_PAR, Cn, PR.SEED, PR.CHAIN_LO)
    assert x.tobytes() == wx.tobytes(), np.argwhere(x != wx)[:5]
    assert q.tobytes() == wq.tobytes(), np.argwhere(q != wq)[:5]
    assert yrep.tobytes() == wy.tobytes(), np.argwhere(yrep != wy)[:5]
    assert state.tobytes() == wstate.tobytes()
    assert cm.last_kernel_ms > 0.0
    if Cn == 1:
        return
    # the Python call: the same tensors, the reference's map per chain, the datum names in the handle's order
    r = PP.prior_samples(cm, PR.S_PAR, Cn, seed=PR.SEED, chain_lo=PR.CHAIN_LO)
    assert r["x"].cpu().numpy().tobytes() == wx.tobytes() and r["q"].cpu().numpy().tobytes() == wq.tobytes()
    assert r["yrep"].cpu().numpy().tobytes() == wy.tobytes() and len(r["names"]) == wy.shape[1]
    sp = PI.spec(kind)
    for j in (0, sp.d - 1):
        assert r[sp.var_names[j]].shape == (Cn, PR.S_PAR) and r[sp.var_names[j]][5, 2] == wx[2, j, 5]
    if kind == models.RADON:
        assert r["names"][0] == ("radon", int(sp.datum_order[0]))


@pytest.mark.parametrize("kind", PI.KINDS)
def test_continuation_and_sharding(kind, hip):
    cm = comp(kind)
    whole = device_call(cm, 5, 70, 23, 1)
    a = device_call(cm, 2, 70, 23, 1)
    b = device_call(cm, 3, 70, 99, 7, resume=True, state=a[3])      # a resumed call reads neither seed nor chain_lo
    for k in range(3):
        assert np.concatenate([a[k], b[k]]).tobytes() == whole[k].tobytes()
    assert b[3].tobytes() == whole[3].tobytes()
    # chains [0, 70) in one call == [0, 32) and [32, 70) with chain_lo = 32, with or without a state
    lo = device_call(cm, 5, 32, 23, 1)
    hi = device_call(cm, 5, 38, 23, 1 + 32, want_state=False)
    for k in range(3):
        assert np.concatenate([lo[k], hi[k]], axis=2).tobytes() == whole[k].tobytes()
    assert lo[3].tobytes() == np.ascontiguousarray(whole[3][:, :32]).tobytes() and hi[3] is None


@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.SV_NCP])
def test_without_replicates_no_datum_is_drawn(kind, hip):
    cm = comp(kind)
    Cn, S = 70, 2
    wx, wq, wy, wstate, _ = PR.run(PI.spec(kind), S, Cn, seed=41, chain_lo=0, replicates=False)
    x, q, yrep, state = device_call(cm, S, Cn, 41, 0, replicates=False)
    assert wy is None and yrep is None
    assert x.tobytes() == wx.tobytes() and q.tobytes() == wq.tobytes() and state.tobytes() == wstate.tobytes()
    full = device_call(cm, S, Cn, 41, 0)
    assert full[0][0].tobytes() == x[0].tobytes() and full[0][1].tobytes() != x[1].tobytes()
    r = PP.prior_samples(cm, S, Cn, seed=41, replicates=False)
    assert r["yrep"] is None and r["names"] == [] and r["x"].cpu().numpy().tobytes() == wx.tobytes()


@pytest.mark.parametrize("kind", [models.EIGHT_SCHOOLS, models.SV_NCP, models.RADON])
def test_host_form_and_block_form(kind, hip):
    cm = comp(kind)
    S, Cn, d = 5, 70, cm.d
    wx, wq, wy, wst = device_call(cm, S, Cn, 31, 0)
    N = wy.shape[1]
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    hx, hq, hy, hst = np.zeros((Cn, S, d)), np.zeros((Cn, S, d)), np.zeros((Cn, S, N)), np.zeros((2, Cn), np.uint64)
    f = cm.L.exmc_hip_prior_samples_host
    cm.check(f(cm.h, _lib.PredictiveOpts(31, 0, 0), S, Cn, hst.ctypes.data_as(up), hx.ctypes.data_as(dp),
               hq.ctypes.data_as(dp), hy.ctypes.data_as(dp)))
    assert hx.tobytes() == np.ascontiguousarray(wx.transpose(2, 0, 1)).tobytes()
    assert hq.tobytes() == np.ascontiguousarray(wq.transpose(2, 0, 1)).tobytes()
    assert hy.tobytes() == np.ascontiguousarray(wy.transpose(2, 0, 1)).tobytes()
    assert hst.tobytes() == wst.tobytes()
    # ... resumed on the host, and without replicates or a state
    x1, q1, y1 = np.zeros((Cn, 2, d)), np.zeros((Cn, 2, d)), np.zeros((Cn, 2, N))
    cm.check(f(cm.h, _lib.PredictiveOpts(31, 0, 0), 2, Cn, hst.ctypes.data_as(up), x1.ctypes.data_as(dp),
               q1.ctypes.data_as(dp), y1.ctypes.data_as(dp)))
    x2, q2, y2 = np.zeros((Cn, 3, d)), np.zeros((Cn, 3, d)), np.zeros((Cn, 3, N))
    cm.check(f(cm.h, _lib.PredictiveOpts(0, 0, 1), 3, Cn, hst.ctypes.data_as(up), x2.ctypes.data_as(dp),
               q2.ctypes.data_as(dp), y2.ctypes.data_as(dp)))
    assert np.concatenate([x1, x2], axis=1).tobytes() == hx.tobytes() and np.concatenate([y1, y2], axis=1).tobytes() == hy.tobytes()
    assert np.concatenate([q1, q2], axis=1).tobytes() == hq.tobytes() and hst.tobytes() == wst.tobytes()
    x3, q3 = np.zeros((Cn, 1, d)), np.zeros((Cn, 1, d))
    cm.check(f(cm.h, _lib.PredictiveOpts(31, 0, 0), 1, Cn, None, x3.ctypes.data_as(dp), q3.ctypes.data_as(dp), None))
    assert x3.tobytes() == np.ascontiguousarray(hx[:, :1]).tobytes() and q3.tobytes() == np.ascontiguousarray(hq[:, :1]).tobytes()
    # the Python forms: the whole and the blocks joined
    blocks = list(PP.prior_samples_blocks(cm, S, Cn, 2, seed=31))
    assert [s0 for s0, _ in blocks] == [0, 2, 4] and [b["x"].shape[0] for _, b in blocks] == [2, 2, 1]
    for key, want in (("x", wx), ("q", wq), ("yrep", wy)):
        assert torch.cat([b[key] for _, b in blocks]).cpu().numpy().tobytes() == want.tobytes()
    name = PI.spec(kind).var_names[1]
    assert np.concatenate([b[name] for _, b in blocks], axis=1).tobytes() == np.ascontiguousarray(wx[:, 1, :].T).tobytes()
    nbytes = wx.nbytes + wq.nbytes + wy.nbytes
    assert PP.prior_samples(cm, S, Cn, seed=31, max_bytes=nbytes)["yrep"].cpu().numpy().tobytes() == wy.tobytes()
    with pytest.raises(ValueError, match="prior_samples_blocks"):
        PP.prior_samples(cm, S, Cn, seed=31, max_bytes=nbytes - 1)
    assert PP.prior_samples(cm, S, Cn, seed=31, replicates=False, max_bytes=wx.nbytes + wq.nbytes)["yrep"] is None
    with pytest.raises(ValueError):
        next(PP.prior_samples_blocks(cm, S, Cn, 0))


def test_refusals(hip):
    cm = comp(models.SIMPLE)
    S, Cn, d = 2, 3, cm.d
    x = torch.zeros((S, d, Cn), dtype=torch.float64, device="cuda")
    q = torch.zeros((S, d, Cn), dtype=torch.float64, device="cuda")
    out = torch.zeros((S, 10, Cn), dtype=torch.float64, device="cuda")
    st = torch.zeros((2, Cn), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L, O = cm.L, _lib.PredictiveOpts
    f = L.exmc_hip_prior_samples
    assert f(cm.h, O(1, 0, 0), S, Cn, st.data_ptr(), x.data_ptr(), q.data_ptr(), out.data_ptr()) == _lib.OK
    assert f(cm.h, O(1, 0, 1), S, Cn, st.data_ptr(), x.data_ptr(), q.data_ptr(), None) == _lib.OK
    bad = [(cm.h, O(1, 0, 0), S, Cn, None, None, q.data_ptr(), out.data_ptr()),             # no x
           (cm.h, O(1, 0, 0), S, Cn, None, x.data_ptr(), None, out.data_ptr()),             # no q
           (cm.h, O(1, 0, 0), 0, Cn, None, x.data_ptr(), q.data_ptr(), out.data_ptr()),
           (cm.h, O(1, 0, 0), S, 0, None, x.data_ptr(), q.data_ptr(), out.data_ptr()),
           (cm.h, O(1, -1, 0), S, Cn, None, x.data_ptr(), q.data_ptr(), out.data_ptr()),
           (cm.h, O(1, 0, 1), S, Cn, None, x.data_ptr(), q.data_ptr(), out.data_ptr()),     # resume without a state
           (None, O(1, 0, 0), S, Cn, None, x.data_ptr(), q.data_ptr(), out.data_ptr())]
    for args in bad:
        assert f(*args) == _lib.ERR_BADARG, args[1:]
    dp = C.POINTER(C.c_double)
    hx, hq, hy = np.zeros((Cn, S, d)), np.zeros((Cn, S, d)), np.zeros((Cn, S, 10))
    g = L.exmc_hip_prior_samples_host
    assert g(cm.h, O(1, 0, 0), S, Cn, None, hx.ctypes.data_as(dp), hq.ctypes.data_as(dp), hy.ctypes.data_as(dp)) == _lib.OK
    assert g(cm.h, O(1, 0, 0), S, Cn, None, None, hq.ctypes.data_as(dp), hy.ctypes.data_as(dp)) == _lib.ERR_BADARG
    assert g(cm.h, O(1, 0, 0), S, Cn, None, hx.ctypes.data_as(dp), None, hy.ctypes.data_as(dp)) == _lib.ERR_BADARG
    assert g(cm.h, O(1, 0, 1), S, Cn, None, hx.ctypes.data_as(dp), hq.ctypes.data_as(dp), None) == _lib.ERR_BADARG
    assert g(cm.h, O(1, -3, 0), S, Cn, None, hx.ctypes.data_as(dp), hq.ctypes.data_as(dp), None) == _lib.ERR_BADARG
    assert g(cm.h, O(1, 0, 0), 0, Cn, None, hx.ctypes.data_as(dp), hq.ctypes.data_as(dp), None) == _lib.ERR_BADARG
    with pytest.raises(_lib.ExmcHipError):
        PP.prior_samples(cm, 0, 3)
    with pytest.raises(_lib.ExmcHipError):
        PP.prior_samples(cm, 2, 3, chain_lo=-1)


def test_a_generated_handle_is_unsupported(hip):
    from exmc_amd import codegen
    gen = sampler.compile(codegen.compile_ir(codegen.eight_schools_ir(), pointwise=True))
    try:
        for name in _lib.PRIOR_EXPORTS:
            getattr(gen.L, name)
        x = torch.zeros((2, gen.d, 3), dtype=torch.float64, device="cuda")
        q = torch.zeros((2, gen.d, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = gen.L.exmc_hip_prior_samples(gen.h, _lib.PredictiveOpts(1, 0, 0), 2, 3, None, x.data_ptr(), q.data_ptr(), None)
        assert rc == _lib.ERR_UNSUPPORTED
        assert b"prior samples" in gen.L.exmc_hip_last_error()
        dp = C.POINTER(C.c_double)
        hx, hq = np.zeros((3, 2, gen.d)), np.zeros((3, 2, gen.d))
        assert gen.L.exmc_hip_prior_samples_host(gen.h, _lib.PredictiveOpts(1, 0, 0), 2, 3, None, hx.ctypes.data_as(dp),
                                                 hq.ctypes.data_as(dp), None) == _lib.ERR_UNSUPPORTED
        with pytest.raises(_lib.ExmcHipError):
            PP.prior_samples(gen, 2, 3)
    finally:
        gen.close()


def test_device_tangent_equals_the_host_contract(hip, tmp_path):
    """exmc_tan_halfpi on the device (tools/probe/tan_probe.hip) against the host build of the same header,
    bit for bit, on the inputs the accuracy test of tests/test_detmath_tan.py measures, and on arguments
    outside [0, 1]"""
    src = os.path.join(ROOT, "tools", "probe", "tan_probe.hip")
    exe = os.path.join(ROOT, "tools", "probe", "tan_probe")
    hdr = os.path.join(ROOT, "include", "exmc_detmath.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off",
                        "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True)
    u = np.concatenate([DT.tan_inputs(), [-0.0, -5e-324, -1.0, np.nextafter(1.0, 2.0), 2.0, np.inf, -np.inf, np.nan]])
    fin, fout = str(tmp_path / "u.bin"), str(tmp_path / "t.bin")
    u.tofile(fin)
    out = subprocess.run([exe, fin, fout], check=False, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.fromfile(fout, dtype=np.float64)
    want = DT.tan_many(PR.shim(), u)
    assert got.size == u.size
    nan = np.isnan(want)
    assert nan.sum() == 7 and (np.isnan(got) == nan).all()
    assert got[~nan].tobytes() == want[~nan].tobytes(), u[~nan][got[~nan] != want[~nan]][:5]


@pytest.mark.parametrize("kind", PI.KINDS)
def test_posterior_predictive_accepts_the_positions(kind, hip):
    cm = comp(kind)
    r = PP.prior_samples(cm, 3, 70, seed=PR.SEED, chain_lo=PR.CHAIN_LO)
    yrep, names = PP.posterior_predictive(cm, r["q"], seed=5)
    assert names == r["names"] and tuple(yrep.shape) == tuple(r["yrep"].shape)
    q, y = r["q"].cpu().numpy(), yrep.cpu().numpy()
    rows = np.isfinite(q).all(axis=1)                 # [S][C]: the draws whose whole position is finite
    assert rows.all()                                 # (tests/test_prior_statement.py: these positions are finite)
    assert np.isfinite(y[np.broadcast_to(rows[:, None, :], y.shape)]).all()
