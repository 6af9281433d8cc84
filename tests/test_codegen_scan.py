"""Scan chains of the 64-lane layout (exmc_amd/codegen_lanes.py): the random walks the non-centred
rewrite makes (s_k = s_{k-1} + sigma z_k) evaluated as wave-wide prefix / suffix sums. On the CPU the
generated text runs on virtual lanes (tests/gen_checker.py, unchanged), the scans through their host
statement (include/exmc_scan.h); the GPU tests check that the device gives the same bits."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import chain_models as CM
import gen_checker as GC
import gen_models as GM
import oracle as O
import sv_ncp_checker as S
from exmc_amd import codegen as cg, codegen_lanes as cl, models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 100
R = np.asarray(models.sv_returns())

# gen.digest of texts that have no scan chain, recorded before scan chains existed: they stay byte for byte
PINNED = {
    "eight_one_lane": "ee12fa47781c358b",
    "eight_plate": "6ec91d1b3fefcd49",
    "gen_sv": "e034be2966526d8f",
    "gen_radon": "45c4e79337f9a367",
    "gen_logistic": "d05bbc3eadcf1746",
    "sv_ncp_16": "f462f452c485bd39",
    "sv_ncp_64_unrolled": "3d601abb6fbc1176",
    "chain_short": "82216d3431af3771",
}


def _pinned_text(name):
    if name == "eight_one_lane":
        return cg.generate(cg.eight_schools_ir(), vectorize=False)
    if name == "eight_plate":
        return cg.generate(cg.eight_schools_ir())
    if name.startswith("gen_"):
        ir, ncp, _, lanes = GM.baseline_pair(name[4:])
        return cg.generate(ir, ncp=ncp, lanes=lanes)
    if name == "sv_ncp_16":
        return cg.generate(cg.sv_ir(R), ncp=True, lanes=16)
    if name == "sv_ncp_64_unrolled":
        return cg.generate(cg.sv_ir(R), ncp=True, lanes=64, scan=False)
    return cg.generate(CM.chain_ir([cl.MIN_SCAN // 2], seed=1), lanes=64)


@pytest.mark.parametrize("name", sorted(PINNED))
def test_texts_without_scan_chains_are_unchanged(name):
    gen = _pinned_text(name)
    assert gen.digest == PINNED[name]
    assert gen.scan_chains == [] and "EXMC_GEN_SCAN" not in gen.header


def test_sv_ncp_is_one_scan_chain():
    gen = cg.generate(cg.sv_ir(R), ncp=True, lanes=64)
    assert [(c["head"], c["sigma"], c["increments"], c["slots"]) for c in gen.scan_chains] == [("s_1", "sigma", 99, 2)]
    assert (gen.scan_chains[0]["first"], gen.scan_chains[0]["last"]) == ("s_2", "s_100")
    assert len(gen.header) < 40 * 1024
    assert gen.header.count("EXMC_GEN_SCAN_FWD(2, ") == 1 and gen.header.count("EXMC_GEN_SCAN_BWD(2, ") == 1
    # the likelihood's 100 terms are ONE family again (s_1 gathered from the position, s_2.. from the walk)
    assert gen.lane_layout["family_sizes"] == [100, 99]
    assert cg.generate(cg.sv_ir(R), ncp=True, lanes=64, scan=False).scan_chains == []


def _sv_points(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, T + 2))
    q[:, 0] *= 0.3
    q[:, T] = rng.uniform(np.log(0.02), np.log(1.0), size=n)
    q[:, T + 1] = rng.uniform(np.log(2.0), np.log(60.0), size=n)
    return q


def _close(lp_a, g_a, lp_b, g_b):
    assert abs(lp_a - lp_b) <= 1e-12 * max(1.0, abs(lp_b)), (lp_a, lp_b)
    np.testing.assert_allclose(g_a, g_b, rtol=1e-11, atol=1e-12)


def test_sv_scan_text_agrees_with_the_kind_checker():
    gen = cg.generate(cg.sv_ir(R), ncp=True, lanes=64)
    assert gen.scan_chains
    spec = models.sv_ncp(R)
    perm = [spec.var_names.index(n) for n in gen.var_names]
    for q in _sv_points(20, 3):
        lp_g, g_g = GC.logp_grad(gen, q[perm], lanes=64)
        for dev in (True, False):
            lp_c, g_c = S.logp_grad(R, q, dev=dev)
            _close(lp_c, g_c[perm], lp_g, g_g)


def test_sv_scan_text_agrees_with_numpy_and_central_differences():
    import test_sv_ncp_model as TS
    gen = cg.generate(cg.sv_ir(R), ncp=True, lanes=64)
    spec = models.sv_ncp(R)
    perm = [spec.var_names.index(n) for n in gen.var_names]
    for q in _sv_points(8, 4):
        lp_n, g_n = TS._numpy_statement(R, q)
        lp_g, g_g = GC.logp_grad(gen, q[perm], lanes=64)
        assert abs(lp_g - lp_n) <= 1e-11 * max(1.0, abs(lp_n))
        np.testing.assert_allclose(g_g, g_n[perm], rtol=1e-9, atol=1e-10)
    q = _sv_points(1, 5)[0][perm]
    _, g = GC.logp_grad(gen, q, lanes=64)
    h = 1e-6
    for i in range(gen.d):
        a, b = q.copy(), q.copy()
        a[i] += h
        b[i] -= h
        fd = (GC.logp_grad(gen, a, lanes=64)[0] - GC.logp_grad(gen, b, lanes=64)[0]) / (2 * h)
        assert abs(fd - g[i]) <= 1e-5 * max(1.0, abs(g[i])), (gen.var_names[i], fd, g[i])


_SHIM = r"""
#include <math.h>
#include "exmc_detmath.h"
#include "exmc_scan.h"
/* sv's walk through the product header: x = (s_1, sigma z_2, ..., sigma z_100, 0, ...) */
void walk_fwd(const double* q, double* out) {
  const double sigma = exmc_exp(fmax(-200.0, fmin(q[100], 200.0)));
  for (int i = 0; i < 128; i++) out[i] = (i == 0) ? q[0] : ((i < 100) ? sigma * q[i] : 0.0);
  exmc_scan_fwd64(out, 2);
}
void scan_fwd(double* x, int n) { exmc_scan_fwd64(x, n); }
void scan_bwd(double* x, int n) { exmc_scan_bwd64(x, n); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("scan_shim")
    src, so = d / "shim.c", d / "shim.so"
    src.write_text(_SHIM)
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                           "-I", os.path.join(ROOT, "include"), "-shared", "-o", str(so), str(src), "-lm"])
    L = C.CDLL(str(so))
    dp = C.POINTER(C.c_double)
    L.walk_fwd.argtypes = [dp, dp]
    L.scan_fwd.argtypes = L.scan_bwd.argtypes = [dp, C.c_int]
    return L


def test_host_scan_header_equals_the_kind_checker_walk(shim):
    rng = np.random.default_rng(6)
    for q in _sv_points(30, 7):
        q = np.ascontiguousarray(q * rng.uniform(0.1, 30.0))
        out = np.zeros(128)
        shim.walk_fwd(O.dptr(q), O.dptr(out))
        assert np.array_equal(out[:T], S.walk(q, dev=True))
        assert np.all(out[T:] == out[T - 1])          # the padding adds exact zeros


def test_host_backward_scan_is_the_mirror_of_the_forward_one(shim):
    rng = np.random.default_rng(8)
    for n in (1, 2, 3, 4):
        x = rng.normal(size=64 * n) * np.exp(rng.normal(size=64 * n) * 3.0)
        f = np.ascontiguousarray(x[::-1])
        shim.scan_fwd(O.dptr(f), n)
        b = np.ascontiguousarray(x.copy())
        shim.scan_bwd(O.dptr(b), n)
        assert np.array_equal(b, f[::-1])
        np.testing.assert_allclose(b, np.cumsum(x[::-1])[::-1], rtol=1e-12, atol=1e-12 * np.abs(x).sum())


def _agree(ir, n=12, seed=0):
    """scan text against the model's own scan=False text, 1e-12 relative (to the gradient's scale)"""
    gs = cg.generate(ir, lanes=64)
    gu = cg.generate(ir, lanes=64, scan=False)
    assert gu.scan_chains == []
    rng = np.random.default_rng(seed)
    for t in range(n):
        q = rng.normal(size=gs.d) * (0.3 + t % 3)
        for i, name in enumerate(gs.var_names):
            if name.startswith(("sig", "tau")):
                q[i] = rng.uniform(-3.0, 0.5)
        lp_s, g_s = GC.logp_grad(gs, q, lanes=64)
        lp_u, g_u = GC.logp_grad(gu, q, lanes=64)
        assert abs(lp_s - lp_u) <= 1e-12 * max(1.0, abs(lp_u)), (t, lp_s, lp_u)
        assert np.all(np.abs(g_s - g_u) <= 1e-12 * max(1.0, np.max(np.abs(g_u)))), t
    return gs


@pytest.mark.parametrize("m", [cl.MIN_SCAN - 1, cl.MIN_SCAN, cl.MIN_SCAN + 1, 63, 64, 65, 128, 129, 254])
def test_random_walk_lengths(m):
    gs = _agree(CM.chain_ir([m], seed=m), seed=m)
    if m < cl.MIN_SCAN:
        assert gs.scan_chains == [] and gs.digest == cg.generate(CM.chain_ir([m], seed=m), lanes=64, scan=False).digest
    else:
        assert [(c["head"], c["increments"], c["slots"]) for c in gs.scan_chains] == [("w0_1", m, (m + 64) // 64)]
    if m == 254:
        assert gs.d == 256


def test_two_disjoint_walks():
    gs = _agree(CM.chain_ir([40, 70], seed=2), seed=2)
    assert [(c["head"], c["sigma"], c["increments"]) for c in gs.scan_chains] == [("w0_1", "sig0", 40), ("w1_1", "sig1", 70)]


@pytest.mark.parametrize("head", ["log", "ncp"])
def test_heads_that_are_transformed_or_non_centred(head):
    gs = _agree(CM.chain_ir([50], seed=3, head=head), seed=3)
    assert [(c["head"], c["increments"]) for c in gs.scan_chains] == [("w0_1", 50)]


def test_a_branch_ends_the_chain():
    """w0_20 is the mu of w0_21 and b_1: the walk up to w0_20 is one chain, w0_21.. and b_1..b_5 start
    chains of their own with head w0_20. b_1..b_5 is too short for a scan, so it reads w0_20 in the
    uniform part; the chain up to w0_20 is then not scanned and w0_20 is an unrolled value."""
    ir = CM.chain_ir([60], seed=4, branch=20)
    found = cl.find_chains(*_chain_input(ir))
    assert [(c.ids[0], c.ids[-1], c.head_id) for c in found] == [("b_1", "b_5", "w0_20"), ("w0_2", "w0_20", "w0_1"),
                                                                  ("w0_21", "w0_61", "w0_20")]
    gs = _agree(ir, seed=4)
    assert [(c["first"], c["last"], c["head"]) for c in gs.scan_chains] == [("w0_21", "w0_61", "w0_20")]


def test_a_change_of_sigma_splits_the_path():
    ir = CM.chain_ir([60], seed=5, sigma_split=30)
    found = cl.find_chains(*_chain_input(ir))
    assert [(c.ids[0], c.ids[-1], c.sigma_id) for c in found] == [("w0_2", "w0_30", "sig0"), ("w0_31", "w0_61", "sigb0")]
    gs = _agree(ir, seed=5)
    # the second chain's head is a step of the first, which the uniform part then evaluates unrolled
    assert [(c["first"], c["last"], c["head"]) for c in gs.scan_chains] == [("w0_31", "w0_61", "w0_30")]


def _chain_input(ir):
    """(graph, ncp_info, ncp_nodes) as generate hands them to find_chains"""
    seen = {}
    orig = cl.find_chains

    def spy(g, info, nodes):
        seen["args"] = (g, info, dict(nodes))
        return orig(g, info, nodes)
    cl.find_chains = spy
    try:
        cg.generate(ir, lanes=64)
    finally:
        cl.find_chains = orig
    return seen["args"]


def test_other_layouts_keep_the_unrolled_walk():
    ir = CM.chain_ir([40], seed=6)
    for lanes in (16, 32):
        assert cg.generate(ir, lanes=lanes).scan_chains == []
    assert cg.generate(ir, lanes=64, ncp=False).scan_chains == []


def test_scan_key_round_trips_through_json(tmp_path):
    rng = np.random.default_rng(9)
    nodes = {"sigma": {"op": "rv", "dist": "exponential", "params": {"lambda": 4.0}, "transform": "log"},
             "x_1": {"op": "rv", "dist": "normal", "params": {"mu": 0.0, "sigma": 1.0}, "transform": None}}
    for k in range(2, 42):
        nodes["x_%d" % k] = {"op": "rv", "dist": "normal", "params": {"mu": "x_%d" % (k - 1), "sigma": "sigma"},
                             "transform": None}
    for k in range(1, 42):
        nodes["y_%d" % k] = {"op": "rv", "dist": "normal", "params": {"mu": "x_%d" % k, "sigma": 0.5}, "transform": None}
        nodes["o_%d" % k] = {"op": "obs", "target": "y_%d" % k, "value": float(rng.normal())}
    metas = {}
    for scan in (True, False, None):
        doc = {"ncp": True, "lanes": 64, "nodes": nodes}
        if scan is not None:
            doc["scan"] = scan
        src = tmp_path / ("m_%s.json" % scan)
        src.write_text(json.dumps(doc))
        cg.main([str(src), str(tmp_path / ("out_%s" % scan)), "--no-build"])
        metas[scan] = json.loads((tmp_path / ("out_%s" % scan) / "model.json").read_text())
        gen = cg.generate(cg.ir_from_json(doc), lanes=64, scan=scan is not False)
        assert metas[scan]["digest"] == gen.digest
        assert (tmp_path / ("out_%s" % scan) / "exmc_gen_model.h").read_text() == gen.header
    assert metas[True]["scan"] is True and metas[None]["scan"] is True and metas[False]["scan"] is False
    assert metas[None]["digest"] == metas[True]["digest"] != metas[False]["digest"]
    assert [(c["head"], c["increments"]) for c in metas[True]["scan_chains"]] == [("x_1", 40)]
    assert metas[False]["scan_chains"] == []
