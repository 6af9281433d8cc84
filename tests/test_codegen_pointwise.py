"""The per-datum terms of generated models (exmc_amd/codegen.py generate(pointwise=True)) without a
GPU: what a datum is, the emitted section compiled for the host (tests/gen_pointwise_checker.py) against
numpy statements that share no code with the generator, and the C ABI of the new entry point."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gen_checker
import gen_models
import gen_pointwise_checker as PC
import pw_models as PM
from exmc_amd import _lib
from exmc_amd import codegen as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _q(d, n=20, seed=1, scale=0.8):
    return np.random.default_rng(seed).normal(size=(n, d)) * scale


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


# ---- the default text -----------------------------------------------------------------------------
@pytest.mark.parametrize("make", [cg.simple_ir, cg.eight_schools_ir, lambda: PM.walk_ir(22)],
                         ids=["simple", "eight_schools", "walk24_lanes"])
def test_default_text_is_unchanged_and_the_section_is_an_addition(make):
    plain, off, on = cg.generate(make()), cg.generate(make(), pointwise=False), cg.generate(make(), pointwise=True)
    assert plain.header == off.header and plain.digest == off.digest
    assert plain.datum_names is None and plain.n_datums == -1
    head = "#ifndef EXMC_GEN_PW_SECTION\n"
    assert on.header.startswith(head + plain.header)
    added = on.header[len(head) + len(plain.header):]
    assert added.startswith("#if !defined(EXMC_GEN_VEC_SECTION) && !defined(EXMC_GEN_LANES_SECTION)\n")
    assert added.endswith("#endif   /* EXMC_GEN_PW_SECTION */\n")
    assert "#define EXMC_GEN_POINTWISE 1\n" in added and "EXMC_GEN_PW" not in plain.header
    assert on.digest != plain.digest                       # the plug-in cache keeps the two forms apart
    assert np.array_equal(on.data[:plain.data.size], plain.data)
    # the wrapper of the existing checker compiles the longer header: same log-density, same gradient
    for q in _q(plain.d, n=3):
        a, ga = gen_checker.logp_grad(plain, q, lanes=plain.lanes)
        b, gb = gen_checker.logp_grad(on, q, lanes=on.lanes)
        assert _same_bits(a, b) and _same_bits(ga, gb)


# ---- names and counts -----------------------------------------------------------------------------
def _names(ir, **kw):
    return cg.generate(ir, pointwise=True, **kw).datum_names


def test_scalar_and_vector_obs_names():
    assert _names(cg.eight_schools_ir()) == ["y_obs_%d" % j for j in range(8)]
    assert _names(cg.simple_ir([1.0, 2.0, 3.0])) == [("y_obs", 0), ("y_obs", 1), ("y_obs", 2)]


def test_what_counts_as_a_datum():
    assert _names(PM.meta_ir()) == [
        ("a_w", 0), ("a_w", 1), ("a_w", 2),
        ("b_mask", 0), ("b_mask", 2), ("b_mask", 4),          # switched-off elements dropped, indices kept
        "c_mean", "d_lse",                                     # one datum each; e_off, f_meas: none
        ("g_left", 0), ("g_left", 1), "h_right", ("i_int", 0), ("i_int", 1),
        "k_custom", "l_mv"]                                    # (j_masked_scalar: switched off)


def test_weight_and_mask_are_in_the_datum_and_reductions_are_the_logp_term():
    gen = cg.generate(PM.meta_ir(), pointwise=True)
    q = _q(gen.d, n=5)
    t = PC.terms(gen, q)
    nm = gen.datum_names
    s = np.exp(PM.clamp200(q[:, 1]))
    ll = lambda v: PM.normal_logpdf(v, q[:, 0], s)   # noqa: E731
    np.testing.assert_allclose(t[:, nm.index(("a_w", 1))], ll(0.2) * 0.5, rtol=1e-12)
    np.testing.assert_allclose(t[:, nm.index(("b_mask", 4))], ll(0.5) * 2.0, rtol=1e-12)
    np.testing.assert_allclose(t[:, nm.index("c_mean")], (ll(0.5) + ll(0.6)) / 2.0, rtol=1e-12)
    e = np.stack([ll(0.5), ll(0.6), ll(0.7)])
    np.testing.assert_allclose(t[:, nm.index("d_lse")], np.log(np.sum(np.exp(e - e.max(0)), 0)) + e.max(0), rtol=1e-12)
    np.testing.assert_allclose(t[:, nm.index("k_custom")],
                               sum(PM.normal_logpdf(v, q[:, 0], 1.0) for v in (0.4, -1.1, 2.0)), rtol=1e-12)
    assert np.all(t[:, nm.index("l_mv")] == t[0, nm.index("l_mv")])      # no q in it: a constant column


def test_term_order_of_more_than_32_nodes_is_followed():
    obs = [("x%02d" % i, 0.1 * i) for i in range(17)]
    ir = PM.ref_ir(0.0, 10.0, obs)                   # 35 nodes
    order = sorted(ir.nodes, reverse=True)
    ir.order(order)
    assert _names(ir) == [i for i in order if i.endswith("_obs")]
    assert _names(PM.ref_ir(0.0, 10.0, obs)) == sorted(i for i in order if i.endswith("_obs"))


def test_a_model_without_a_datum_raises():
    ir = PM.no_datum_ir()
    cg.generate(ir)
    with pytest.raises(cg.CodegenError, match="no datum"):
        cg.generate(ir, pointwise=True)


# ---- values ---------------------------------------------------------------------------------------
def test_normal_terms_equal_the_numpy_statement():
    gen = cg.generate(PM.ref_ir(0.0, 10.0, [("x1", 4.0), ("x2", 5.0)]), pointwise=True)
    q = _q(gen.d, scale=3.0)
    want = np.stack([PM.normal_logpdf(4.0, q[:, 0], 1.0), PM.normal_logpdf(5.0, q[:, 0], 1.0)], axis=1)
    np.testing.assert_allclose(PC.terms(gen, q), want, rtol=1e-12, atol=0)
    gen = cg.generate(PM.long_ir(), pointwise=True)
    q = _q(gen.d)
    want = PM.normal_logpdf(PM.LONG_Y, q[:, 0:1], np.exp(PM.clamp200(q[:, 1:2])))
    np.testing.assert_allclose(PC.terms(gen, q), want, rtol=1e-12, atol=0)


def test_bernoulli_poisson_student_t_terms_equal_the_numpy_statements():
    gen = cg.generate(PM.counts_ir(), pointwise=True)
    assert gen.var_names == ["df", "p", "rate", "scale"]
    assert gen.datum_names == [("b", i) for i in range(4)] + [("cnt", i) for i in range(5)] + [("t", i) for i in range(3)]
    q = _q(gen.d)
    np.testing.assert_allclose(PC.terms(gen, q), PM.counts_numpy(q), rtol=1e-12, atol=0)


def test_datums_of_a_sum_obs_fold_left_to_right_to_its_logp_term():
    full, rest = cg.generate(PM.two_obs_ir(True), pointwise=True), cg.generate(PM.two_obs_ir(False))
    idx = [k for k, nm in enumerate(full.datum_names) if nm[0] == "y_a"]
    assert len(idx) == 7
    for q in _q(full.d):
        t = PC.terms(full, q)
        acc = t[idx[0]]
        for k in idx[1:]:
            acc = acc + t[k]
        want = gen_checker.logp_grad(full, q)[0] - gen_checker.logp_grad(rest, q)[0]
        assert abs(acc - want) <= 1e-11 * abs(want), (acc, want)


def test_results_do_not_depend_on_the_group_size():
    ir = gen_models.survival_ir()
    small, large = cg.generate(ir, pointwise=True, _pw_group=3), cg.generate(ir, pointwise=True, _pw_group=1000)
    assert small.digest != large.digest and small.datum_names == large.datum_names
    assert small.header.count("EXMC_GEN_PW_FN void") > 5 and large.header.count("EXMC_GEN_PW_FN void") == 1
    q = _q(small.d)
    assert _same_bits(PC.terms(small, q), PC.terms(large, q))
    # a range is the matching columns, whatever groups it cuts
    assert _same_bits(PC.terms(small, q, 4, 11), PC.terms(large, q)[:, 4:11])


def test_lane_layout_only_model_agrees_with_its_one_lane_sibling_statement():
    big, sib = cg.generate(PM.walk_ir(22), pointwise=True), cg.generate(PM.walk_ir(6), pointwise=True)
    assert big.d == 24 and "EXMC_GEN_ONE_LANE" not in big.header and big.lanes > 1
    assert sib.d == 8 and "EXMC_GEN_ONE_LANE" in sib.header
    assert big.datum_names == [("y", i) for i in range(22)]
    for gen, steps in ((big, 22), (sib, 6)):
        q = _q(gen.d)
        np.testing.assert_allclose(PC.terms(gen, q), PM.walk_numpy(q, steps), rtol=1e-12, atol=0)
    # the section ships the data its terms read: after the lane layout's table
    off = int(re.search(r"#define EXMC_GEN_PW_DOFF (\d+)", big.header).group(1))
    n = int(re.search(r"#define EXMC_GEN_PW_NDATA (\d+)", big.header).group(1))
    assert off > 0 and off + n == big.data.size
    assert "#define EXMC_GEN_PW_NDATA 0 " in sib.header


# ---- spec, front door, ABI --------------------------------------------------------------------------
def test_spec_and_json_front_door_carry_the_names(tmp_path):
    gen = cg.generate(cg.simple_ir([1.0, 2.0]), pointwise=True)
    spec = cg.GeneratedSpec(gen, "unused.so")
    assert spec.datum_names == [("y_obs", 0), ("y_obs", 1)] and spec.n_datums == 2
    assert cg.GeneratedSpec(cg.generate(cg.simple_ir()), "unused.so").datum_names is None
    doc = dict(pointwise=True, nodes={
        "mu": dict(op="rv", dist="normal", params=dict(mu=0.0, sigma=5.0)),
        "x": dict(op="rv", dist="normal", params=dict(mu="mu", sigma=1.0)),
        "x_obs": dict(op="obs", target="x", value=[2.1, 1.8]),
        "z": dict(op="rv", dist="normal", params=dict(mu="mu", sigma=2.0)),
        "z_obs": dict(op="obs", target="z", value=0.5)})
    (tmp_path / "m.json").write_text(json.dumps(doc))
    cg.main([str(tmp_path / "m.json"), str(tmp_path / "out"), "--no-build"])
    meta = json.load(open(tmp_path / "out" / "model.json"))
    assert meta["datum_names"] == [["x_obs", 0], ["x_obs", 1], "z_obs"] and meta["n_datums"] == 3
    assert "#define EXMC_GEN_POINTWISE 1" in open(tmp_path / "out" / "exmc_gen_model.h").read()
    doc.pop("pointwise")
    (tmp_path / "m.json").write_text(json.dumps(doc))
    cg.main([str(tmp_path / "m.json"), str(tmp_path / "out2"), "--no-build"])
    assert "datum_names" not in json.load(open(tmp_path / "out2" / "model.json"))


def _declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(exmc_hip_\w+)\s*\(", txt)))


def test_pointwise_header_is_plain_c_and_its_export_list_equals_it(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "exmc_hip_compare.h"\n'
                   "int main(void){int (*f)(exmc_hip_model*, const double*, int, int, int, int, int, double*) = "
                   "exmc_hip_pointwise_loglik_range; return f != 0;}\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INCLUDE, "-c", str(src),
                           "-o", str(tmp_path / "t.o")])
    assert sorted(_lib.POINTWISE_EXPORTS) == _declared(os.path.join(INCLUDE, "exmc_hip_pointwise.h"))
    others = set(_lib.EXPORTS) | set(_lib.COMPARE_EXPORTS) | set(_lib.PSIS_EXPORTS)
    assert not set(_lib.POINTWISE_EXPORTS) & others


def test_python_psis_default_scratch_is_the_headers():
    from exmc_amd import model_comparison as MC
    txt = open(os.path.join(INCLUDE, "exmc_hip_psis.h")).read()
    m = re.search(r"#define EXMC_PSIS_DEFAULT_SCRATCH \((\d+)ull << (\d+)\)", txt)
    assert m and MC.PSIS_DEFAULT_SCRATCH == int(m.group(1)) << int(m.group(2))
    assert MC.CUSTOM is cg.CUSTOM


def test_every_position_entry_is_read_once_per_function():
    gen = cg.generate(PM.long_ir(), pointwise=True)
    body = gen.header.split("EXMC_GEN_PW_FN void exmc_gen_pw_1(")[1].split("\n}\n")[0]
    assert body.count("EXMC_GEN_PW_Q(0)") == 1 and body.count("EXMC_GEN_PW_Q(1)") == 1
