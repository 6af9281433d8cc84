"""The generator's output is pinned: for every case of tools/gen_digests.py (the test models in every
layout, the three baseline models over lanes x waves per SIMD x scan, walks around MIN_SCAN and the
ones whose chain is dropped and tried again, wide table rows on both sides of PAIR_MIN_COLS and of
the workgroup form, random hierarchical models, exported term orders, the per-datum section, one small
model per branch of the term walk and per refusal -- a refusal is pinned by its message) the digest of
the header, the sha256 of the data table and the line count equal tests/golden/generated_digests.json.
Identical text means identical plug-in binaries and identical plug-in cache tags, so a restructuring
of codegen*.py is proved to change nothing on the CPU, in seconds.

A change that alters the text on purpose regenerates the file in its own commit:

    python tools/gen_digests.py --write tests/golden/generated_digests.json
"""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("gen_digests", os.path.join(ROOT, "tools", "gen_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generated_text_and_tables_are_what_was_committed():
    with open(os.path.join(ROOT, "tests", "golden", "generated_digests.json")) as fh:
        pinned = json.load(fh)
    now = _tool().digests()
    assert sorted(now) == sorted(pinned)                   # no case dropped, none added without its digest
    assert len(now) >= 250
    differ = {k: (pinned[k], now[k]) for k in pinned if now[k] != pinned[k]}
    assert not differ, "%d of %d cases differ, the first: %r" % (len(differ), len(pinned), sorted(differ.items())[0])


def test_the_corpus_reaches_the_branches_it_is_there_for():
    from exmc_amd import codegen as cg, codegen_lanes as cl
    cases = dict(_tool().cases())
    import gen_models as GM

    def gen(name):
        return cases[name]()
    assert len(gen("scan/walk/m=%d" % cl.MIN_SCAN).scan_chains) == 1
    assert gen("scan/walk/m=%d" % (cl.MIN_SCAN - 1)).scan_chains == []
    # a chain the uniform part reads is dropped and the rest tried again: fewer scans than qualify
    retry = gen("scan/branch_retry")
    assert [c["first"] for c in retry.scan_chains] == ["w0_21"]
    assert "EXMC_GEN_LT2(" in gen("wide/n=64/k=%d/wps=2" % cl.PAIR_MIN_COLS).header
    assert "EXMC_GEN_LT2(" not in gen("wide/n=64/k=%d/wps=2" % (cl.PAIR_MIN_COLS - 1)).header
    assert "#define EXMC_GEN_WG 1" in gen("wg/n=500/k=20").header
    assert "#define EXMC_GEN_WG 0" in gen("wg/n=48/k=20").header
    assert sum(1 for k in cases if k.startswith("random/")) >= 20
    assert len(cases) == len(_tool().cases())              # names are unique
    assert gen("term_order/sorted").digest != gen("term_order/reversed").digest and cg.MAX_NODES_SORTED < 40

    def refused(name):
        try:
            gen(name)
        except cg.CodegenError as e:
            return str(e)
        return None
    # pointwise: a one-lane model, one with the lane layout only (the section ships its data), every kind of
    # obs node, group sizes, the two refusals
    pw = gen("pointwise/simple")
    assert "#define EXMC_GEN_POINTWISE 1" in pw.header and "#define EXMC_GEN_PW_DOFF 0 " in pw.header and pw.n_datums == 10
    big = gen("pointwise/walk24_lanes")
    assert "EXMC_GEN_ONE_LANE" not in big.header and "#define EXMC_GEN_PW_DOFF 0 " not in big.header and big.n_datums == 22
    meta = gen("pointwise/meta")
    assert meta.n_datums == 15 and "c_mean" in meta.datum_names and "j_masked_scalar" not in meta.datum_names
    assert ("b_mask", 1) not in meta.datum_names and ("b_mask", 2) in meta.datum_names
    assert gen("corner/meta/scalar_mask_true/pointwise").datum_names == ["o"]
    assert gen("pointwise/counts/group=1").header.count("EXMC_GEN_PW_FN void") == 12
    assert gen("pointwise/long").n_datums == 37 and gen("pointwise/long").header.count("EXMC_GEN_PW_FN void") == 3
    assert "no datum" in refused("pointwise/no_datum") and "at least one datum" in refused("pointwise/counts/group=0")
    assert "#define EXMC_GEN_PW_NCONST 1\n" in gen("pointwise/literal_custom").header     # nothing to fold
    # rewrite passes: default transforms on a free and on an observed rv, both lifts, their refusal
    assert gen("corner/rewrite/poisson").transforms == {"mu": "log"} and gen("corner/rewrite/poisson").digest != \
        cg.generate(GM.poisson_ir()).digest
    assert gen("corner/rewrite/lifted").var_names == ["m"] and "det node" in refused("corner/rewrite/lifted_censored")
    assert gen("corner/rewrite/default_transforms").transforms == {"mix": "log"}
    assert gen("corner/rewrite/weibull_censored").digest == gen("corner/rewrite/weibull").digest    # dropped silently
    # "__obs_data": rank 0, 1, 2 and none
    assert [gen("corner/data/%s" % k).data.size for k in ("scalar", "vector", "matrix")] == [1, 5, 4]
    assert "has no data" in refused("corner/data/missing")
    # observation of a transformed target
    for tr in ("log", "softplus", "logit"):
        assert gen("corner/obs_tr/%s" % tr).n_ops < gen("corner/obs_tr/%s/vector" % tr).n_ops
    assert "'cube'-transformed" in refused("corner/obs_tr/uncovered")
    assert "softplus-transformed target of a computed value" in refused("corner/meas/transformed/softplus")
    # observation metadata
    assert gen("corner/meta/scalar_weight").digest != gen("corner/meta/scalar_mask_true").digest
    assert gen("corner/meta/scalar_mask_false").digest != gen("corner/meta/scalar_mask_true").digest
    assert "vector weight on a scalar term" in refused("corner/meta/vector_weight_on_scalar_term")
    assert "vector mask on a scalar term" in refused("corner/meta/vector_mask_on_scalar_term")
    assert "mask does not match" in refused("corner/meta/mask_length") and "needs a reduce" in refused("corner/meta/no_reduce")
    assert gen("corner/meta/likelihood_false").var_names == ["m"]
    # meas_obs
    assert gen("corner/meas/affine/vector_a").digest != gen("corner/meas/affine/vector_b").digest
    assert gen("corner/meas/matmul").d == gen("corner/meas/transformed/scalar").d + 1 == gen("corner/meas/transformed/logit").d == 2
    assert "target not covered" in refused("corner/meas/vector_target") and "eagerly" in refused("corner/meas/ref_param")
    # obs
    assert "does not target an rv" in refused("corner/obs/det_target")
    assert "this distribution / censoring" in refused("corner/obs_tr/interval")
    assert gen("corner/obs/censored/scalar").d == gen("corner/obs/censored/vector").d == 2
    assert "vector params are not covered" in refused("corner/obs/censored/vector_param")
    assert gen("corner/obs/vector_dist/plain").digest != gen("corner/rewrite/dirichlet_obs").digest
    assert "transform 'log' on a vector distribution" in refused("corner/obs/vector_dist/transform")
    assert "plain vector value" in refused("corner/obs/vector_dist/scalar_value")
    assert gen("corner/obs/mixture_scalar").n_ops < gen("corner/obs/mixture_vector").n_ops and "lengths differ" in refused("corner/obs/vector_lengths")
    # free rvs
    assert "#define EXMC_GEN_NDATA 0\n" in gen("corner/free/custom").header
    assert "callable" in refused("corner/free/custom/not_callable") and "return a scalar" in refused("corner/free/custom/list")
    assert "has a vector param" in refused("corner/free/vector_param")
    assert "transformed vector rv" in refused("corner/free/transformed_vector")
    # the whole model
    assert "unknown node" in refused("corner/model/unknown_target") and "no free" in refused("corner/model/all_observed")
    assert "at most %d" % cg.MAX_D_LANES in refused("corner/model/too_many_dimensions")
    assert "16, 32 or 64" in refused("corner/model/lanes=8")
    assert (gen("corner/model/d=25/lanes=auto").lanes, gen("corner/model/d=40/lanes=auto").lanes) == (16, 64)
    assert "does not match the node map" in refused("corner/model/term_order/keys")
    assert "must be the sorted ids" in refused("corner/model/term_order/unsorted")
    assert "does not depend on the free variables" in refused("corner/model/constant_density")
    assert "not a free random variable" in refused("corner/model/ref_to_observed")
    assert "cyclic" in refused("corner/model/cyclic_ncp") and gen("corner/model/cyclic_ncp/ncp=0").d == 3
