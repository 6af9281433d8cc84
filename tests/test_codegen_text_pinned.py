"""The generator's output is pinned: for every case of tools/gen_digests.py (the test models in every
layout, the three baseline models over lanes x waves per SIMD x scan, walks around MIN_SCAN and the
ones whose chain is dropped and tried again, wide table rows on both sides of PAIR_MIN_COLS and of
the workgroup form, random hierarchical models, exported term orders) the digest of the header, the
sha256 of the data table and the line count equal tests/golden/generated_digests.json. Identical
text means identical plug-in binaries and identical plug-in cache tags, so a restructuring of
codegen*.py is proved to change nothing on the CPU, in seconds.

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
    assert len(now) >= 150
    differ = {k: (pinned[k], now[k]) for k in pinned if now[k] != pinned[k]}
    assert not differ, "%d of %d cases differ, the first: %r" % (len(differ), len(pinned), sorted(differ.items())[0])


def test_the_corpus_reaches_the_branches_it_is_there_for():
    from exmc_amd import codegen as cg, codegen_lanes as cl
    cases = dict(_tool().cases())

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
