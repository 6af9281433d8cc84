#!/usr/bin/env python3
"""Digests of the generator's output over a fixed corpus of models: one line per case with the case
name, Generated.digest (sha256 of the header, 16 hex digits), the sha256 of Generated.data.tobytes()
and the header's line count. A case the generator refuses prints the error message in place of the
digests. Runs on the CPU in seconds.

    python tools/gen_digests.py                 # print
    python tools/gen_digests.py --write tests/golden/generated_digests.json

tests/test_codegen_text_pinned.py compares the committed file with what the code gives now: a
restructuring of the generator leaves every line as it is, a change that alters the text on purpose
regenerates the file in its own commit."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np   # noqa: E402

from exmc_amd import codegen as cg, codegen_lanes as cl, models   # noqa: E402

N_RANDOM = 24


def cases():
    """[(name, thunk -> Generated)] in a fixed order. The models are those of the tests (imported from
    there, so the corpus follows them)."""
    import chain_models as CM
    import gen_models as GM
    from test_codegen_lanes import _random_big_ir
    from test_codegen_term_order import _ir as term_order_ir
    out = []

    def add(name, ir_fn, **kw):
        out.append((name, lambda: cg.generate(ir_fn(), **kw)))
    small = dict(simple=cg.simple_ir, eight_schools=cg.eight_schools_ir, zoo=GM.zoo_ir, walk=GM.walk_ir,
                 simplex=GM.simplex_ir, survival=GM.survival_ir)
    for name, fn in small.items():
        for ncp in (True, False):
            for lanes in (None, 16, 64):
                add("test/%s/ncp=%d/lanes=%s" % (name, ncp, lanes), fn, ncp=ncp, lanes=lanes)
    for which in ("sv", "logistic", "radon"):
        for lanes in (16, 32, 64):
            for wps in (1, 2):
                for scan in (True, False):
                    add("baseline/%s/lanes=%d/wps=%d/scan=%d" % (which, lanes, wps, scan),
                        lambda w=which: GM.baseline_pair(w)[0], ncp=GM.baseline_pair(which)[1], lanes=lanes,
                        waves_per_simd=wps, scan=scan)
    add("scan/sv_ncp", lambda: cg.sv_ir(GM.sv_returns()), ncp=True, lanes=64)
    add("scan/sv_ncp/wps=2", lambda: cg.sv_ir(GM.sv_returns()), ncp=True, lanes=64, waves_per_simd=2)
    # walks: around MIN_SCAN, around the slot boundaries, several chains, heads of every kind, and the two
    # models whose uniform part reads a walk value (the chain is dropped and the others tried again)
    for m in (cl.MIN_SCAN - 1, cl.MIN_SCAN, cl.MIN_SCAN + 1, 63, 64, 65, 129, 254):
        add("scan/walk/m=%d" % m, lambda m=m: CM.chain_ir([m], seed=m), lanes=64)
    add("scan/walk/m=40/scan=0", lambda: CM.chain_ir([40], seed=6), lanes=64, scan=False)
    add("scan/walk/m=40/lanes=16", lambda: CM.chain_ir([40], seed=6), lanes=16)
    add("scan/walk/m=40/lanes=32", lambda: CM.chain_ir([40], seed=6), lanes=32)
    add("scan/walk/m=40/ncp=0", lambda: CM.chain_ir([40], seed=6), lanes=64, ncp=False)
    add("scan/two_walks", lambda: CM.chain_ir([40, 70], seed=2), lanes=64)
    add("scan/two_walks/wps=2", lambda: CM.chain_ir([40, 70], seed=2), lanes=64, waves_per_simd=2)
    for head in ("log", "ncp"):
        add("scan/head=%s" % head, lambda h=head: CM.chain_ir([50], seed=3, head=h), lanes=64)
    add("scan/branch_retry", lambda: CM.chain_ir([60], seed=4, branch=20), lanes=64)
    add("scan/sigma_split_retry", lambda: CM.chain_ir([60], seed=5, sigma_split=30), lanes=64)
    # wide table rows: both sides of PAIR_MIN_COLS, and both answers to the workgroup form
    for n_obs, k in ((500, 20), (333, 12), (100, 9), (64, 8), (64, 7), (48, 20)):
        for wps in (1, 2):
            add("wide/n=%d/k=%d/wps=%d" % (n_obs, k, wps),
                lambda n=n_obs, k=k: cg.logistic_ir(*models.logistic_data(seed=11 + n + k, n=n, k=k)),
                ncp=True, lanes=16, waves_per_simd=wps)
    for n_obs, k in ((500, 20), (333, 24), (48, 20)):
        add("wg/n=%d/k=%d" % (n_obs, k),
            lambda n=n_obs, k=k: cg.logistic_ir(*models.logistic_data(seed=300 + n + k, n=n, k=k)),
            ncp=True, lanes=16, waves_per_simd=2)
    add("wide/n=333/k=24/lanes=32", lambda: cg.logistic_ir(*models.logistic_data(seed=657, n=333, k=24)),
        ncp=True, lanes=32, waves_per_simd=2)
    for seed in range(N_RANDOM):
        for lanes in sorted({(16, 32, 64)[seed % 3], 64 if seed % 3 != 2 else 16}):
            add("random/seed=%d/lanes=%d" % (seed, lanes), lambda s=seed: _random_big_ir(s)[0], lanes=lanes)
    ids = sorted(term_order_ir()[0].nodes)
    add("term_order/sorted", lambda: term_order_ir()[0], ncp=False)
    add("term_order/reversed", lambda: term_order_ir()[0].order(list(reversed(ids))), ncp=False)
    add("term_order/reversed/lanes=16", lambda: term_order_ir()[0].order(list(reversed(ids))), ncp=False, lanes=16)
    # the per-datum section: one-lane models, one that has the lane layout only (its section ships its own
    # data), every kind of obs node, group sizes that do and do not divide the datum count, the refusals
    import pw_models as PM
    for name, fn in (("simple", cg.simple_ir), ("eight_schools", cg.eight_schools_ir), ("walk24_lanes", lambda: PM.walk_ir(22)),
                     ("walk8", lambda: PM.walk_ir(6)), ("meta", PM.meta_ir), ("counts", PM.counts_ir), ("long", PM.long_ir),
                     ("two_obs", PM.two_obs_ir), ("survival", GM.survival_ir), ("no_datum", PM.no_datum_ir),
                     ("literal_custom", lambda: GM.literal_custom_ir(observed=True))):
        add("pointwise/%s" % name, fn, pointwise=True)
    for group in (0, 1, 3, 1000):
        add("pointwise/counts/group=%d" % group, PM.counts_ir, pointwise=True, _pw_group=group)
    add("pointwise/walk24_lanes/lanes=64", lambda: PM.walk_ir(22), pointwise=True, lanes=64)
    add("pointwise/simple/lanes=16", cg.simple_ir, pointwise=True, lanes=16)
    # one small model per remaining branch of the term walk, the refusals with their messages
    for name, fn, kw in GM.corner_cases():
        add("corner/%s" % name, fn, **kw)
    return out


def digests():
    """{case name: {"header", "data", "lines"} or {"error"}}"""
    res = {}
    for name, thunk in cases():
        try:
            gen = thunk()
        except cg.CodegenError as e:
            res[name] = {"error": str(e)}
            continue
        res[name] = {"header": gen.digest,
                     "data": hashlib.sha256(np.ascontiguousarray(gen.data, dtype=np.float64).tobytes()).hexdigest(),
                     "lines": gen.n_ops}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--write", metavar="FILE", help="write the digests as JSON instead of printing them")
    args = ap.parse_args(argv)
    res = digests()
    if args.write:
        with open(args.write, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    else:
        for name, r in res.items():
            print(name, r.get("error") or "%s %s %d" % (r["header"], r["data"], r["lines"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
