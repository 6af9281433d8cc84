"""CPU guard of the handle-state matrix (tests/test_gpu_handle_state.py): every entry point of
include/exmc_hip.h that takes a model handle is called by an op of the catalogue or exempt with a
reason, so that a new entry point cannot escape the pair and continuation rules."""
import os
import re

import test_gpu_handle_state as HS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "exmc_hip.h")


def handle_functions(path):
    """names of the exmc_hip_* functions declared in `path` with an exmc_hip_model* parameter"""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    decls = re.findall(r"\b(exmc_hip_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    return {name for name, params in decls if re.search(r"\bexmc_hip_model\s*\*", params)}


def uncovered(path):
    covered = {f for fns in HS.ENTRY_POINTS.values() for f in fns}
    return sorted(handle_functions(path) - covered - set(HS.EXEMPT))


def test_every_handle_entry_point_is_in_the_matrix():
    found = handle_functions(HEADER)
    assert {"exmc_hip_chains_advance", "exmc_hip_stream_next_host", "exmc_hip_model_dim"} <= found
    assert not uncovered(HEADER), "add these to the catalogue of test_gpu_handle_state.py or to EXEMPT"
    assert set(HS.ENTRY_POINTS) == set(HS.OPS)
    # the catalogue and the exemptions name declared entry points only, each once
    covered = {f for fns in HS.ENTRY_POINTS.values() for f in fns}
    assert covered <= found and set(HS.EXEMPT) <= found
    assert not covered & set(HS.EXEMPT)
    assert all(reason.strip() for reason in HS.EXEMPT.values())


def test_guard_sees_a_new_entry_point(tmp_path):
    hdr = tmp_path / "exmc_hip.h"
    src = open(HEADER).read()
    i = src.rindex("#ifdef __cplusplus")
    hdr.write_text(src[:i] + "int exmc_hip_model_new_thing(exmc_hip_model* m, int k);\n"
                   "int exmc_hip_device_only_thing(int device, int k);\n" + src[i:])
    assert uncovered(str(hdr)) == ["exmc_hip_model_new_thing"]
