"""The BEAM side of every per-call NIF module as source files, checked without a BEAM in the style of
test_elixir_sources.py (which holds HipNative to the same): ONE table, a row per module, and every row
held to the same checks -- the ErlNifFunc table and ERL_NIF_INIT line of the C file against the Elixir
stub, the wrapper's call against the stub's arity, balanced blocks, the shim compiling against the
declaration header, its mention in INTEGRATION.md. (tests/test_gpu_*_nif.py call the modules on the device,
tests/test_nif_frame.py holds their shared decode to badarg without one.)"""
import collections
import os
import re
import subprocess

import pytest

import test_elixir_sources as ES

# c: the file under c_src/; module: Exmc.NUTS.<module>; funcs: {function: arity}; stub, wrapper: files under
# elixir/lib/exmc/nuts/; call: the wrapper's call of the stub; texts: what else the wrapper's code must hold (the
# public function, and the feature's own: the reference's result keys, the transform back to the constrained
# space); args: a call's arguments after the model tuple that decode, count: the index of the chain / fit /
# path count among ALL arguments (tests/test_nif_frame.py makes the refused calls from these)
Row = collections.namedtuple("Row", "c module funcs stub wrapper call texts args count")
TRACE = bytes(8 * 2 * 3 * 10)
ROWS = [
    Row("exmc_hip_compare_nif.c", "HipCompareNative", {"ic_stats": 4}, "hip_compare_native.ex", "hip_sampler.ex",
        "HipCompareNative.ic_stats(", ("HipCompareNative.ic_stats(model, draws,",), [TRACE, 2, 3], 2),
    Row("exmc_hip_psis_nif.c", "HipPsisNative", {"psis_stats": 4}, "hip_psis_native.ex", "hip_sampler.ex",
        "HipPsisNative.psis_stats(", ("Exmc.NUTS.HipPsisNative.psis_stats(model, draws,", "def psis_loo("),
        [TRACE, 2, 3], 2),
    Row("exmc_hip_pathfinder_nif.c", "HipPathfinderNative", {"fit": 9}, "hip_pathfinder_native.ex", "hip_pathfinder.ex",
        "HipPathfinderNative.fit(",
        ("def fit(", "Transform.apply(entry.transform", "pm.entries", "elbo:", "mu:", "sigma:", "num_iters:"),
        [[], 2, 0, 3, 7, 4, 19, 0], 2),
    Row("exmc_hip_advi_nif.c", "HipAdviNative", {"fit": 12}, "hip_advi_native.ex", "hip_advi.ex", "HipAdviNative.fit(",
        ("def fit(", "Transform.apply(entry.transform", "pm.entries", "elbo_history:", "mu:", "log_sigma:", "converged:",
         "num_iters:"),
        [[], 2, 0, 3, 7, 1, 4, 0.01, 1e-4, 19, 0], 2),
    Row("exmc_hip_predictive_nif.c", "HipPredictiveNative", {"posterior_predictive": 6}, "hip_predictive_native.ex",
        "hip_predictive.ex", "HipPredictiveNative.posterior_predictive(", ("def posterior_predictive(",),
        [TRACE, 2, 3, 19, 0], 2),
    Row("exmc_hip_ppc_nif.c", "HipPpcNative", {"ppc": 6}, "hip_ppc_native.ex", "hip_ppc.ex", "HipPpcNative.ppc(",
        ("def ppc(",), [TRACE, 2, 3, 19, 0], 2),
    Row("exmc_hip_loo_pit_nif.c", "HipLooPitNative", {"loo_pit": 6}, "hip_loo_pit_native.ex", "hip_loo_pit.ex",
        "HipLooPitNative.loo_pit(", ("def loo_pit(", "HipPredictive.datum_names("), [TRACE, 2, 3, 19, 0], 2),
    Row("exmc_hip_prior_nif.c", "HipPriorNative", {"prior_samples": 6}, "hip_prior_native.ex", "hip_prior.ex",
        "HipPriorNative.prior_samples(", ("def prior_samples(",), [2, 3, 19, 0, 1], 1),
]
rows = pytest.mark.parametrize("row", ROWS, ids=[r.module for r in ROWS])


def _ex(name):
    return ES._read(ES.EX, "lib", "exmc", "nuts", name)


@rows
def test_nif_table_equals_the_elixir_stub(row):
    (fn, arity), = row.funcs.items()
    c = ES._read(ES.ROOT, "c_src", row.c)
    table = re.findall(r'\{"(\w+)", (\d+), (\w+), (\w+)\}', c[c.index("static ErlNifFunc nif_funcs[]"):])
    assert table == [(fn, str(arity), fn, "ERL_NIF_DIRTY_JOB_IO_BOUND")]
    assert "ERL_NIF_INIT(Elixir.Exmc.NUTS.%s," % row.module in c
    ex = _ex(row.stub)
    assert "defmodule Exmc.NUTS.%s do" % row.module in ex and "@on_load :load_nif" in ex
    assert ":erlang.load_nif" in ex and os.path.splitext(row.c)[0] in ex
    stubs = {m.group(1): len(ES._split_args(m.group(2))) for m in re.finditer(
        r"def\s+([a-z_]+)\(([^)]*)\)\s*,?\s*do:\s*:erlang\.nif_error\(:nif_not_loaded\)", ES._strip(ex))}
    assert stubs == row.funcs


@rows
def test_wrapper_calls_the_stub_with_its_arity(row):
    (fn, arity), = row.funcs.items()
    assert row.call == "%s.%s(" % (row.module, fn)
    src = ES._strip(_ex(row.wrapper))
    i, depth = src.index(row.call) + len(row.call), 1
    start = i
    while depth:
        depth += {"(": 1, ")": -1}.get(src[i], 0)
        i += 1
    assert len(ES._split_args(src[start:i - 1])) == arity
    for text in row.texts:
        assert text in src, text


@rows
def test_blocks_balance(row):
    for name in (row.stub, row.wrapper):
        src = ES._strip(_ex(name))
        opens = len(re.findall(r"\bdo\b(?!:)", src)) + len(re.findall(r"\bfn\b", src))
        assert opens == len(re.findall(r"\bend\b", src)), name
        for a, b in ("()", "[]", "{}"):
            assert src.count(a) == src.count(b), (name, a)
        assert src.lstrip().startswith("defmodule Exmc.NUTS.")


@rows
def test_shim_compiles_against_the_declaration_header(row, tmp_path):
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-fPIC", "-c", "-o",
                           str(tmp_path / "nif.o"), os.path.join(ES.ROOT, "c_src", row.c)])
    assert os.path.splitext(row.c)[0] in ES._read(ES.ROOT, "INTEGRATION.md")


def test_the_table_is_every_per_call_module():
    """every NIF module of c_src/ but the two that hold resources (test_elixir_sources.py, test_nif_shim.py)"""
    have = {f for f in os.listdir(os.path.join(ES.ROOT, "c_src")) if f.endswith("_nif.c")}
    assert have - {"exmc_hip_nif.c", "exmc_native_tree_nif.c"} == {r.c for r in ROWS}


def test_loo_pit_takes_its_datum_keys_from_hip_predictive():
    """the datum keys are HipPredictive's, stated there once (one public clause per kind with datums)"""
    pred = ES._strip(_ex("hip_predictive.ex"))
    assert len(re.findall(r"\bdef datum_names\(", pred)) == 5 and "defp datum_names(" not in pred
