"""The BEAM side of LOO-PIT as source files: the NIF table of c_src/exmc_hip_loo_pit_nif.c names what the
Elixir stub names, the wrapper calls the stub with its arity, and the shim compiles against the declaration
header. (tests/test_gpu_loo_pit_nif.py calls it on the device.)"""
import os
import re
import subprocess

import pytest

import test_elixir_sources as ES

C_SRC = os.path.join(ES.ROOT, "c_src", "exmc_hip_loo_pit_nif.c")


def test_nif_table_equals_the_elixir_stub():
    c = open(C_SRC).read()
    rows = re.findall(r'\{"(\w+)", (\d+), (\w+), (\w+)\}', c[c.index("static ErlNifFunc nif_funcs[]"):])
    assert rows == [("loo_pit", "6", "loo_pit", "ERL_NIF_DIRTY_JOB_IO_BOUND")]
    assert "ERL_NIF_INIT(Elixir.Exmc.NUTS.HipLooPitNative," in c
    ex = ES._read(ES.EX, "lib", "exmc", "nuts", "hip_loo_pit_native.ex")
    assert "defmodule Exmc.NUTS.HipLooPitNative do" in ex and "@on_load :load_nif" in ex
    assert ":erlang.load_nif" in ex and "exmc_hip_loo_pit_nif" in ex
    stubs = {m.group(1): len(ES._split_args(m.group(2))) for m in re.finditer(
        r"def\s+([a-z_]+)\(([^)]*)\)\s*,?\s*do:\s*:erlang\.nif_error\(:nif_not_loaded\)", ES._strip(ex))}
    assert stubs == {"loo_pit": 6}


def test_wrapper_calls_the_stub_with_its_arity():
    src = ES._strip(ES._read(ES.EX, "lib", "exmc", "nuts", "hip_loo_pit.ex"))
    m = re.search(r"HipLooPitNative\.loo_pit\(", src)
    i, depth = m.end(), 1
    while depth:
        depth += {"(": 1, ")": -1}.get(src[i], 0)
        i += 1
    assert len(ES._split_args(src[m.end():i - 1])) == 6
    assert "def loo_pit(" in src
    # the datum keys are HipPredictive's, stated there once
    assert "HipPredictive.datum_names(" in src
    pred = ES._strip(ES._read(ES.EX, "lib", "exmc", "nuts", "hip_predictive.ex"))
    assert len(re.findall(r"\bdef datum_names\(", pred)) == 5 and "defp datum_names(" not in pred


@pytest.mark.parametrize("name", ["hip_loo_pit_native.ex", "hip_loo_pit.ex", "hip_predictive.ex"])
def test_blocks_balance(name):
    src = ES._strip(ES._read(ES.EX, "lib", "exmc", "nuts", name))
    opens = len(re.findall(r"\bdo\b(?!:)", src)) + len(re.findall(r"\bfn\b", src))
    assert opens == len(re.findall(r"\bend\b", src)), name
    for a, b in ("()", "[]", "{}"):
        assert src.count(a) == src.count(b), (name, a)
    assert src.lstrip().startswith("defmodule Exmc.NUTS.")


def test_shim_compiles_against_the_declaration_header(tmp_path):
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-fPIC", "-c", "-o",
                           str(tmp_path / "nif.o"), C_SRC])
    assert "exmc_hip_loo_pit_nif" in open(os.path.join(ES.ROOT, "INTEGRATION.md")).read()
