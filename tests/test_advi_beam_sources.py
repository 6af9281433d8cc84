"""The BEAM side of ADVI as source files, checked without a BEAM in the style of
test_elixir_sources.py: the ErlNifFunc table of c_src/exmc_hip_advi_nif.c (module name, arity,
dirty flag) against the stub of elixir/.../hip_advi_native.ex, the call in hip_advi.ex
against that arity, balanced blocks, and the shim compiling against the declaration header."""
import os
import re
import subprocess

import pytest

import test_elixir_sources as ES

ROOT = ES.ROOT
C_SRC = os.path.join(ROOT, "c_src", "exmc_hip_advi_nif.c")


def _table():
    c = open(C_SRC).read()
    return c, re.findall(r'\{"(\w+)", (\d+), (\w+), (\w+)\}', c[c.index("static ErlNifFunc nif_funcs[]"):])


def test_nif_table_equals_the_elixir_stub():
    c, rows = _table()
    assert rows == [("fit", "12", "fit", "ERL_NIF_DIRTY_JOB_IO_BOUND")]
    assert "ERL_NIF_INIT(Elixir.Exmc.NUTS.HipAdviNative," in c
    ex = ES._read(ES.EX, "lib", "exmc", "nuts", "hip_advi_native.ex")
    assert "defmodule Exmc.NUTS.HipAdviNative do" in ex and "@on_load :load_nif" in ex
    assert ":erlang.load_nif" in ex and "exmc_hip_advi_nif" in ex
    stubs = {m.group(1): len(ES._split_args(m.group(2))) for m in re.finditer(
        r"def\s+([a-z_]+)\(([^)]*)\)\s*,?\s*do:\s*:erlang\.nif_error\(:nif_not_loaded\)", ES._strip(ex))}
    assert stubs == {"fit": 12}


def test_fit_calls_the_stub_with_its_arity_and_builds_the_reference_shape():
    src = ES._strip(ES._read(ES.EX, "lib", "exmc", "nuts", "hip_advi.ex"))
    m = re.search(r"HipAdviNative\.fit\(", src)
    i, depth = m.end(), 1
    while depth:
        depth += {"(": 1, ")": -1}.get(src[i], 0)
        i += 1
    assert len(ES._split_args(src[m.end():i - 1])) == 12
    assert "def fit(" in src and "Transform.apply(entry.transform" in src and "pm.entries" in src
    for key in ("elbo_history:", "mu:", "log_sigma:", "converged:", "num_iters:"):
        assert key in src, key


@pytest.mark.parametrize("name", ["hip_advi_native.ex", "hip_advi.ex"])
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
    assert "exmc_hip_advi_nif" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
