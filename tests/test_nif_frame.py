"""The frame the per-call NIF modules share (c_src/exmc_nif_util.h: the model tuple, the per-call handle, the
int32 list, the raising body, the device), without a GPU: every module's decode failures are badargs raised
before any library call (the per-call counterpart of test_nif_shim.py::test_decode_failures_are_badarg), and
tests/host/nif_frame_driver.c drives the helpers themselves under ASan + UBSan as a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import nif_harness as H
from test_beam_boundary_sources import ROWS, rows

HOST = os.path.join(H.ROOT, "tests", "host")


@pytest.fixture(scope="module")
def outdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("nifframe"))


@rows
def test_decode_failures_are_badarg(row, outdir):
    mod = H.load_shim(outdir, row.c)
    (fn, arity), = row.funcs.items()
    assert mod.name == "Elixir.Exmc.NUTS." + row.module and len(row.args) + 1 == arity
    kind, data = 2, np.zeros(16)
    refused = {"a list": [kind, data], "a 3-tuple": H.tuple_term(mod, kind, data, 1),
               "12 bytes of data": H.tuple_term(mod, kind, bytes(12))}
    calls = [(why, [model] + row.args) for why, model in refused.items()]
    good = [H.tuple_term(mod, kind, data)] + row.args
    calls.append(("a zero count", good[:row.count] + [0] + good[row.count + 1:]))
    if isinstance(row.args[0], list):                     # Pathfinder, ADVI: perm
        calls.append(("an atom for perm", good[:1] + [H.Atom("none")] + good[2:]))
    for why, args in calls:
        with pytest.raises(H.BadArg):
            mod.call(fn, *args)
            pytest.fail("%s/%d took %s" % (fn, arity, why))


def test_pathfinder_and_advi_are_the_rows_with_a_perm():
    assert [r.module for r in ROWS if isinstance(r.args[0], list)] == ["HipPathfinderNative", "HipAdviNative"]


def test_frame_driver_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "nif_frame_driver")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread",
                           "-o", exe] + [os.path.join(HOST, f) for f in
                                         ("nif_frame_driver.c", "fake_erl_nif.c", "stub_exmc_hip.c")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "nif_frame_driver: ok" in r.stdout, out[-3000:]
    assert "Sanitizer" not in out and "runtime error:" not in out, out[-3000:]
