"""include/exmc_detmath.h: exmc_log_ge1 and exmc_log_unit are one main path (exmc_log_main) with a fix-up
each (exmc_log_ge1_fix, exmc_log_unit_fix), stated separately so that a kernel can evaluate the main path
once for an argument of each (exmc_nuts.hpp, the outer merge). Over each function's stated domain the
main path plus the fix-up equals the function, and the general exmc_log, bit for bit: 0, the smallest
uniform, 1, values in [1, 2], large values and NaN included. Host build of the shared header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("detmath_parts") / "libdetmath_parts.so")
    fma = ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared"]
                          + fma + ["-o", out, os.path.join(ROOT, "tests", "host", "detmath_log_parts_shim.c"), "-lm"])
    L = C.CDLL(out)
    for n in ("h_ge1_parts", "h_unit_parts", "h_log_ge1", "h_log_unit"):
        getattr(L, n).argtypes = [C.c_double]
        getattr(L, n).restype = C.c_double
    L.h_parts_compare.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_long]
    L.h_parts_compare.restype = C.c_long
    return L


def _bad(lib, which, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return lib.h_parts_compare(which, x.ctypes.data_as(C.POINTER(C.c_double)), x.size)


def _bits(v):
    return np.float64(v).view(np.uint64)


def test_log_ge1_parts(lib):
    rng = np.random.default_rng(5)
    x = np.r_[1.0 + rng.uniform(0, 1, 500_000), np.exp(rng.uniform(0, 709, 500_000)),
              [1.0, 2.0, 1.0000000000000002, 1.9999999999999998, 1e308, 1.7976931348623157e308, np.nan]]
    assert _bad(lib, 0, x) == 0
    assert lib.h_ge1_parts(1.0) == 0.0 and _bits(lib.h_ge1_parts(1.0)) == _bits(lib.h_log_ge1(1.0))
    assert np.isnan(lib.h_ge1_parts(np.nan)) and _bits(lib.h_ge1_parts(np.nan)) == _bits(lib.h_log_ge1(np.nan))


def test_log_unit_parts(lib):
    rng = np.random.default_rng(6)
    x = np.r_[np.floor(rng.uniform(0, 1, 1_000_000) * 2.0 ** 53) / 2.0 ** 53,
              [0.0, 2.0 ** -53, 2.0 ** -52, 0.5, 1 - 2.0 ** -53]]
    assert _bad(lib, 1, x) == 0
    assert lib.h_unit_parts(0.0) == -np.inf and lib.h_log_unit(0.0) == -np.inf
    # a NaN is outside log_unit's domain; the separated form still gives what the function gives
    assert _bits(lib.h_unit_parts(np.nan)) == _bits(lib.h_log_unit(np.nan))
