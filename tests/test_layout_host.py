"""The host library's layout loops (exmc_amd/csrc/exmc_layout_host.hpp: chains_last, transpose_trace_vec,
transpose_trace_scalar, fits_first) compiled for the CPU -- the header includes no HIP header -- against
numpy's transposes: identical arrays. The same shapes run as a stand-alone program under
-fsanitize=address,undefined (tests/host/layout_host_shim.cpp with -DLAYOUT_HOST_MAIN)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "layout_host_shim.cpp")
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)

# (C, S, d): the smallest, an odd one, and more chains than one 64-lane block of the device layout
TRACE_SHAPES = [(1, 1, 1), (3, 2, 5), (65, 2, 3)]
# rows x C of a per-fit result
FIT_SHAPES = [(1, 1), (5, 3)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("layout") / "liblayout_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", out, SRC])
    L = C.CDLL(out)
    L.layout_chains_last.argtypes = L.layout_trace_vec.argtypes = [DP, DP, C.c_int, C.c_int, C.c_int]
    L.layout_trace_scalar_f64.argtypes = [DP, DP, C.c_int, C.c_int]
    L.layout_trace_scalar_i32.argtypes = [IP, IP, C.c_int, C.c_int]
    L.layout_fits_first_f64.argtypes = [DP, DP, C.c_long, C.c_long]
    L.layout_fits_first_i32.argtypes = [IP, IP, C.c_long, C.c_long]
    for f in (L.layout_chains_last, L.layout_trace_vec, L.layout_trace_scalar_f64, L.layout_trace_scalar_i32,
              L.layout_fits_first_f64, L.layout_fits_first_i32):
        f.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(DP if a.dtype == np.float64 else IP)


def test_header_includes_no_hip_header():
    text = open(os.path.join(ROOT, "exmc_amd", "csrc", "exmc_layout_host.hpp")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<cstddef>"]


@pytest.mark.parametrize("Cn,S,d", TRACE_SHAPES)
def test_trace_layouts(shim, Cn, S, d):
    rng = np.random.default_rng(100 * Cn + 10 * S + d)
    host = rng.normal(size=(Cn, S, d))                      # the caller's [C][S][d]
    dev = np.full((S, d, Cn), np.nan)
    shim.layout_chains_last(_p(host), _p(dev), S, d, Cn)
    assert np.array_equal(dev, host.transpose(1, 2, 0))     # the device's [S][d][C]
    back = np.full((Cn, S, d), np.nan)
    shim.layout_trace_vec(_p(dev), _p(back), S, d, Cn)
    assert np.array_equal(back, host)
    sd = rng.normal(size=(S, Cn))
    sh = np.full((Cn, S), np.nan)
    shim.layout_trace_scalar_f64(_p(sd), _p(sh), S, Cn)
    assert np.array_equal(sh, sd.T)
    idv = rng.integers(-2**31, 2**31 - 1, size=(S, Cn), dtype=np.int32)
    ih = np.zeros((Cn, S), dtype=np.int32)
    shim.layout_trace_scalar_i32(_p(idv), _p(ih), S, Cn)
    assert np.array_equal(ih, idv.T)


@pytest.mark.parametrize("rows,Cn", FIT_SHAPES)
def test_fits_first(shim, rows, Cn):
    rng = np.random.default_rng(10 * rows + Cn)
    src = rng.normal(size=(rows, Cn))
    dst = np.full((Cn, rows), np.nan)
    shim.layout_fits_first_f64(_p(src), _p(dst), rows, Cn)
    assert np.array_equal(dst, src.T)
    isrc = rng.integers(-2**31, 2**31 - 1, size=(rows, Cn), dtype=np.int32)
    idst = np.zeros((Cn, rows), dtype=np.int32)
    shim.layout_fits_first_i32(_p(isrc), _p(idst), rows, Cn)
    assert np.array_equal(idst, isrc.T)
    # a null dst is accepted
    shim.layout_fits_first_f64(_p(src), None, rows, Cn)
    shim.layout_fits_first_i32(_p(isrc), None, rows, Cn)
