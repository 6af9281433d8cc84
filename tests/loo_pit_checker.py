"""ctypes binding of tests/host/loo_pit_host_checker.c, the host statement of PSIS-LOO-PIT on the device
(built on first use with -ffp-contract=off into a temporary directory)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="loo_pit_checker_"), "libloo_pit_checker.so")
        subprocess.check_call(["cc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared",
                               "-I", os.path.join(ROOT, "include"), "-o", out,
                               os.path.join(ROOT, "tests", "host", "loo_pit_host_checker.c"), "-lm"])
        L = C.CDLL(out)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        L.loo_pit.argtypes = [dp, dp, dp, C.c_int, C.c_int, C.c_int, dp, ip]
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def run(ll, yrep, y, tails=False):
    """out [4][N] (p_lt, p_eq, pit, k) of ll, yrep [S][N][C] and y [N] in the device's orders (and the
    tail sizes)"""
    ll = np.ascontiguousarray(ll, dtype=np.float64)
    yrep = np.ascontiguousarray(yrep, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    S, N, Cn = ll.shape
    assert yrep.shape == ll.shape and y.shape == (N,)
    out = np.empty((4, N))
    T = np.zeros(N, dtype=np.int32)
    rc = lib().loo_pit(_dp(ll), _dp(yrep), _dp(y), S, N, Cn, _dp(out), T.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    return (out, T) if tails else out
