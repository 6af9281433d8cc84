"""ctypes binding of tests/host/psis_host_checker.c, the host statement of PSIS-LOO on the device (built
on first use with -ffp-contract=off into a temporary directory)."""
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
        out = os.path.join(tempfile.mkdtemp(prefix="psis_checker_"), "libpsis_checker.so")
        subprocess.check_call(["cc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared",
                               "-I", os.path.join(ROOT, "include"), "-o", out,
                               os.path.join(ROOT, "tests", "host", "psis_host_checker.c"), "-lm"])
        L = C.CDLL(out)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        L.psis_expm1.argtypes = [C.c_double]
        L.psis_expm1.restype = C.c_double
        L.psis_expm1_v.argtypes = [dp, C.c_long, dp]
        L.psis_tail_len.argtypes = [C.c_longlong]
        L.psis_fit.argtypes = [dp, C.c_int, dp, dp]
        L.psis_stats.argtypes = [dp, C.c_int, C.c_int, C.c_int, dp, ip]
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def expm1(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    lib().psis_expm1_v(_dp(x), x.size, _dp(out))
    return out


def tail_len(n):
    return lib().psis_tail_len(n)


def fit(t):
    """(k, sigma) of the ascending tail t"""
    t = np.ascontiguousarray(t, dtype=np.float64)
    k, s = C.c_double(), C.c_double()
    lib().psis_fit(_dp(t), t.size, C.byref(k), C.byref(s))
    return k.value, s.value


def stats_from_ll(ll, tails=False):
    """[3][N] (elpd_loo, p_loo, k) of ll [S][N][C] in the device's orders (and the tail sizes)"""
    ll = np.ascontiguousarray(ll, dtype=np.float64)
    S, N, Cn = ll.shape
    out = np.empty((3, N))
    T = np.zeros(N, dtype=np.int32)
    rc = lib().psis_stats(_dp(ll), S, N, Cn, _dp(out), T.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    return (out, T) if tails else out
