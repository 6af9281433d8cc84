"""ctypes binding of tests/host/ic_host_checker.c, the host statement of model comparison (built on
first use with -ffp-contract=off into a temporary directory), and a numpy/libm statement of the
reference's formulas (lib/exmc/model_comparison.ex:233-276) to hold it against."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ic_checker_"), "libic_checker.so")
        subprocess.check_call(["cc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared",
                               "-I", os.path.join(ROOT, "include"), "-o", out,
                               os.path.join(ROOT, "tests", "host", "ic_host_checker.c"), "-lm"])
        L = C.CDLL(out)
        dp, vp = C.POINTER(C.c_double), C.c_void_p
        L.ic_n_data.argtypes = [C.c_int, C.c_int]
        L.ic_terms.argtypes = [C.c_int, dp, C.c_int, dp, dp]
        L.ic_stats.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, dp]
        L.ic_pointwise.argtypes = [C.c_int, dp, C.c_int, dp, C.c_int, C.c_int, C.c_int, dp]
        L.ic_chunk.argtypes = [C.c_longlong]
        L.ic_chunk.restype = C.c_longlong
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def terms(kind, blob, q):
    blob = np.ascontiguousarray(blob, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    N = lib().ic_n_data(kind, blob.size)
    out = np.empty(N)
    lib().ic_terms(kind, _dp(blob), blob.size, _dp(q), _dp(out))
    return out


def pointwise(kind, blob, draws):
    """ll [S][N][C] of draws [S][d][C]"""
    blob = np.ascontiguousarray(blob, dtype=np.float64)
    x = np.ascontiguousarray(draws, dtype=np.float64)
    S, d, Cn = x.shape
    N = lib().ic_n_data(kind, blob.size)
    ll = np.empty((S, N, Cn))
    lib().ic_pointwise(kind, _dp(blob), blob.size, _dp(x), d, S, Cn, _dp(ll))
    return ll


def stats_from_ll(ll):
    """stats [4][N] of ll [S][N][C] in the device's chunk and merge order"""
    ll = np.ascontiguousarray(ll, dtype=np.float64)
    S, N, Cn = ll.shape
    out = np.empty((4, N))
    lib().ic_stats(ll.ctypes.data, 0, None, 0, None, 0, S, N, Cn, _dp(out))
    return out


def stats_kind(kind, blob, draws):
    blob = np.ascontiguousarray(blob, dtype=np.float64)
    x = np.ascontiguousarray(draws, dtype=np.float64)
    S, d, Cn = x.shape
    N = lib().ic_n_data(kind, blob.size)
    out = np.empty((4, N))
    lib().ic_stats(None, kind, blob.ctypes.data, blob.size, x.ctypes.data, d, S, N, Cn, _dp(out))
    return out


# ---- the reference's formulas, per datum over the pooled samples (libm) ----
def log_mean_exp(v):
    m = max(v)
    return m + math.log(sum(math.exp(x - m) for x in v)) - math.log(len(v))


def variance(v):
    n = len(v)
    if n < 2:
        return 0.0
    mean = sum(v) / n
    return sum((x - mean) * (x - mean) for x in v) / (n - 1)


def reference_stats(ll):
    """[4][N] by model_comparison.ex's log_mean_exp / variance / loo_i_basic over ll [S][N][C]"""
    ll = np.asarray(ll, dtype=np.float64)
    S, N, Cn = ll.shape
    out = np.empty((4, N))
    for i in range(N):
        v = [float(x) for x in ll[:, i, :].reshape(-1)]
        lppd = log_mean_exp(v)
        elpd = -log_mean_exp([-x for x in v])
        out[:, i] = (lppd, variance(v), elpd, lppd - elpd)
    return out
