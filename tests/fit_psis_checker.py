"""ctypes binding of tests/host/fit_psis_host_checker.c, the host statement of the smoothing and the
resampling of log importance ratios on the device (built on first use with -ffp-contract=off into a
temporary directory)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ("khat", "log_mean_ratio", "ess", "n_zero", "tail")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="fit_psis_checker_"), "libfit_psis_checker.so")
        subprocess.check_call(["cc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared",
                               "-I", os.path.join(ROOT, "include"), "-o", out,
                               os.path.join(ROOT, "tests", "host", "fit_psis_host_checker.c"), "-lm"])
        L = C.CDLL(out)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        L.fit_psis_first_uniform.argtypes = [C.c_uint64]
        L.fit_psis_first_uniform.restype = C.c_double
        L.fit_psis_groups.argtypes = [dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, dp, dp, ip]
        _lib = L
    return _lib


def first_uniform(seed):
    return lib().fit_psis_first_uniform(seed)


def view(n_draws, n_fits, pooled):
    """(S, Nb, C) of lr [S][n_fits]: per fit the groups are the fits, pooled there is one group"""
    return (n_draws, 1, n_fits) if pooled else (n_draws, n_fits, 1)


def groups(lr, pooled, n_resample=0, seed=0):
    """lr [S][n_fits] -> out [5][G], lw [S][n_fits], idx [R][G] in the device's orders"""
    lr = np.ascontiguousarray(lr, dtype=np.float64)
    S, F = lr.shape
    _, Nb, Cn = view(S, F, pooled)
    out = np.empty((5, Nb))
    lw = np.empty((S, F))
    idx = np.zeros((n_resample, Nb), dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = lib().fit_psis_groups(lr.ctypes.data_as(dp), S, Nb, Cn, n_resample, seed, out.ctypes.data_as(dp),
                               lw.ctypes.data_as(dp), idx.ctypes.data_as(ip))
    assert rc == 0
    return out, lw, idx


def gather(draws, idx, pooled):
    """draws [S][d][n_fits], idx [R][G] -> [R][d][G], NaN where idx < 0"""
    S, d, F = draws.shape
    R, G = idx.shape
    out = np.full((R, d, G), np.nan)
    for j in range(R):
        for g in range(G):
            k = int(idx[j, g])
            if k >= 0:
                s, c = (k // F, k % F) if pooled else (k, g)
                out[j, :, g] = draws[s, :, c]
    return out
