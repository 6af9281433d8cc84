"""Host checker for the non-centred sv kind (TEST INFRASTRUCTURE, like tests/gen_checker.py).

tests/host/sv_ncp_checker.c is compiled here with gcc (-O2 -ffp-contract=off, against
include/exmc_detmath.h) into a small shared object and hooked into the CPU oracle as
EXO_MODEL_CUSTOM, with the flat order of sv, so that the oracle's leapfrog / tree / sampler run
over the statement of EXMC_MODEL_SV_NCP. Two entry points:
  sv_ncp_dev  the kernel's association order (scans, butterfly) and detmath: the bit-exact target
              of the GPU tests, used with O.Cfg(1, 64);
  sv_ncp_ref  the reference's order (the walk in sequence, sums left to right) and libm.
Product code never imports this file.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DIR = os.path.join(ROOT, "oracle", "build")
SRC = os.path.join(ROOT, "tests", "host", "sv_ncp_checker.c")
T = 100
D = T + 2

_lib = None


def build():
    """The checker's shared object (rebuilt when its source or the math header is newer)."""
    os.makedirs(OUT_DIR, exist_ok=True)
    so = os.path.join(OUT_DIR, "sv_ncp_checker.so")
    deps = [SRC, os.path.join(ROOT, "include", "exmc_detmath.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = "%s.%d.tmp" % (so, os.getpid())
        fma = ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]
                              + fma + ["-I", os.path.join(ROOT, "include"), "-shared", "-o", tmp, SRC, "-lm"])
        os.replace(tmp, so)
    return so


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        dp = C.POINTER(C.c_double)
        for name in ("sv_ncp_dev", "sv_ncp_ref"):
            f = getattr(L, name)
            f.restype = C.c_double
            f.argtypes = [dp, dp, dp]
        L.sv_ncp_walk.restype = None
        L.sv_ncp_walk.argtypes = [dp, dp, C.c_int]
        _lib = L
    return _lib


def sv_flat_order():
    """The string sort of sv's names (nu, s_1, s_10, s_100, s_11, ..., sigma) as kernel dimensions."""
    names = ["s_%d" % t for t in range(1, T + 1)] + ["sigma", "nu"]
    return sorted(range(D), key=lambda i: names[i])


def model(returns, dev=True):
    """The oracle Model of the kind: data r[100], the custom function of the chosen order."""
    r = np.ascontiguousarray(returns, dtype=np.float64)
    assert r.shape == (T,)
    L = lib()
    m = O.Model(O.EXO_MODEL_CUSTOM, D, r)
    fn = C.cast(L.sv_ncp_dev if dev else L.sv_ncp_ref, C.c_void_p)
    O.lib().exo_model_set_custom(m.h, fn)
    m.set_flat_order(sv_flat_order())
    m.checker_lib = L
    m.lanes = 64
    return m


def logp_grad(returns, q, dev=True):
    r = np.ascontiguousarray(returns, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    g = np.zeros(D)
    f = lib().sv_ncp_dev if dev else lib().sv_ncp_ref
    return f(O.dptr(r), O.dptr(q), O.dptr(g)), g


def walk(q, dev=True):
    """s_1..s_T of a point (kernel order), in the kernel's scan order or in sequence."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    out = np.zeros(T)
    lib().sv_ncp_walk(O.dptr(q), O.dptr(out), 1 if dev else 0)
    return out
