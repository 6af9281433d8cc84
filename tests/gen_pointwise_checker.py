"""Host checker for the pointwise section of a generated model (TEST INFRASTRUCTURE, like
tests/gen_checker.py, whose conventions it follows).

The section exmc_amd/codegen.py emits with pointwise=True is compiled here with gcc -- the same text
the plug-in's gen_pointwise_kernel is compiled from, general exmc_detmath.h functions, no contraction --
and evaluated one position at a time. Product code never imports this file.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_DIR = os.path.join(ROOT, "oracle", "build")

WRAPPER = """
#include <math.h>
#include <stddef.h>
#include "exmc_detmath.h"
#define EXMC_GEN_HOST static inline
#define EXMC_GEN_FN static inline
#define EXMC_GEN_EXP exmc_exp
#define EXMC_GEN_LOG exmc_log
#define EXMC_GEN_LOG1P exmc_log1p
#define EXMC_GEN_ERF exmc_erf
/* the section alone (nothing of the sampling layouts is compiled here), under its own #define lines */
%(defines)s
#define EXMC_GEN_PW_SECTION
#define EXMC_GEN_PW_FN static
#define EXMC_GEN_PW_DECL , const double* q, double* out
#define EXMC_GEN_PW_PASS , q, out
#define EXMC_GEN_PW_Q(j) q[j]
#define EXMC_GEN_PW_OUT(i, v) do { if ((i) >= i0 && (i) < i1) out[(i) - i0] = (v); } while (0)
#include "%(header)s"
int exmc_gen_pw_n(void) { return EXMC_GEN_PW_N; }
int exmc_gen_pw_doff(void) { return EXMC_GEN_PW_DOFF; }
int exmc_gen_pw_ndata(void) { return EXMC_GEN_PW_NDATA; }
/* out[i1 - i0]: the datums [i0, i1) at the position q */
void exmc_gen_pw_check(const double* data, const double* q, int i0, int i1, double* out) {
  double c[EXMC_GEN_PW_NCONST];
  exmc_gen_pw_fold(data, c);
  exmc_gen_pw_eval(c, i0, i1, q, out);
}
"""

_keep = {}


def _defines(gen):
    """the section's #define lines (they sit in the part of the header the section include skips)"""
    return "\n".join(ln for ln in gen.header.split("\n") if ln.startswith("#define EXMC_GEN_PW_"))


def build(gen):
    os.makedirs(OUT_DIR, exist_ok=True)
    hdr = os.path.join(OUT_DIR, "genpw_%s.h" % gen.digest)
    src = os.path.join(OUT_DIR, "genpw_%s.c" % gen.digest)
    so = os.path.join(OUT_DIR, "genpw_%s.so" % gen.digest)
    if not os.path.exists(so):
        with open(hdr, "w") as f:
            f.write(gen.header)
        with open(src, "w") as f:
            f.write(WRAPPER % dict(header=hdr, defines=_defines(gen)))
        fma = ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
        subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                               "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unused-variable"] + fma +
                              ["-I", os.path.join(ROOT, "include"), "-shared", "-o", so, src, "-lm"])
    return so


def _lib(gen):
    if gen.digest not in _keep:
        L = C.CDLL(build(gen))
        dp = C.POINTER(C.c_double)
        L.exmc_gen_pw_check.argtypes = [dp, dp, C.c_int, C.c_int, dp]
        L.exmc_gen_pw_check.restype = None
        _keep[gen.digest] = L
    return _keep[gen.digest]


def terms(gen, q, i0=0, i1=None):
    """The datum terms [i0, i1) of `gen` at the positions q [..., d] -> [..., i1 - i0]."""
    L = _lib(gen)
    assert L.exmc_gen_pw_n() == gen.n_datums
    assert L.exmc_gen_pw_doff() + L.exmc_gen_pw_ndata() == gen.data.size or L.exmc_gen_pw_ndata() == 0
    i1 = gen.n_datums if i1 is None else i1
    q = np.ascontiguousarray(q, dtype=np.float64)
    flat = q.reshape(-1, gen.d)
    data = np.ascontiguousarray(gen.data, dtype=np.float64)
    if data.size == 0:
        data = np.zeros(1)
    out = np.empty((flat.shape[0], i1 - i0))
    dp = C.POINTER(C.c_double)
    for k in range(flat.shape[0]):
        row = np.ascontiguousarray(flat[k])
        L.exmc_gen_pw_check(data.ctypes.data_as(dp), row.ctypes.data_as(dp), i0, i1, out[k].ctypes.data_as(dp))
    return out.reshape(q.shape[:-1] + (i1 - i0,))
