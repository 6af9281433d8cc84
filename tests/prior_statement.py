"""A plain-Python statement of Exmc.Predictive.prior_samples (lib/exmc/predictive.ex:19-33, 73-83, 140-196)
for the built-in kinds, written from its text and citing its lines. TEST INFRASTRUCTURE: the product never
imports it. The generator, the Normal / Bernoulli / StudentT samplers and the datums' parameters are those
of tests/predictive_statement.py; exmc_tan_halfpi comes from tests/host/prior_host_shim.c, a host build of
include/exmc_detmath.h.

One chain of a call is prior_samples(ir, S, seed: seed + 7919 (chain_lo + c)): a generator seed_s(:exsss, .)
walks the draws s = 0 .. S - 1 (:27-30). Within a draw the free variables come in the order of topo_sort /
kahn_sort (:140-196) -- always the smallest ready id by string comparison -- over the IR the kind stands for
after Rewrite.apply (:20); kahn_order computes it with that rule from the kind's table of variables
(prior_table), it is not written out. For simple, eight_schools, logistic and radon no variable has a
parent, so the order is the string sort of the names. For sv it is nu, sigma, s_1, ..., s_100: s_1 waits for
sigma, s_t for s_{t-1}. For sv_ncp the non-centring pass (rewrite/non_centered_parameterization.ex:50-55)
has rewritten s_2 .. s_100 to N(0, 1) variables WITHOUT parents: they are ready at once and come in string
order (s_10, s_100, s_11, ...) before sigma, and s_1 ~ N(0.0, sigma), which the pass leaves alone, comes last.
Then the datums follow in the handle's order, as posterior_predictive walks them.

Each variable is dist.sample(resolve_params(params, values), rng) (:75-79), Nx.to_number of the parameters:
  Normal       normal.ex:33-39        mu_f + sigma_f * z, z = normal_s
  HalfCauchy   half_cauchy.ex:34-40   scale_f * tan((pi/2) u), u = uniform_s
  Exponential  exponential.ex:26-31   -log(u) / lambda_f, u = uniform_s
The literals are those of the kind's log-density (exmc_amd/csrc/exmc_models.hpp); where the reference writes
an f32 tensor the value is the f32 value (sv's nu ~ Exponential(f32(0.1))).

Stated deviations (include/exmc_hip_prior.h): one generator per chain; the datums after the variables in the
handle's order; the tangent is exmc_tan_halfpi, of the exact (pi/2) u; uniform_s = 0.0 gives +inf from
Exponential and 0.0 from HalfCauchy where Erlang would raise; for sv_ncp the children see the reconstructed
walk (x), not the raw N(0, 1) value; the datum replicates are project-defined: the family's sample/2 at the
parameters the kind's likelihood has at the unconstrained row q of the draw (PS.datum_params), the very
bits posterior_predictive has at that row.

Outputs per draw: x [d] the constrained values and q [d] the unconstrained position (log for a :log
variable), both in kernel order. For sv_ncp the trace rows 1 .. 99 hold the raw z_t: q holds them, x holds
the walk as the kernels reconstruct it from q (sigma = exp(clamp200(q[100])), the wave scan)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import predictive_statement as PS
from exmc_amd import models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_TENTH = float(np.float32(0.1))

_shim = None


def build_shim(path):
    fma = ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared"]
                          + fma + ["-o", path, os.path.join(ROOT, "tests", "host", "prior_host_shim.c"), "-lm"])
    L = C.CDLL(path)
    L.h_tan_halfpi.argtypes = [C.c_double]
    L.h_tan_halfpi.restype = C.c_double
    L.h_tan_halfpi_n.argtypes = [C.POINTER(C.c_double), C.c_long, C.POINTER(C.c_double)]
    L.h_tan_halfpi_n.restype = None
    return L


def shim():
    global _shim
    if _shim is None:
        tmp = tempfile.mkdtemp(prefix="exmc_prior_shim_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        _shim = build_shim(os.path.join(tmp, "libprior_host.so"))
    return _shim


def tan_halfpi(u):
    return shim().h_tan_halfpi(u)


# ---- sample/2 of the prior families ----------------------------------------------------------------------
def sample_half_cauchy(scale, g):
    u = g.uniform()                          # half_cauchy.ex:36
    return scale * tan_halfpi(u)             # :38 (non-negative: no abs)


def sample_exponential(lam, g):
    u = g.uniform()                          # exponential.ex:28
    return PS._div(-PS._log(u), lam)         # :29 (log(0.0) = -inf: the variate is +inf)


_SAMPLERS = {"normal": PS.sample_normal, "half_cauchy": sample_half_cauchy, "exponential": sample_exponential}


# ---- the kinds' free variables ---------------------------------------------------------------------------
def prior_table(kind, names):
    """{name: (family, parameters, transform)} of the IR the kind stands for after Rewrite.apply; a parameter
    is a number or the name of a parent. `names` are the kind's variable names in kernel order."""
    t = {}
    if kind == models.SIMPLE:
        t["mu"] = ("normal", (0.0, 5.0), None)
        t["sigma"] = ("exponential", (1.0,), "log")
    elif kind == models.EIGHT_SCHOOLS:
        t["mu"] = ("normal", (0.0, 5.0), None)
        t["tau"] = ("half_cauchy", (5.0,), "log")
        for j in range(8):
            t["theta_trans_%d" % j] = ("normal", (0.0, 1.0), None)
    elif kind in (models.SV, models.SV_NCP):
        t["sigma"] = ("exponential", (50.0,), "log")
        t["nu"] = ("exponential", (F32_TENTH,), "log")
        t["s_1"] = ("normal", (0.0, "sigma"), None)
        for k in range(2, 101):
            # sv_ncp: mu and sigma are both references, so the pass rewrites the node to z ~ N(0, 1)
            t["s_%d" % k] = ("normal", (0.0, 1.0) if kind == models.SV_NCP else ("s_%d" % (k - 1), "sigma"), None)
    elif kind == models.LOGISTIC:
        for n in names:
            t[n] = ("normal", (0.0, 10.0), None)
    elif kind == models.RADON:
        for n in names:
            if n.startswith("alpha_raw_"):
                t[n] = ("normal", (0.0, 1.0), None)
        t["mu_alpha"] = ("normal", (0.0, 10.0), None)
        t["gamma_u"] = ("normal", (0.0, 5.0), None)
        t["sigma_alpha"] = ("half_cauchy", (2.5,), "log")
        t["sigma_y"] = ("half_cauchy", (2.5,), "log")
        t["beta"] = ("normal", (0.0, 5.0), None)
    else:
        raise ValueError("no prior walk for kind %r" % kind)
    assert sorted(t) == sorted(names)
    return t


def kahn_order(table):
    """topo_sort / kahn_sort (predictive.ex:140-196): the queue is kept sorted, its head is taken"""
    deps = {n: [p for p in par if isinstance(p, str) and p in table] for n, (_, par, _) in table.items()}   # :144-154
    in_degree = {n: len(p) for n, p in deps.items()}                        # :161-162
    queue = sorted(n for n, k in in_degree.items() if k == 0)               # :164-168
    out = []
    while queue:                                                            # do_kahn, :173-196
        n = queue.pop(0)
        new_ready = []
        for child, parents in deps.items():                                 # :180-192
            if n in parents:
                in_degree[child] -= 1
                if in_degree[child] == 0:
                    new_ready.append(child)
        queue = sorted(queue + new_ready)                                   # :194
        out.append(n)
    return out


def sample_prior_once(table, order, g):
    """sample_prior_once (predictive.ex:73-83): {name: constrained value}"""
    values = {}
    for n in order:
        fam, par, _ = table[n]
        resolved = [values[p] if isinstance(p, str) else p for p in par]    # resolve_params, :115-120
        values[n] = _SAMPLERS[fam](*resolved, g)
    return values


def position(kind, names, table, values):
    """(x [d], q [d]) of one draw in kernel order"""
    x = [values[n] for n in names]
    q = [PS._log(v) if table[n][2] == "log" else v for n, v in zip(names, x)]
    if kind == models.SV_NCP:
        sigma = PS._exp(PS.clamp200(q[100]))
        x[:100] = PS.scan_fwd64([q[0] if i == 0 else (sigma * q[i] if i < 100 else 0.0) for i in range(128)])[:100]
    return x, q


def prior_samples(spec, S, seed=0, state=None, counters=None, replicates=True, gen=None):
    """One chain: (x [S][d], q [S][d], yrep [S][N] or None, the generator's final state (a, b))"""
    g = gen if gen is not None else PS.Gen(seed=seed, state=state, counters=counters)    # predictive.ex:21-22
    kind, names = spec.kind, spec.var_names
    blob = np.asarray(spec.data, dtype=np.float64)
    table = prior_table(kind, names)
    order = kahn_order(table)                                                            # :24-25
    N = PS.n_data(kind, blob)
    x, q = np.empty((S, spec.d)), np.empty((S, spec.d))
    yrep = np.empty((S, N)) if replicates else None
    for s in range(S):                                                                   # :27-30
        x[s], q[s] = position(kind, names, table, sample_prior_once(table, order, g))
        if replicates:
            for i, (fam, *par) in enumerate(PS.datum_params(kind, blob, q[s])):
                yrep[s, i] = PS._SAMPLERS[fam](*par, g)
    return x, q, yrep, g.state()


def run(spec, S, Cn, seed=0, chain_lo=0, states=None, replicates=True):
    """The call: (x [S][d][C], q [S][d][C], yrep [S][N][C] or None, states [2][C] uint64, counters). Chain c
    draws with seed + 7919 (chain_lo + c), or goes on from states[:, c]."""
    blob = np.asarray(spec.data, dtype=np.float64)
    x, q = np.empty((S, spec.d, Cn)), np.empty((S, spec.d, Cn))
    yrep = np.empty((S, PS.n_data(spec.kind, blob), Cn)) if replicates else None
    out_states = np.zeros((2, Cn), dtype=np.uint64)
    n = PS.new_counters()
    for c in range(Cn):
        xc, qc, yc, st = prior_samples(spec, S, seed=int(seed) + 7919 * (int(chain_lo) + c),
                                       state=None if states is None else states[:, c], counters=n,
                                       replicates=replicates)
        x[:, :, c], q[:, :, c] = xc, qc
        if replicates:
            yrep[:, :, c] = yc
        out_states[:, c] = st
    return x, q, yrep, out_states, n


# ---- the inputs of the GPU parity tests, computed once per process ---------------------------------------
C_PAR, S_PAR, SEED, CHAIN_LO = 70, 3, 19, 2     # two wavefronts, the second partial
_expected = {}


def expected(kind, Cn=C_PAR, S=S_PAR):
    """(x, q, yrep, states, counters) of the statement at the parity sizes"""
    import predictive_inputs as PI
    key = (kind, Cn, S)
    if key not in _expected:
        _expected[key] = run(PI.spec(kind), S, Cn, seed=SEED, chain_lo=CHAIN_LO)
    return _expected[key]
