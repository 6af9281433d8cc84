"""A plain-Python statement of Exmc.Predictive.posterior_predictive (lib/exmc/predictive.ex:44-63,
98-108) and of the sample/2 callbacks it calls for the built-in kinds, written from their texts and
citing their lines. TEST INFRASTRUCTURE: the product never imports it.

One chain of a call is posterior_predictive(ir, trace_c, seed: seed + 7919 (chain_lo + c)): a generator
seed_s(:exsss, .) walks the draws s = 0 .. S - 1 and within a draw the datums i = 0 .. N - 1, each
datum's replicate dist.sample(params, rng) (:98-108) of the datum's family:
  Normal     normal.ex:33-39      mu_f + sigma_f * z, z = normal_s
  Bernoulli  bernoulli.ex:36-41   u = uniform_s; 1.0 if u < p_f else 0.0
  StudentT   student_t.ex:38-46   z = normal_s; chi2 = sample_gamma(df_f / 2.0, 0.5);
                                  loc_f + scale_f * z / sqrt(chi2 / df_f)
  sample_gamma  gamma.ex:43-72    Marsaglia-Tsang, the alpha < 1 boost
The generator is the checker's (exo_rng_seed / exo_rng_uniform / exo_rng_normal in deterministic-math
mode), exp and log are exo_det_exp / exo_det_log; sqrt and / are IEEE. Products and sums round
separately. The parameters per kind are DESIGN.md "Posterior predictive"'s table.

Stated deviations (include/exmc_hip_predictive.h): one generator per chain, where the reference has
one for the one trace it is handed; the datums in the handle's order, where the reference walks obs
nodes in map order; :math.pow(u, 1.0 / alpha) as exp((1.0 / alpha) * log(u)); a gamma variate whose loop
rejects GAMMA_CAP times in a row is NaN and the generator goes on from there (the reference loops on).

Every sampler counts the branches it takes (COUNTERS), so that a test can show its inputs reach them."""
import ctypes as C
import math

import numpy as np

import oracle as O

SIMPLE, EIGHT_SCHOOLS, SV, LOGISTIC, RADON, SV_NCP = 1, 2, 3, 4, 5, 7
GAMMA_CAP = 64
TINY32 = float(np.float32(1.0e-30))
COUNTERS = ("zig_wedge", "zig_tail", "gamma_v_reject", "gamma_log_reject", "boost", "cap")

_libm = C.CDLL("libm.so.6")
_libm.fma.argtypes = [C.c_double] * 3
_libm.fma.restype = C.c_double
fma = _libm.fma


def new_counters():
    return {k: 0 for k in COUNTERS}


# ---- IEEE arithmetic where Python's floats raise ----------------------------------------------------
def _div(a, b):
    if b == 0.0 or b != b:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))
    return a / b


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else math.nan      # NaN compares false


def _fmax(a, b):   # C's fmax / fmin: the number where one argument is NaN
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def clamp200(z):
    return _fmax(-200.0, _fmin(z, 200.0))


def _exp(x):
    return O.lib().exo_det_exp(x)


def _log(x):
    return O.lib().exo_det_log(x)


# ---- the generator -------------------------------------------------------------------------------------
class Gen:
    """:rand's exsss state of one chain and the branch counters of what it has drawn"""

    def __init__(self, seed=None, state=None, counters=None):
        self.r = O.Rng()
        self.L = O.lib()
        if state is not None:
            self.r.a, self.r.b = int(state[0]), int(state[1])
        else:
            self.L.exo_rng_seed(C.byref(self.r), int(seed) & 0xFFFFFFFFFFFFFFFF)
        self.n = counters if counters is not None else new_counters()

    def state(self):
        return int(self.r.a), int(self.r.b)

    def uniform(self):
        return self.L.exo_rng_uniform(C.byref(self.r))

    def normal(self):
        """normal_s; which ziggurat branch it took is read off the words it consumed: the first word
        alone is the fast accept, otherwise its layer (bits 7..14) says tail (layer 0) or wedge"""
        before = O.Rng(self.r.a, self.r.b)
        z = self.L.exo_rng_normal(C.byref(self.r), 1)
        w = self.L.exo_rng_next(C.byref(before))
        if (before.a, before.b) != (self.r.a, self.r.b):
            self.n["zig_tail" if ((w >> 7) & 255) == 0 else "zig_wedge"] += 1
        return z


# ---- sample/2 of the families --------------------------------------------------------------------------
def sample_normal(loc, scale, g):
    z = g.normal()                      # normal.ex:36
    return loc + scale * z              # :37


def sample_bernoulli(p, g):
    u = g.uniform()                     # bernoulli.ex:38
    return 1.0 if u < p else 0.0        # :39 (a NaN p compares false)


def sample_gamma(alpha, beta, g):
    """gamma.ex:43-72. An alpha that is not >= 1.0 takes the second clause once (:49-54)."""
    boost = not (alpha >= 1.0)
    a = alpha + 1.0 if boost else alpha
    d = a - 1.0 / 3.0                   # :44
    c = _div(1.0, _sqrt(9.0 * d))       # :45
    value = math.nan
    for _ in range(GAMMA_CAP):          # marsaglia_loop, :56-72, at most GAMMA_CAP rounds
        x = g.normal()                  # :57
        v = 1.0 + c * x                 # :58
        if v <= 0.0:                    # :60
            g.n["gamma_v_reject"] += 1
            continue
        v = (v * v) * v                 # :63
        u = g.uniform()                 # :64
        if _log(u) < (((0.5 * x) * x + d) - d * v) + d * _log(v):   # :66
            value = _div(d * v, beta)   # :67
            break
        g.n["gamma_log_reject"] += 1
    else:
        g.n["cap"] += 1
    if boost:
        g.n["boost"] += 1
        u = g.uniform()                 # :52
        value = value * _exp(_div(1.0, alpha) * _log(u))   # :53, pow as exp(log)
    return value


def sample_student_t(df, loc, scale, g):
    z = g.normal()                                  # student_t.ex:42
    chi2 = sample_gamma(df / 2.0, 0.5, g)           # :43
    return loc + _div(scale * z, _sqrt(_div(chi2, df)))   # :44


# ---- the datums' parameters per kind (DESIGN.md "Posterior predictive") ---------------------------------
def scan_fwd64(x):
    """include/exmc_scan.h exmc_scan_fwd64: x of 64 * nslots floats, in place"""
    nslots = len(x) // 64
    for k in range(nslots):
        v = x[64 * k:64 * k + 64]
        d = 1
        while d < 16:
            v = [v[l] + v[l - d] if (l & 15) >= d else v[l] for l in range(64)]
            d <<= 1
        t = [v[(l & ~15) + 15] for l in range(64)]
        t2 = [0.0] * 64
        for l in range(64):
            p = t[l ^ 16]
            if l & 16:
                v[l] = v[l] + p
            t2[l] = t[l] + p
        for l in range(64):
            if l & 32:
                v[l] = v[l] + t2[l ^ 32]
        x[64 * k:64 * k + 64] = v
    for k in range(1, nslots):
        carry = x[64 * k - 1]
        for l in range(64):
            x[64 * k + l] = x[64 * k + l] + carry
    return x


def n_data(kind, blob):
    n = len(blob)
    return {SIMPLE: n, EIGHT_SCHOOLS: 8, SV: 100, SV_NCP: 100, LOGISTIC: n // 21, RADON: (n - 171) // 2}[kind]


def datum_params(kind, blob, q):
    """[(family, parameters...)] of the N datums at the sample q [d] (kernel order)"""
    q = [float(v) for v in q]
    N = n_data(kind, blob)
    if kind == SIMPLE:
        scale = _fmax(_exp(clamp200(q[1])), TINY32)
        return [("normal", q[0], scale)] * N
    if kind == EIGHT_SCHOOLS:
        tau = _exp(clamp200(q[1]))
        return [("normal", q[0] + tau * q[2 + j], float(blob[8 + j])) for j in range(8)]
    if kind in (SV, SV_NCP):
        df = _fmax(_exp(clamp200(q[101])), TINY32)
        if kind == SV_NCP:
            sigma = _exp(clamp200(q[100]))
            s = scan_fwd64([q[0] if i == 0 else (sigma * q[i] if i < 100 else 0.0) for i in range(128)])
        else:
            s = q
        return [("student_t", df, 0.0, _exp(s[t])) for t in range(100)]
    if kind == LOGISTIC:
        out = []
        for i in range(N):
            eta = q[0]
            for j in range(20):
                eta = fma(float(blob[i * 20 + j]), q[1 + j], eta)
            out.append(("bernoulli", 1.0 / (1.0 + _exp(-eta))))
        return out
    if kind == RADON:
        J = 85
        u, cs, fl = blob[:J], blob[J:2 * J + 1], blob[2 * J + 1:2 * J + 1 + N]
        sa = _exp(clamp200(q[J + 2]))
        scale = _fmax(_exp(clamp200(q[J + 3])), TINY32)
        out = []
        for j in range(J):
            alpha = (q[J] + q[J + 1] * float(u[j])) + sa * q[j]
            for i in range(int(cs[j]), int(cs[j + 1])):
                out.append(("normal", alpha + q[J + 4] * float(fl[i]), scale))
        return out
    raise ValueError("no datums for kind %r" % kind)


_SAMPLERS = {"normal": sample_normal, "bernoulli": sample_bernoulli, "student_t": sample_student_t}


def posterior_predictive(kind, blob, trace, seed=0, state=None, counters=None):
    """One chain: trace [S][d] -> (yrep [S][N], the generator's final state (a, b)). state: the
    generator an earlier call left (then seed is not read)."""
    g = Gen(seed=seed, state=state, counters=counters)     # predictive.ex:46-47
    trace = np.asarray(trace, dtype=np.float64)
    blob = np.asarray(blob, dtype=np.float64)
    out = np.empty((trace.shape[0], n_data(kind, blob)))
    for s in range(trace.shape[0]):                        # :57
        for i, (fam, *par) in enumerate(datum_params(kind, blob, trace[s])):   # :100-104
            out[s, i] = _SAMPLERS[fam](*par, g)
    return out, g.state()


def run(kind, blob, draws, seed=0, chain_lo=0, states=None):
    """The call: draws [S][d][C] -> (yrep [S][N][C], states [2][C] uint64, counters). Chain c draws
    with seed + 7919 (chain_lo + c), or goes on from states[:, c]."""
    draws = np.asarray(draws, dtype=np.float64)
    S, d, Cn = draws.shape
    blob = np.asarray(blob, dtype=np.float64)
    yrep = np.empty((S, n_data(kind, blob), Cn))
    out_states = np.zeros((2, Cn), dtype=np.uint64)
    n = new_counters()
    for c in range(Cn):
        y, st = posterior_predictive(kind, blob, draws[:, :, c], seed=int(seed) + 7919 * (int(chain_lo) + c),
                                     state=None if states is None else states[:, c], counters=n)
        yrep[:, :, c] = y
        out_states[:, c] = st
    return yrep, out_states, n
