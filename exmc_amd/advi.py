"""Host-side mirror of Exmc.ADVI (lib/exmc/advi.ex) over libexmc_hip.so.

    fit(ir, opts)                -> (draws, info)                     advi.ex:21-50
    fit(ir, opts, num_fits=n)    -> ([draws], [info], best_fit)       fit c: seed + 7919 c

`draws` is {name: [num_draws, ...]} in constrained space (sampler._build_trace, so the non-centred
kinds report the reconstructed variables), `info` is {elbo_history, mu, log_sigma, converged,
num_iters} with elbo_history a list of num_iters floats and mu and log_sigma in the unconstrained
kernel space. best_fit is the first fit of the largest mean ELBO over its last half window. The whole
fit -- the stochastic-gradient loop, its convergence test, the draws -- is one kernel launch with one
fit per lane group (include/exmc_hip_advi.h). There is no CPU fallback. An IR without free variables
(advi.ex:25-26) does not reach this module: the generator refuses it."""
import ctypes as C

import numpy as np

from . import _lib

# advi.ex:11-19
DEFAULT_OPTS = dict(num_draws=1000, max_iters=10000, learning_rate=0.01, num_mc_samples=1, seed=0,
                    convergence_tol=1.0e-4, window_size=100)


def _validate(opts, num_fits):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    for key in ("max_iters", "num_draws", "num_mc_samples"):
        if int(o[key]) < 1:
            raise ValueError("%s must be >= 1" % key)
    if int(o["window_size"]) < 2:
        raise ValueError("window_size must be >= 2")
    if int(num_fits) < 1:
        raise ValueError("num_fits must be >= 1")
    if int(o.get("chain_lo", 0)) < 0:
        raise ValueError("chain_lo must be >= 0")
    float(o["learning_rate"]), float(o["convergence_tol"])
    return o


def fit_raw(compiled, opts=None, num_fits=1):
    """The arrays of exmc_hip_advi_host: draws [C][S][d] (unconstrained, kernel order), mu and
    log_sigma [C][d], elbo_history [C][max_iters] (NaN at and after num_iters), num_iters and
    converged [C]. opts["chain_lo"] offsets the seeds."""
    o = _validate(opts, num_fits)
    Cn, S, d, iters = int(num_fits), int(o["num_draws"]), compiled.d, int(o["max_iters"])
    out = dict(draws=np.zeros((Cn, S, d)), mu=np.zeros((Cn, d)), log_sigma=np.zeros((Cn, d)),
               elbo_history=np.zeros((Cn, iters)), num_iters=np.zeros(Cn, np.int32),
               converged=np.zeros(Cn, np.int32))
    ao = _lib.AdviOpts(S, iters, int(o["num_mc_samples"]), int(o["window_size"]), float(o["learning_rate"]),
                       float(o["convergence_tol"]), int(o["seed"]), int(o.get("lanes_per_chain") or 0))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    compiled.check(compiled.L.exmc_hip_advi_host(
        compiled.h, ao, Cn, int(o.get("chain_lo", 0)),
        *[out[k].ctypes.data_as(dp) for k in ("draws", "mu", "log_sigma", "elbo_history")],
        *[out[k].ctypes.data_as(ip) for k in ("num_iters", "converged")]))
    out["kernel_ms"] = compiled.last_kernel_ms
    return out


def fit(ir_or_compiled, opts=None, num_fits=1):
    """Exmc.ADVI.fit/2; with num_fits > 1 a batch of fits and the index of the best one."""
    o = _validate(opts, num_fits)        # before the library is touched
    from . import sampler
    compiled = ir_or_compiled if isinstance(ir_or_compiled, sampler.Compiled) else \
        sampler.Compiled(ir_or_compiled, device=o.get("device", 0))
    raw = fit_raw(compiled, o, num_fits)
    h = int(o["window_size"]) // 2
    draws, infos, score = [], [], []
    for c in range(int(num_fits)):
        n = int(raw["num_iters"][c])
        hist = raw["elbo_history"][c, :n]
        draws.append(sampler._build_trace(compiled.spec, raw["draws"][c]))
        infos.append(dict(elbo_history=[float(x) for x in hist], mu=raw["mu"][c], log_sigma=raw["log_sigma"][c],
                          converged=bool(raw["converged"][c]), num_iters=n))
        tail = float(np.mean(hist[-h:]))
        score.append(tail if np.isfinite(tail) else -np.inf)
    if int(num_fits) == 1:
        return draws[0], infos[0]
    return draws, infos, int(np.argmax(score))


def fit_psis(ir_or_compiled, opts=None, num_fits=1, pooled=False, num_resample=0, resample_seed=0):
    """fit_raw, then importance.psis_fit over its fits: the Pareto k of every fit (or of the pool), the
    smoothed log weights and, with num_resample > 0, the importance-resampled draws. Returns (raw, result)."""
    o = _validate(opts, num_fits)
    from . import importance, sampler
    compiled = ir_or_compiled if isinstance(ir_or_compiled, sampler.Compiled) else \
        sampler.Compiled(ir_or_compiled, device=o.get("device", 0))
    raw = fit_raw(compiled, o, num_fits)
    return raw, importance.psis_fit(compiled, raw, pooled=pooled, num_resample=num_resample, seed=resample_seed,
                                    lanes_per_chain=int(o.get("lanes_per_chain") or 0))
