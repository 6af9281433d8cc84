"""Host-side mirror of Exmc.Pathfinder (lib/exmc/pathfinder.ex) over libexmc_hip.so.

    fit(ir, opts)                 -> (draws, info)                     pathfinder.ex:30-56
    fit(ir, opts, num_paths=n)    -> ([draws], [info], best_path)      path c: seed + 7919 c

`draws` is {name: [num_draws, ...]} in constrained space (sampler._build_trace, so the non-centred
kinds report the reconstructed variables), `info` is {elbo, mu, sigma, num_iters} with mu and sigma in
the unconstrained kernel space, plus best_index and status (1: no path point had a finite ELBO; the
results are NaN then, where the reference raises). The whole fit -- start, L-BFGS path, ELBO of
every path point, the draws -- is one kernel launch with one path per lane group
(include/exmc_hip_pathfinder.h). There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib

DEFAULT_OPTS = dict(num_draws=1000, max_iters=100, history_size=6, seed=0)   # pathfinder.ex:16-21


def _validate(opts, num_paths):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    if int(o["max_iters"]) < 1:
        raise ValueError("max_iters must be >= 1")
    if int(o["num_draws"]) < 1:
        raise ValueError("num_draws must be >= 1")
    if not 1 <= int(o["history_size"]) <= _lib.PF_MAX_HISTORY:
        raise ValueError("history_size must be in 1..%d" % _lib.PF_MAX_HISTORY)
    if int(num_paths) < 1:
        raise ValueError("num_paths must be >= 1")
    if int(o.get("chain_lo", 0)) < 0:
        raise ValueError("chain_lo must be >= 0")
    return o


def fit_raw(compiled, opts=None, num_paths=1):
    """The arrays of exmc_hip_pathfinder_host: draws [C][S][d] (unconstrained, kernel order), mu and
    sigma [C][d], elbo, num_iters, best_index, status [C]. opts["chain_lo"] offsets the seeds."""
    o = _validate(opts, num_paths)
    Cn, S, d = int(num_paths), int(o["num_draws"]), compiled.d
    out = dict(draws=np.zeros((Cn, S, d)), mu=np.zeros((Cn, d)), sigma=np.zeros((Cn, d)), elbo=np.zeros(Cn),
               num_iters=np.zeros(Cn, np.int32), best_index=np.zeros(Cn, np.int32), status=np.zeros(Cn, np.int32))
    po = _lib.PfOpts(S, int(o["max_iters"]), int(o["history_size"]), int(o["seed"]),
                     int(o.get("lanes_per_chain") or 0))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    compiled.check(compiled.L.exmc_hip_pathfinder_host(
        compiled.h, po, Cn, int(o.get("chain_lo", 0)),
        *[out[k].ctypes.data_as(dp) for k in ("draws", "mu", "sigma", "elbo")],
        *[out[k].ctypes.data_as(ip) for k in ("num_iters", "best_index", "status")]))
    out["kernel_ms"] = compiled.last_kernel_ms
    return out


def fit(ir_or_compiled, opts=None, num_paths=1):
    """Exmc.Pathfinder.fit/2; with num_paths > 1 a batch of paths and the index of the largest ELBO."""
    o = _validate(opts, num_paths)        # before the library is touched
    from . import sampler
    compiled = ir_or_compiled if isinstance(ir_or_compiled, sampler.Compiled) else \
        sampler.Compiled(ir_or_compiled, device=o.get("device", 0))
    raw = fit_raw(compiled, o, num_paths)
    draws, infos = [], []
    for c in range(int(num_paths)):
        draws.append(sampler._build_trace(compiled.spec, raw["draws"][c]))
        infos.append(dict(elbo=float(raw["elbo"][c]), mu=raw["mu"][c], sigma=raw["sigma"][c],
                          num_iters=int(raw["num_iters"][c]), best_index=int(raw["best_index"][c]),
                          status=int(raw["status"][c])))
    if int(num_paths) == 1:
        return draws[0], infos[0]
    elbo = np.where(np.isfinite(raw["elbo"]), raw["elbo"], -np.inf)
    return draws, infos, int(np.argmax(elbo))


def fit_psis(ir_or_compiled, opts=None, num_paths=1, pooled=False, num_resample=0, resample_seed=0):
    """fit_raw, then importance.psis_fit over its paths: the Pareto k of every fit (or of the pool), the
    smoothed log weights and, with num_resample > 0, the importance-resampled draws. Returns (raw, result)."""
    o = _validate(opts, num_paths)
    from . import importance, sampler
    compiled = ir_or_compiled if isinstance(ir_or_compiled, sampler.Compiled) else \
        sampler.Compiled(ir_or_compiled, device=o.get("device", 0))
    raw = fit_raw(compiled, o, num_paths)
    return raw, importance.psis_fit(compiled, raw, pooled=pooled, num_resample=num_resample, seed=resample_seed,
                                    lanes_per_chain=int(o.get("lanes_per_chain") or 0))
