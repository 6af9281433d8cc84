"""Importance diagnostics of the variational fits over libexmc_hip.so (include/exmc_hip_fit_psis.h).

    psis_fit(compiled, raw, pooled=False, num_resample=0, seed=0, lanes_per_chain=0) -> dict

`raw` is the dict of pathfinder.fit_raw or advi.fit_raw: draws [C][S][d], mu [C][d] and `sigma`
(Pathfinder) or `log_sigma` (ADVI) [C][d], all unconstrained and in kernel order. The device evaluates
log p - log q at every draw under its own fit, Pareto-smooths the ratios per fit or pooled over all fits,
and resamples the draws systematically from the smoothed weights. The Pareto k answers whether an
approximation is usable (Yao, Vehtari, Simpson, Gelman 2018: below 0.7); pooled over the paths with
num_resample > 0 the result is multi-path Pathfinder's importance resampling (Zhang et al. 2022).

The result holds, per group (per fit: arrays over the fits; pooled: scalars):
    khat, log_mean_ratio, ess, n_zero, tail    the rows of the device's out [5][G]
    log_weights    [C][S], the normalised smoothed log weights of every draw (NaN in a NaN group)
    indices        per fit [C][R], the draw picked; pooled [R], the pooled index k = s C + c
    draws          per fit [C][R][d]; pooled [R][d]: the resampled draws, unconstrained
    trace          sampler._build_trace of them: per fit a list, pooled one trace (None without resampling)
    kept, dropped  pooled: the fits that were pooled and the ones left out (status != 0, or a non-finite
                   mu or scale), by their index in `raw`; C above counts the kept fits, in that order
    kernel_ms      the time of the device launches
There is no CPU fallback. A generated model evaluates its ratios in its plug-in library and has them
smoothed by libexmc_hip.so's model-free calls, as its pointwise terms are."""
import ctypes as C

import numpy as np

from . import _lib
from .codegen import CUSTOM


def _scale(raw):
    if ("sigma" in raw) == ("log_sigma" in raw):
        raise ValueError("raw must hold sigma (pathfinder.fit_raw) or log_sigma (advi.fit_raw)")
    return (raw["sigma"], _lib.FIT_SIGMA) if "sigma" in raw else (raw["log_sigma"], _lib.FIT_LOG_SIGMA)


def psis_fit(compiled, raw, pooled=False, num_resample=0, seed=0, lanes_per_chain=0):
    scale, kind = _scale(raw)
    draws = np.ascontiguousarray(raw["draws"], dtype=np.float64)
    mu = np.ascontiguousarray(raw["mu"], dtype=np.float64)
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    if draws.ndim != 3 or draws.shape[2] != compiled.d or mu.shape != (draws.shape[0], compiled.d) or \
            scale.shape != mu.shape:
        raise ValueError("raw must hold draws [C][S][d] and mu and a scale [C][d]")
    R = int(num_resample)
    if R < 0:
        raise ValueError("num_resample must be >= 0")
    kept = np.arange(draws.shape[0])
    dropped = kept[:0]
    if pooled:
        ok = np.all(np.isfinite(mu), axis=1) & np.all(np.isfinite(scale), axis=1)
        if "status" in raw:
            ok &= np.asarray(raw["status"]) == 0
        kept, dropped = np.nonzero(ok)[0], np.nonzero(~ok)[0]
        if kept.size == 0:
            raise ValueError("no fit is left to pool: every fit failed or has a non-finite mu or scale")
        draws, mu, scale = (np.ascontiguousarray(a[kept]) for a in (draws, mu, scale))
    Cn, S, d = draws.shape
    G = 1 if pooled else Cn
    run = _run_generated if compiled.spec.kind == CUSTOM else _run_kind
    out, lw, idx, res, ms = run(compiled, draws, mu, scale, kind, bool(pooled), R, int(seed) & (2 ** 64 - 1),
                                int(lanes_per_chain or 0))
    r = {k: (float(out[i, 0]) if pooled else out[i].copy()) for i, k in enumerate(_lib.FIT_PSIS_ROWS)}
    r["log_weights"] = lw
    r["kernel_ms"] = ms
    if pooled:
        r["kept"], r["dropped"] = kept, dropped
    from . import sampler
    if R == 0:
        r["indices"] = np.zeros((R,) if pooled else (Cn, R), dtype=np.int32)
        r["draws"] = r["trace"] = None
    elif pooled:
        r["indices"], r["draws"] = idx[0], res[0]
        r["trace"] = sampler._build_trace(compiled.spec, res[0]) if idx[0, 0] >= 0 else None
    else:
        r["indices"], r["draws"] = idx, res
        r["trace"] = [sampler._build_trace(compiled.spec, res[c]) if idx[c, 0] >= 0 else None for c in range(Cn)]
    assert out.shape == (len(_lib.FIT_PSIS_ROWS), G)
    return r


def _run_kind(compiled, draws, mu, scale, kind, pooled, R, seed, lanes):
    """exmc_hip_fit_psis_host: the whole chain on the handle's stream"""
    Cn, S, d = draws.shape
    G = 1 if pooled else Cn
    out = np.zeros((len(_lib.FIT_PSIS_ROWS), G))
    lw = np.zeros((Cn, S))
    idx = np.zeros((G, R), dtype=np.int32)
    res = np.zeros((G, R, d))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    compiled.check(compiled.L.exmc_hip_fit_psis_host(
        compiled.h, draws.ctypes.data_as(dp), mu.ctypes.data_as(dp), scale.ctypes.data_as(dp), kind, S, d, Cn, lanes,
        int(pooled), R, seed, out.ctypes.data_as(dp), lw.ctypes.data_as(dp), idx.ctypes.data_as(ip),
        res.ctypes.data_as(dp), None, None))
    return out, lw, idx, res, compiled.last_kernel_ms


def _run_generated(compiled, draws, mu, scale, kind, pooled, R, seed, lanes):
    """the plug-in's exmc_hip_fit_log_ratio, then libexmc_hip.so's model-free smoothing, resampling and gather"""
    import torch
    from .diagnostics import _ordered_after_torch
    Cn, S, d = draws.shape
    G = 1 if pooled else Cn
    dev = torch.device("cuda", compiled.device)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    x, m, sc = up(draws.transpose(1, 2, 0)), up(mu.T), up(scale.T)        # [S][d][C], [d][C]
    lr = torch.empty((S, Cn), dtype=torch.float64, device=dev)
    lw = torch.empty((S, Cn), dtype=torch.float64, device=dev)
    out = torch.empty((len(_lib.FIT_PSIS_ROWS), G), dtype=torch.float64, device=dev)
    idx = torch.empty((max(R, 1), G), dtype=torch.int32, device=dev)
    res = torch.empty((max(R, 1), d, G), dtype=torch.float64, device=dev)
    _ordered_after_torch(x)
    compiled.check(compiled.L.exmc_hip_fit_log_ratio(compiled.h, x.data_ptr(), m.data_ptr(), sc.data_ptr(), kind, S, d,
                                                     Cn, lanes, lr.data_ptr(), None))
    ms = compiled.last_kernel_ms
    main = _lib.load()
    _lib.check(main.exmc_hip_ratio_psis_from_lr(compiled.device, lr.data_ptr(), S, Cn, int(pooled), R, seed,
                                                out.data_ptr(), lw.data_ptr(), idx.data_ptr() if R else None), main)
    if R:
        _lib.check(main.exmc_hip_ratio_gather(compiled.device, x.data_ptr(), idx.data_ptr(), S, d, Cn, int(pooled), R,
                                              res.data_ptr()), main)
    torch.cuda.synchronize(dev)
    idx_h = np.ascontiguousarray(idx.cpu().numpy()[:R].T)                       # [G][R]
    res_h = np.ascontiguousarray(res.cpu().numpy()[:R].transpose(2, 0, 1))      # [G][R][d]
    return out.cpu().numpy(), np.ascontiguousarray(lw.cpu().numpy().T), idx_h, res_h, ms
