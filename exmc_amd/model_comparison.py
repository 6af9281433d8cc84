"""Host-side mirror of Exmc.ModelComparison (lib/exmc/model_comparison.ex) over the device kernels.

    pointwise_log_likelihood(compiled, draws) -> (ll [S][N][C] device tensor, datum names)
    waic(compiled, draws)  -> {waic, elpd_waic, p_waic, se, n_obs, pointwise}   model_comparison.ex:63-84
    loo(compiled, draws)   -> {loo, elpd_loo, p_loo, se, n_obs, pointwise}      model_comparison.ex:95-114
    waic_from_pointwise(ll) / loo_from_pointwise(ll)  the same from a matrix [S][N][C]
    psis_loo(compiled, draws) / psis_loo_from_pointwise(ll)  Pareto-smoothed LOO: loo's keys, plus
                           pointwise["pareto_k"], k_threshold and n_high_k (DESIGN.md "PSIS-LOO")
    compare(results)       -> the results sorted by IC with d_elpd              model_comparison.ex:127-150

The unit is the datum of a built-in kind (include/exmc_hip_compare.h, DESIGN.md "Model comparison"):
one y_i, one return r_t. `draws` is the device trace [S][d][C] or a host array [C][S][d], as for
exmc_amd/diagnostics.py. The per-datum statistics (lppd_i, p_waic_i, elpd_loo_i, p_loo_i) are formed on
the GPU in one pass over the trace; the totals and `se` here, with the reference's formulas, summing in
datum order.

A generated model takes part when it was compiled with its per-datum terms (codegen.compile_ir(...,
pointwise=True)): its datums are the terms of its obs nodes (DESIGN.md "Per-datum terms of generated
models"). Its plug-in evaluates them over the trace a block of datums at a time
(exmc_hip_pointwise_loglik_range) and libexmc_hip.so's model-free reductions take each block; the
result per datum does not depend on the blocking. Generated models compiled without them form their ll
matrix themselves and use the *_from_pointwise forms. No CPU fallback.
"""
import math

import numpy as np

from . import _lib
from .diagnostics import _device_trace, _ordered_after_torch
from .codegen import CUSTOM   # a generated model's plug-in
from .models import EIGHT_SCHOOLS, LOGISTIC, RADON, SIMPLE, SV, SV_NCP

# pointwise_log_likelihood refuses matrices above this many bytes: waic / loo never form them
POINTWISE_MAX_BYTES = 2 << 30
# waic / loo of a generated model: the scratch matrix of a block of datums (scratch_bytes=0)
GENERATED_DEFAULT_SCRATCH = 1 << 30
# psis_loo of a generated model with scratch_bytes=0: EXMC_PSIS_DEFAULT_SCRATCH of include/exmc_hip_psis.h
# (tests/test_codegen_pointwise.py holds the two together)
PSIS_DEFAULT_SCRATCH = 8 << 30


def n_data(compiled):
    n = compiled.L.exmc_hip_model_n_data(compiled.h)
    if n < 0:
        raise _lib.ExmcHipError("model comparison: the %s model has no per-datum terms; form its "
                                "pointwise log-likelihood on the host and use waic_from_pointwise / "
                                "loo_from_pointwise" % compiled.spec.name)
    return n


def _datum_order(compiled, N):
    """caller's index of the handle's datum k (radon: the kind sorts its observations by county)"""
    order = getattr(compiled.spec, "datum_order", None)
    return np.arange(N) if order is None else np.asarray(order, dtype=np.int64)


def datum_names(compiled):
    """names of the datums in the CALLER's order: the reference's obs keys where it has them
    (eight_schools "y_obs_j", simple ("y_obs", i)), else ("returns", t), ("y", i), ("radon", i);
    every index is 0-based, as the reference's {obs_id, idx} keys are"""
    N = n_data(compiled)
    kind = compiled.spec.kind
    if kind == CUSTOM:
        names = getattr(compiled.spec, "datum_names", None)
        if names is None or len(names) != N:
            raise _lib.ExmcHipError("model comparison: the plug-in of %s reports %d datums, its spec names %s"
                                    % (compiled.spec.name, N, "none" if names is None else len(names)))
        return list(names)
    if kind == EIGHT_SCHOOLS:
        return ["y_obs_%d" % j for j in range(N)]
    if kind == SIMPLE:
        return [("y_obs", i) for i in range(N)]
    if kind in (SV, SV_NCP):
        return [("returns", t) for t in range(N)]
    if kind == LOGISTIC:
        return [("y", i) for i in range(N)]
    if kind == RADON:
        return [("radon", i) for i in range(N)]
    raise _lib.ExmcHipError("model comparison: no datum names for kind %d" % kind)


def _check_samples(S, C):
    if S * C < 2:
        raise ValueError("model comparison needs at least 2 samples (the variance divides by n - 1)")


def pointwise_log_likelihood(compiled, draws, max_bytes=POINTWISE_MAX_BYTES):
    """pointwise_log_likelihood/2 (model_comparison.ex:19-50) per datum: a float64 device tensor
    ll [S][N][C] in the handle's datum order (radon: county-sorted; `names` says which is which) and the
    datum names. Refuses matrices above max_bytes: waic / loo reduce without forming them."""
    import torch
    N = n_data(compiled)
    x = _device_trace(compiled, draws)
    S, d, C = x.shape
    _check_samples(S, C)
    nbytes = S * N * C * 8
    if nbytes > max_bytes:
        raise ValueError("the pointwise matrix would take %.1f GB (limit %.1f GB): use waic() / loo(), which "
                         "reduce on the device without forming it" % (nbytes / 1e9, max_bytes / 1e9))
    ll = torch.empty((S, N, C), dtype=torch.float64, device=x.device)
    _ordered_after_torch(x)
    compiled.check(compiled.L.exmc_hip_pointwise_loglik(compiled.h, x.data_ptr(), S, d, C, ll.data_ptr()))
    torch.cuda.synchronize(x.device)
    names = datum_names(compiled)
    order = _datum_order(compiled, N)
    return ll, [names[k] for k in order]


def _generated_blocks(compiled, x, N, scratch_bytes, rows, reduce_block):
    """A generated model's datums in blocks of Nb = scratch_bytes / (8 S C), one at the least: the plug-in
    writes the block's matrix ll[S][nb][C] into scratch, reduce_block(main library, ll pointer, nb, out
    pointer) -- a *_from_ll entry point of libexmc_hip.so -- reduces it, its rows go to their columns."""
    import torch
    S, d, C = x.shape
    Nb = max(1, min(N, int(scratch_bytes) // (8 * S * C)))
    ll = torch.empty((S, Nb, C), dtype=torch.float64, device=x.device)
    blk = torch.empty((rows, Nb), dtype=torch.float64, device=x.device)
    out = np.empty((rows, N))
    main = _lib.load()
    _ordered_after_torch(x)
    for i0 in range(0, N, Nb):
        nb = min(Nb, N - i0)
        # (both calls return when their results are written: the scratch is free for the next block)
        compiled.check(compiled.L.exmc_hip_pointwise_loglik_range(compiled.h, x.data_ptr(), S, d, C, i0, nb,
                                                                  ll.data_ptr()))
        _lib.check(reduce_block(main, ll.data_ptr(), nb, blk.data_ptr()), main)
        out[:, i0:i0 + nb] = blk.cpu().numpy().reshape(-1)[:rows * nb].reshape(rows, nb)
    return out


def pointwise_stats(compiled, draws, scratch_bytes=0):
    """the per-datum statistics [4][N] (lppd, p_waic, elpd_loo, p_loo) in the CALLER's datum order.
    scratch_bytes: a generated model's block matrix (0: GENERATED_DEFAULT_SCRATCH); kinds reduce in one
    pass and take no scratch."""
    import torch
    N = n_data(compiled)
    x = _device_trace(compiled, draws)
    S, d, C = x.shape
    _check_samples(S, C)
    if compiled.spec.kind == CUSTOM:
        dev = x.device.index
        return _generated_blocks(compiled, x, N, scratch_bytes or GENERATED_DEFAULT_SCRATCH, 4,
                                 lambda L, ll, nb, out: L.exmc_hip_ic_stats_from_ll(dev, ll, S, nb, C, out))
    out = torch.empty((4, N), dtype=torch.float64, device=x.device)
    _ordered_after_torch(x)
    compiled.check(compiled.L.exmc_hip_ic_stats(compiled.h, x.data_ptr(), S, d, C, out.data_ptr()))
    torch.cuda.synchronize(x.device)
    st = out.cpu().numpy()
    res = np.empty_like(st)
    res[:, _datum_order(compiled, N)] = st
    return res


def _ll_tensor(ll, device=None):
    """a pointwise matrix [S][N][C] as a contiguous float64 device tensor"""
    import torch
    if isinstance(ll, torch.Tensor):
        if ll.dtype != torch.float64 or ll.dim() != 3 or not ll.is_cuda:
            raise ValueError("pointwise matrix must be a float64 CUDA tensor [S][N][C] or a host array")
        return ll.contiguous()
    a = np.asarray(ll, dtype=np.float64)
    if a.ndim != 3:
        raise ValueError("pointwise matrix must be [S][N][C]")
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0 if device is None else device))


def _stats_from_ll(ll, device=None):
    import torch
    x = _ll_tensor(ll, device)
    S, N, C = x.shape
    if N < 1:
        raise ValueError("No observations for WAIC / LOO computation")
    _check_samples(S, C)
    out = torch.empty((4, N), dtype=torch.float64, device=x.device)
    _ordered_after_torch(x)
    _lib.check(_lib.load().exmc_hip_ic_stats_from_ll(x.device.index, x.data_ptr(), S, N, C, out.data_ptr()))
    torch.cuda.synchronize(x.device)
    return out.cpu().numpy()


def psis_pointwise_stats(compiled, draws, scratch_bytes=0):
    """PSIS-LOO per datum, [3][N] (elpd_loo, p_loo, Pareto k) in the CALLER's datum order, and the number of
    pooled samples. The device walks the datums in blocks whose pointwise matrix fits scratch_bytes (0: the
    library's default, 8 GiB); the result does not depend on it."""
    import torch
    N = n_data(compiled)
    x = _device_trace(compiled, draws)
    S, d, C = x.shape
    _check_samples(S, C)
    if compiled.spec.kind == CUSTOM:
        dev = x.device.index
        st = _generated_blocks(compiled, x, N, scratch_bytes or PSIS_DEFAULT_SCRATCH, 3,
                               lambda L, ll, nb, out: L.exmc_hip_psis_stats_from_ll(dev, ll, S, nb, C, out))
        return st, S * C
    out = torch.empty((3, N), dtype=torch.float64, device=x.device)
    _ordered_after_torch(x)
    compiled.check(compiled.L.exmc_hip_psis_stats(compiled.h, x.data_ptr(), S, d, C, scratch_bytes, out.data_ptr()))
    torch.cuda.synchronize(x.device)
    st = out.cpu().numpy()
    res = np.empty_like(st)
    res[:, _datum_order(compiled, N)] = st
    return res, S * C


def _psis_from_ll(ll, device=None):
    import torch
    x = _ll_tensor(ll, device)
    S, N, C = x.shape
    if N < 1:
        raise ValueError("No observations for WAIC / LOO computation")
    _check_samples(S, C)
    out = torch.empty((3, N), dtype=torch.float64, device=x.device)
    _ordered_after_torch(x)
    _lib.check(_lib.load().exmc_hip_psis_stats_from_ll(x.device.index, x.data_ptr(), S, N, C, out.data_ptr()))
    torch.cuda.synchronize(x.device)
    return out.cpu().numpy(), S * C


def _variance(v):
    """variance (model_comparison.ex:260-269): mean = sum / n, then sum of squares / (n - 1)"""
    n = len(v)
    if n < 2:
        return 0.0
    mean = _lsum(v) / n
    return _lsum([(x - mean) * (x - mean) for x in v]) / (n - 1)


def _lsum(v):
    """Enum.sum: left to right from 0"""
    acc = 0
    for x in v:
        acc = acc + x
    return float(acc)


def waic_totals(lppd, p_waic):
    """waic/1's totals (model_comparison.ex:63-84) from the per-datum values, in datum order"""
    lppd, p_waic = [float(x) for x in lppd], [float(x) for x in p_waic]
    n = len(lppd)
    if n == 0:
        raise ValueError("No observations for WAIC computation")
    lp, pw = _lsum(lppd), _lsum(p_waic)
    elpd = lp - pw
    se = math.sqrt(n * _variance([a - b for a, b in zip(lppd, p_waic)])) if n > 1 else 0.0
    return dict(waic=-2 * elpd, elpd_waic=elpd, p_waic=pw, se=se, n_obs=n)


def loo_totals(elpd_loo, p_loo):
    """loo/1's totals (model_comparison.ex:95-114) from the per-datum values, in datum order"""
    elpd_loo, p_loo = [float(x) for x in elpd_loo], [float(x) for x in p_loo]
    n = len(elpd_loo)
    if n == 0:
        raise ValueError("No observations for LOO computation")
    e = _lsum(elpd_loo)
    se = math.sqrt(n * _variance(elpd_loo)) if n > 1 else 0.0
    return dict(loo=-2 * e, elpd_loo=e, p_loo=_lsum(p_loo), se=se, n_obs=n)


def _waic_result(st, names):
    r = waic_totals(st[0], st[1])
    r["pointwise"] = dict(names=list(names), lppd=st[0].copy(), p_waic=st[1].copy(), elpd_waic=st[0] - st[1])
    return r


def _loo_result(st, names):
    r = loo_totals(st[2], st[3])
    r["pointwise"] = dict(names=list(names), elpd_loo=st[2].copy(), p_loo=st[3].copy(), lppd=st[0].copy())
    return r


def waic(compiled, draws, scratch_bytes=0):
    """waic/1 over the model's datums; "pointwise" holds the per-datum arrays in the caller's order.
    scratch_bytes: see pointwise_stats (generated models only)"""
    return _waic_result(pointwise_stats(compiled, draws, scratch_bytes), datum_names(compiled))


def loo(compiled, draws, scratch_bytes=0):
    """loo/1 (plain importance-sampling LOO, loo_i_basic) over the model's datums"""
    return _loo_result(pointwise_stats(compiled, draws, scratch_bytes), datum_names(compiled))


def waic_from_pointwise(ll, names=None, device=None):
    """waic/1 from a pointwise matrix [S][N][C] (device tensor or host array)"""
    st = _stats_from_ll(ll, device)
    return _waic_result(st, names if names is not None else list(range(st.shape[1])))


def loo_from_pointwise(ll, names=None, device=None):
    st = _stats_from_ll(ll, device)
    return _loo_result(st, names if names is not None else list(range(st.shape[1])))


def k_threshold(n):
    """the sample-size dependent bound on a reliable Pareto k: min(1 - 1 / log10(n), 0.7)"""
    return min(1.0 - 1.0 / math.log10(n), 0.7)


def _psis_result(st, n, names):
    r = loo_totals(st[0], st[1])
    thr = k_threshold(n)
    r["pointwise"] = dict(names=list(names), elpd_loo=st[0].copy(), p_loo=st[1].copy(), pareto_k=st[2].copy())
    r["k_threshold"] = thr
    r["n_high_k"] = int(np.sum(~(st[2] <= thr)))   # NaN (a degenerate fit, a non-finite term) counts
    return r


def psis_loo(compiled, draws, scratch_bytes=0):
    """Pareto-smoothed importance-sampling LOO over the model's datums: loo's keys, the Pareto k of every
    datum in pointwise["pareto_k"] (+inf where the tail is too short to fit: nothing was smoothed),
    k_threshold and n_high_k, the number of datums whose k is not at or below it (above it, +inf, or NaN
    from a degenerate fit: nothing vouches for their elpd_loo_i). A datum with a non-finite term has NaN in all three."""
    st, n = psis_pointwise_stats(compiled, draws, scratch_bytes)
    return _psis_result(st, n, datum_names(compiled))


def psis_loo_from_pointwise(ll, names=None, device=None):
    """psis_loo from a pointwise matrix [S][N][C] (device tensor or host array)"""
    st, n = _psis_from_ll(ll, device)
    return _psis_result(st, n, names if names is not None else list(range(st.shape[1])))


def compare(results):
    """compare/1 (model_comparison.ex:127-150): [(label, result)] of waic or loo results, sorted by
    their IC (stable, best first), with d_elpd = elpd - the best model's elpd"""
    results = list(results)

    def ic(r):
        return r.get("waic", r.get("loo", 0))

    ranked = sorted(results, key=lambda lr: ic(lr[1]))
    best = ranked[0][1]
    best_elpd = best["elpd_waic"] if "elpd_waic" in best else best["elpd_loo"]
    out = []
    for label, r in ranked:
        elpd = r["elpd_waic"] if "elpd_waic" in r else r["elpd_loo"]
        out.append(dict(label=label, ic=r["waic"] if "waic" in r else r["loo"], elpd=elpd, se=r["se"],
                        d_elpd=elpd - best_elpd))
    return out
