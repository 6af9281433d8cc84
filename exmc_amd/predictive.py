"""Host-side mirror of Exmc.Predictive (lib/exmc/predictive.ex: prior_samples :19-33, posterior_predictive
:44-63) over the device kernels.

    prior_samples(compiled, n, chains, seed=0)     -> {name: [C][n] numpy, x, q, yrep device tensors, names}:
                                                      the prior walk and the prior predictive replicates
    prior_samples_blocks(compiled, n, chains, block_draws, seed=0) -> yields (s0, dict of the block)
    posterior_predictive(compiled, draws, seed=0)  -> (yrep [S][N][C] device tensor, datum names)
    posterior_predictive_blocks(compiled, draws, block_draws, seed=0) -> yields (s0, yrep block)
    as_trace(yrep, names)                          -> {name: [C][S] numpy}, the reference's map
    ppc(compiled, draws, seed=0)                   -> posterior predictive checks of the same replicates,
                                                      reduced on the device without the matrix
    loo_pit(compiled, draws, seed=0)               -> PSIS-LOO-PIT: the same replicates under the smoothed
                                                      leave-one-out weights of PSIS-LOO
    loo_pit_from_pointwise(ll, yrep, y)            -> the same from matrices the caller made

The unit is the datum of a built-in kind, as in exmc_amd/model_comparison.py (include/exmc_hip_compare.h):
one y_i, one return r_t, in the handle's datum order (`names` says which is which). `draws` is the device
trace [S][d][C] or a host array [C][S][d]. Chain c draws its replicates with one generator seeded with
seed + 7919 (chain_lo + c), walking the draws and within a draw the datums; the replicates are
bit-identical to the statement of predictive.ex and its sample/2 callbacks (DESIGN.md "Posterior
predictive", which states the deviations). The work of a chain is serial by contract, so the throughput
grows with the number of chains. Generated models are not supported. No CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from .diagnostics import _device_trace, _ordered_after_torch
from .model_comparison import _check_samples, _datum_order, _ll_tensor, datum_names, k_threshold, n_data

# posterior_predictive refuses matrices above this many bytes: posterior_predictive_blocks walks the draws
PREDICTIVE_MAX_BYTES = 2 << 30


def _names(compiled, N):
    names = datum_names(compiled)
    return [names[k] for k in _datum_order(compiled, N)]


def _call(compiled, x, s0, ns, seed, chain_lo, resume, state, out):
    S, d, Cn = x.shape
    opts = _lib.PredictiveOpts(int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_lo), 1 if resume else 0)
    compiled.check(compiled.L.exmc_hip_posterior_predictive(
        compiled.h, opts, x.data_ptr() + s0 * d * Cn * 8, ns, d, Cn,
        None if state is None else state.data_ptr(), out.data_ptr()))


def posterior_predictive(compiled, draws, seed=0, chain_lo=0, max_bytes=PREDICTIVE_MAX_BYTES):
    """Replicates of every datum at every draw of every chain: a float64 device tensor yrep [S][N][C]
    in the handle's datum order, and the datum names in that order. Refuses a matrix above max_bytes:
    posterior_predictive_blocks yields it a block of draws at a time."""
    import torch
    N = n_data(compiled)
    x = _device_trace(compiled, draws)
    S, d, Cn = x.shape
    nbytes = S * N * Cn * 8
    if nbytes > max_bytes:
        raise ValueError("the replicate matrix would take %.1f GB (limit %.1f GB): use "
                         "posterior_predictive_blocks, which yields it a block of draws at a time"
                         % (nbytes / 1e9, max_bytes / 1e9))
    yrep = torch.empty((S, N, Cn), dtype=torch.float64, device=x.device)
    _ordered_after_torch(x)
    _call(compiled, x, 0, S, seed, chain_lo, False, None, yrep)
    torch.cuda.synchronize(x.device)
    return yrep, _names(compiled, N)


def posterior_predictive_blocks(compiled, draws, block_draws, seed=0, chain_lo=0):
    """A generator of (s0, yrep_block [ns][N][C]) over the draws in blocks of block_draws, the chains'
    generators carried from block to block on the device: the blocks joined are posterior_predictive's
    matrix, bit for bit. Every block is a tensor of its own; the last may be shorter."""
    import torch
    if int(block_draws) < 1:
        raise ValueError("block_draws must be >= 1")
    N = n_data(compiled)
    x = _device_trace(compiled, draws)
    S, d, Cn = x.shape
    state = torch.zeros((2, Cn), dtype=torch.int64, device=x.device)   # the bits of the uint64 [2][C]
    _ordered_after_torch(x)
    for s0 in range(0, S, int(block_draws)):
        ns = min(int(block_draws), S - s0)
        out = torch.empty((ns, N, Cn), dtype=torch.float64, device=x.device)
        _ordered_after_torch(out)
        _call(compiled, x, s0, ns, seed, chain_lo, s0 > 0, state, out)
        torch.cuda.synchronize(x.device)
        yield s0, out


def as_trace(yrep, names):
    """{name: [C][S]}: the reference's %{obs_name => {n}} per chain, from yrep [S][N][C]"""
    a = yrep.cpu().numpy() if hasattr(yrep, "cpu") else np.asarray(yrep)
    if a.ndim != 3 or a.shape[1] != len(names):
        raise ValueError("yrep must be [S][N][C] with one name per datum")
    return {name: np.ascontiguousarray(a[:, i, :].T) for i, name in enumerate(names)}


# ---- prior and prior predictive samples (include/exmc_hip_prior.h, DESIGN.md "Prior predictive") ---------
def _prior_call(compiled, n, Cn, seed, chain_lo, resume, state, x, q, yrep):
    opts = _lib.PredictiveOpts(int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_lo), 1 if resume else 0)
    compiled.check(compiled.L.exmc_hip_prior_samples(
        compiled.h, opts, int(n), int(Cn), None if state is None else state.data_ptr(), x.data_ptr(), q.data_ptr(),
        None if yrep is None else yrep.data_ptr()))


def _prior_result(compiled, x, q, yrep, N):
    xs = x.cpu().numpy()
    out = {name: np.ascontiguousarray(xs[:, j, :].T) for j, name in enumerate(compiled.spec.var_names)}
    out.update(x=x, q=q, yrep=yrep, names=_names(compiled, N) if yrep is not None else [])
    return out


def _prior_bytes(n, d, N, Cn, replicates):
    return n * (2 * d + (N if replicates else 0)) * Cn * 8


def prior_samples(compiled, n, chains, seed=0, chain_lo=0, replicates=True, max_bytes=PREDICTIVE_MAX_BYTES):
    """Exmc.Predictive.prior_samples (lib/exmc/predictive.ex:19-33) of a built-in kind: n draws of every free
    variable from its prior in each of `chains` chains, chain c with one generator seeded with seed + 7919
    (chain_lo + c), the variables of a draw in the reference's Kahn order, and with replicates=True the
    prior predictive replicates of every datum after them. A dict: per variable name a numpy [C][n] of
    constrained values (the reference's map, per chain); `x` and `q`, the float64 device tensors [n][d][C]
    of the constrained values and of the unconstrained position in kernel order (q is a trace for
    posterior_predictive, ppc and the pointwise terms); `yrep`, the device tensor [n][N][C] in the handle's
    datum order, or None; `names`, the datum names in that order. With replicates=False no datum is drawn
    and the generators do not advance for them. Refuses results above max_bytes: prior_samples_blocks
    yields them a block of draws at a time."""
    import torch
    n, Cn = int(n), int(chains)
    N, d = n_data(compiled), compiled.d
    if n >= 1 and Cn >= 1 and _prior_bytes(n, d, N, Cn, replicates) > max_bytes:
        raise ValueError("the prior samples would take %.1f GB (limit %.1f GB): use prior_samples_blocks, "
                         "which yields them a block of draws at a time"
                         % (_prior_bytes(n, d, N, Cn, replicates) / 1e9, max_bytes / 1e9))
    dev = torch.device("cuda", compiled.device)
    x = torch.empty((max(n, 0), d, max(Cn, 0)), dtype=torch.float64, device=dev)
    q = torch.empty_like(x)
    yrep = torch.empty((max(n, 0), N, max(Cn, 0)), dtype=torch.float64, device=dev) if replicates else None
    _ordered_after_torch(x)
    _prior_call(compiled, n, Cn, seed, chain_lo, False, None, x, q, yrep)
    torch.cuda.synchronize(dev)
    return _prior_result(compiled, x, q, yrep, N)


def prior_samples_blocks(compiled, n, chains, block_draws, seed=0, chain_lo=0, replicates=True):
    """A generator of (s0, dict) over the n draws in blocks of block_draws, the chains' generators carried
    from block to block on the device: the blocks joined are prior_samples' result, bit for bit. Every
    block's dict is prior_samples' of its draws, with tensors of its own; the last may be shorter."""
    import torch
    if int(block_draws) < 1:
        raise ValueError("block_draws must be >= 1")
    n, Cn = int(n), int(chains)
    N, d = n_data(compiled), compiled.d
    dev = torch.device("cuda", compiled.device)
    state = torch.zeros((2, max(Cn, 0)), dtype=torch.int64, device=dev)   # the bits of the uint64 [2][C]
    for s0 in range(0, n, int(block_draws)):
        ns = min(int(block_draws), n - s0)
        x = torch.empty((ns, d, Cn), dtype=torch.float64, device=dev)
        q = torch.empty_like(x)
        yrep = torch.empty((ns, N, Cn), dtype=torch.float64, device=dev) if replicates else None
        _ordered_after_torch(state)
        _prior_call(compiled, ns, Cn, seed, chain_lo, s0 > 0, state, x, q, yrep)
        torch.cuda.synchronize(dev)
        yield s0, _prior_result(compiled, x, q, yrep, N)


PPC_STATS = ("mean", "var", "min", "max")


def ppc(compiled, draws, seed=0, chain_lo=0, tstat=False):
    """Posterior predictive checks (include/exmc_hip_ppc.h, DESIGN.md "Posterior predictive checks"): the
    replicates of posterior_predictive at the same seed and chain_lo, reduced in the kernel that draws
    them; the matrix is never formed. A dict: `names` (the datums in the handle's order, as
    posterior_predictive returns them); per datum [N] numpy `mean` and `var` of its replicates, `p_lt` and
    `p_eq` (the share of replicates below and equal to the observation) and `pit` = p_lt + 0.5 p_eq; per
    test statistic of a whole data set (PPC_STATS) `t_obs` (the observed value) and `p_value` (the share
    of replicated data sets at or above it); with tstat=True also `tstat`, the device tensor [S][4][C] of
    every replicated data set's statistics."""
    import torch
    N = n_data(compiled)
    x = _device_trace(compiled, draws)
    S, d, Cn = x.shape
    B = (Cn + _lib.PPC_BLOCK - 1) // _lib.PPC_BLOCK
    sums = torch.empty((B, N, 2), dtype=torch.float64, device=x.device)
    counts = torch.empty((B, N, 2), dtype=torch.int64, device=x.device)
    chain_counts = torch.empty((4, Cn), dtype=torch.int32, device=x.device)
    ts = torch.empty((S, 4, Cn), dtype=torch.float64, device=x.device) if tstat else None
    t_obs, m0, y = np.zeros(4), np.zeros(1), np.zeros(N)
    dp = C.POINTER(C.c_double)
    opts = _lib.PredictiveOpts(int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_lo), 0)
    _ordered_after_torch(x)
    compiled.check(compiled.L.exmc_hip_ppc(
        compiled.h, opts, x.data_ptr(), S, d, Cn, sums.data_ptr(), counts.data_ptr(), chain_counts.data_ptr(),
        None if ts is None else ts.data_ptr(), t_obs.ctypes.data_as(dp), m0.ctypes.data_as(dp), y.ctypes.data_as(dp)))
    torch.cuda.synchronize(x.device)
    sums, counts, chain_counts = sums.cpu().numpy(), counts.cpu().numpy(), chain_counts.cpu().numpy()
    # the finishing expressions of include/exmc_hip_ppc.h, as exmc_hip_ppc_host writes them
    n = np.float64(S * Cn)
    E, E2 = np.zeros(N), np.zeros(N)
    n_lt, n_eq = np.zeros(N, np.int64), np.zeros(N, np.int64)
    with np.errstate(all="ignore"):
        for b in range(B):
            E = E + sums[b, :, 0]
            E2 = E2 + sums[b, :, 1]
            n_lt = n_lt + counts[b, :, 0]
            n_eq = n_eq + counts[b, :, 1]
        p_lt, p_eq = n_lt.astype(np.float64) / n, n_eq.astype(np.float64) / n
        out = dict(names=_names(compiled, N), mean=y + E / n, var=(E2 - (E * E) / n) / (n - np.float64(1.0)),
                   p_lt=p_lt, p_eq=p_eq, pit=p_lt + 0.5 * p_eq)
        above = chain_counts.astype(np.int64).sum(axis=1)
        out["t_obs"] = {k: float(t_obs[i]) for i, k in enumerate(PPC_STATS)}
        out["p_value"] = {k: float(np.float64(above[i]) / n) for i, k in enumerate(PPC_STATS)}
    if tstat:
        out["tstat"] = ts
    return out


def _loo_pit_result(out, n, names):
    """the rows of include/exmc_hip_loo_pit.h as a dict, k_threshold and n_high_k as psis_loo forms them"""
    r = dict(names=list(names), **{k: out[i].copy() for i, k in enumerate(_lib.LOO_PIT_ROWS)})
    thr = k_threshold(n)
    r["k_threshold"] = thr
    r["n_high_k"] = int(np.sum(~(out[3] <= thr)))   # NaN (a degenerate fit, a non-finite term) counts
    return r


def loo_pit(compiled, draws, seed=0, chain_lo=0, scratch_bytes=0):
    """PSIS-LOO-PIT (include/exmc_hip_loo_pit.h, DESIGN.md "LOO-PIT"): the probability integral transform
    of every observation under its leave-one-out predictive distribution. The replicates are those of
    posterior_predictive at the same seed and chain_lo, each weighted with the Pareto-smoothed importance
    weight of its sample, as psis_loo forms it; neither matrix is kept. A dict: `names` (the datums in the
    handle's order, as posterior_predictive returns them); per datum [N] numpy `p_lt` and `p_eq` (the
    weighted share of replicates below and equal to the observation), `pit` = p_lt + 0.5 p_eq and `k`, the
    datum's Pareto k (+inf where nothing was smoothed); `k_threshold` and `n_high_k`, the number of datums
    whose k is not at or below it: nothing vouches for their PIT. A datum with a non-finite term has NaN in
    all four. The weights pool all chains of the call: there is no sharding, chain_lo only seeds the
    generators. scratch_bytes bounds the pointwise matrix of the first pass (0: the library's default,
    8 GiB); the result does not depend on it."""
    import torch
    N = n_data(compiled)
    x = _device_trace(compiled, draws)
    S, d, Cn = x.shape
    out = torch.empty((len(_lib.LOO_PIT_ROWS), N), dtype=torch.float64, device=x.device)
    opts = _lib.PredictiveOpts(int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_lo), 0)
    _ordered_after_torch(x)
    compiled.check(compiled.L.exmc_hip_loo_pit(compiled.h, opts, x.data_ptr(), S, d, Cn, int(scratch_bytes),
                                               out.data_ptr()))
    torch.cuda.synchronize(x.device)
    return _loo_pit_result(out.cpu().numpy(), S * Cn, _names(compiled, N))


def loo_pit_from_pointwise(ll, yrep, y, names=None, device=None):
    """loo_pit from a pointwise matrix ll [S][N][C], the replicates yrep [S][N][C] and the observations
    y [N] (device tensors or host arrays): for models whose terms and replicates the caller made"""
    import torch
    x = _ll_tensor(ll, device)
    v = _ll_tensor(yrep, x.device.index)
    S, N, Cn = x.shape
    if N < 1:
        raise ValueError("No observations for LOO-PIT computation")
    if tuple(v.shape) != (S, N, Cn) or v.device != x.device:
        raise ValueError("yrep must be [S][N][C] like ll, on the same device")
    _check_samples(S, Cn)
    if isinstance(y, torch.Tensor):
        yd = y.to(device=x.device, dtype=torch.float64).contiguous()
    else:
        yd = torch.from_numpy(np.ascontiguousarray(np.asarray(y, dtype=np.float64))).to(x.device)
    if tuple(yd.shape) != (N,):
        raise ValueError("y must hold one observation per datum")
    out = torch.empty((len(_lib.LOO_PIT_ROWS), N), dtype=torch.float64, device=x.device)
    _ordered_after_torch(x)
    _lib.check(_lib.load().exmc_hip_loo_pit_from_ll(x.device.index, x.data_ptr(), v.data_ptr(), yd.data_ptr(), S, N, Cn,
                                                    out.data_ptr()))
    torch.cuda.synchronize(x.device)
    return _loo_pit_result(out.cpu().numpy(), S * Cn, names if names is not None else list(range(N)))
