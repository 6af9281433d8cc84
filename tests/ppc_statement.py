"""A plain-numpy statement of the posterior predictive checks (include/exmc_hip_ppc.h, DESIGN.md
"Posterior predictive checks"): what exmc_hip_ppc reduces the replicates to, written from the contract.
TEST INFRASTRUCTURE: the product never imports it.

It takes the replicate matrix yrep [S][N][C] (tests/predictive_statement.py's, or the device's own) and the
observed values y [N] in the handle's order. Every running sum is a real loop over the draws and the
chains (or the datums), vectorised over the other index only; numpy's elementwise + - * / on float64 round
once each, so the loops are the contract's arithmetic.

  per datum and block of 64 chains:   E, E2 (float64), n_lt, n_eq (int64)   -> sums, counts [B][N][2]
  per replicated data set (s, c):     T_mean, T_var, T_min, T_max           -> tstat [S][4][C]
  per chain and statistic:            draws with T_k >= T_obs_k             -> chain_counts [4][C] int32
  finished: mean, var, p_lt, p_eq, pit [N]; p_value [4]; t_obs [4]; m0"""
import numpy as np

import predictive_statement as PS

BLOCK = 64
STATS = ("mean", "var", "min", "max")


def observed(kind, blob):
    """y [N] in the handle's order, from the kind's data blob (exmc_amd/models.py)"""
    blob = np.asarray(blob, dtype=np.float64)
    N = PS.n_data(kind, blob)
    if kind == PS.SIMPLE:
        return blob.copy()
    if kind == PS.EIGHT_SCHOOLS:
        return blob[:8].copy()
    if kind in (PS.SV, PS.SV_NCP):
        return blob[:100].copy()
    if kind == PS.LOGISTIC:
        return blob[N * 20:].copy()
    if kind == PS.RADON:
        return blob[2 * 85 + 1 + N:].copy()
    raise ValueError("no datums for kind %r" % kind)


def observed_mean(y):
    s = np.float64(0.0)
    for v in y:
        s = s + v
    return s / np.float64(len(y))


def tstats(v, m0):
    """the four statistics of data sets v [N][...] about m0, the datums ascending: [4][...]"""
    v = np.asarray(v, dtype=np.float64)
    N = v.shape[0]
    Nd = np.float64(N)
    A = np.zeros(v.shape[1:])
    Bq = np.zeros(v.shape[1:])
    mn = np.full(v.shape[1:], np.inf)
    mx = np.full(v.shape[1:], -np.inf)
    with np.errstate(all="ignore"):
        for i in range(N):
            e = v[i] - m0
            A = A + e
            Bq = Bq + e * e
            mn = np.where(v[i] < mn, v[i], mn)
            mx = np.where(v[i] > mx, v[i], mx)
        return np.stack([m0 + A / Nd, (Bq - (A * A) / Nd) / (Nd - np.float64(1.0)), mn, mx])


def finish(sums, counts, chain_counts, y, S, Cn):
    """the host's finishing expressions: the blocks left to right, then mean, var, p_lt, p_eq, pit, p_value"""
    n = np.float64(S * Cn)
    N = sums.shape[1]
    E, E2 = np.zeros(N), np.zeros(N)
    n_lt, n_eq = np.zeros(N, np.int64), np.zeros(N, np.int64)
    with np.errstate(all="ignore"):
        for b in range(sums.shape[0]):
            E = E + sums[b, :, 0]
            E2 = E2 + sums[b, :, 1]
            n_lt = n_lt + counts[b, :, 0]
            n_eq = n_eq + counts[b, :, 1]
        mean = y + E / n
        var = (E2 - (E * E) / n) / (n - np.float64(1.0))
        p_lt = n_lt.astype(np.float64) / n
        p_eq = n_eq.astype(np.float64) / n
        pit = p_lt + 0.5 * p_eq
        p_value = chain_counts.astype(np.int64).sum(axis=1).astype(np.float64) / n
    return dict(mean=mean, var=var, p_lt=p_lt, p_eq=p_eq, pit=pit, p_value=p_value)


def run(yrep, y):
    """yrep [S][N][C], y [N] -> dict(sums [B][N][2], counts [B][N][2] int64, chain_counts [4][C] int32,
    tstat [S][4][C], t_obs [4], m0, and the finished numbers of finish())"""
    yrep = np.asarray(yrep, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    S, N, Cn = yrep.shape
    assert y.shape == (N,)
    B = (Cn + BLOCK - 1) // BLOCK
    sums = np.zeros((B, N, 2))
    counts = np.zeros((B, N, 2), np.int64)
    with np.errstate(all="ignore"):
        for b in range(B):
            E, E2 = np.zeros(N), np.zeros(N)
            n_lt, n_eq = np.zeros(N, np.int64), np.zeros(N, np.int64)
            for s in range(S):
                for c in range(BLOCK * b, min(BLOCK * b + BLOCK, Cn)):
                    v = yrep[s, :, c]
                    e = v - y
                    E = E + e
                    E2 = E2 + e * e
                    n_lt = n_lt + (v < y)
                    n_eq = n_eq + (v == y)
            sums[b, :, 0], sums[b, :, 1] = E, E2
            counts[b, :, 0], counts[b, :, 1] = n_lt, n_eq
    m0 = observed_mean(y)
    t_obs = tstats(y, m0)
    tstat = np.empty((S, 4, Cn))
    for s in range(S):
        tstat[s] = tstats(yrep[s], m0)
    with np.errstate(all="ignore"):
        chain_counts = (tstat >= t_obs[None, :, None]).sum(axis=0).astype(np.int32)     # NaN compares false
    out = dict(sums=sums, counts=counts, chain_counts=chain_counts, tstat=tstat, t_obs=t_obs, m0=float(m0))
    out.update(finish(sums, counts, chain_counts, y, S, Cn))
    return out


def run_sharded(yrep, y, cuts):
    """the statement on the chain shards [cuts[k], cuts[k + 1]), each cut a multiple of 64, joined as a
    caller joins them: the blocks and the chain columns side by side, then finished once"""
    yrep = np.asarray(yrep, dtype=np.float64)
    S, N, Cn = yrep.shape
    parts = [run(yrep[:, :, lo:hi], y) for lo, hi in zip(cuts[:-1], cuts[1:])]
    out = dict(sums=np.concatenate([p["sums"] for p in parts]), counts=np.concatenate([p["counts"] for p in parts]),
               chain_counts=np.concatenate([p["chain_counts"] for p in parts], axis=1),
               tstat=np.concatenate([p["tstat"] for p in parts], axis=2), t_obs=parts[0]["t_obs"], m0=parts[0]["m0"])
    out.update(finish(out["sums"], out["counts"], out["chain_counts"], np.asarray(y, dtype=np.float64), S, Cn))
    return out
