"""Time the posterior predictive checks (exmc_hip_ppc) at the sizes of the BASELINE runs, eight_schools 4096
chains x 1000 draws and logistic 8192 chains x 1000 draws, against today's route to the same numbers,
measured in the same process:

  ppc         exmc_hip_ppc over the whole trace in one call (no replicate matrix), with and without tstat
  predictive  predictive_kernel alone at the same configuration (exmc_hip_posterior_predictive in blocks
              of --block draws into one reused buffer, the generators carried on the device)
  blocks      exmc_amd.predictive.posterior_predictive_blocks in blocks of --block draws, every block
              reduced with torch to the same per-datum sums and counts and per-chain counts

Without --one this is the driver: every config is a step of its own, a child process under its own
`timeout`, chained; the first that fails ends the run with its exit status. With --one CONFIG it is one
step. Kernel milliseconds come from the handle's HIP events (exmc_hip_last_kernel_ms, which enclose the
launch only): --warmup passes are thrown away, --reps passes are kept, median (min .. max). The blocks
route is wall clock between device synchronisations (its kernels are torch's as well). Peak device memory
is torch's allocator's (max_memory_allocated), reset before each route; the trace itself is part of both
peaks. The trace is synthetic (0.1 * normal around the kind's default initial point). One JSON line per
config."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _configs():
    from exmc_amd import models
    # name: (spec factory, chains, draws, draws per block of the matrix routes)
    return {"eight_schools": (models.eight_schools, 4096, 1000, 50),
            "logistic": (models.logistic, 8192, 1000, 50)}


def _spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3))


def one(a):
    import ctypes as C

    import torch

    from exmc_amd import _lib, sampler
    from exmc_amd import predictive as PP
    make, Cn, S, block = _configs()[a.one]
    Cn, S, block = a.chains or Cn, a.draws or S, a.block or block
    spec = make()
    comp = sampler.compile(spec)
    L, d = comp.L, comp.d
    N = L.exmc_hip_model_n_data(comp.h)
    B = (Cn + _lib.PPC_BLOCK - 1) // _lib.PPC_BLOCK
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    q0 = torch.from_numpy(np.asarray(spec.to_unconstrained(spec.default_init), dtype=np.float64)).to(dev)
    x = q0[None, :, None] + 0.1 * torch.randn((S, d, Cn), dtype=torch.float64, device=dev, generator=gen)
    del gen
    torch.cuda.synchronize()
    dp = C.POINTER(C.c_double)
    t_obs, m0, y = np.zeros(4), np.zeros(1), np.zeros(N)

    def timed(run_pass):
        for _ in range(a.warmup):
            run_pass()
        return _spread([run_pass() for _ in range(a.reps)])

    # ---- ppc: one call over the whole trace ----
    def ppc_route(with_tstat):
        torch.cuda.reset_peak_memory_stats(dev)
        sums = torch.empty((B, N, 2), dtype=torch.float64, device=dev)
        counts = torch.empty((B, N, 2), dtype=torch.int64, device=dev)
        cc = torch.empty((4, Cn), dtype=torch.int32, device=dev)
        ts = torch.empty((S, 4, Cn), dtype=torch.float64, device=dev) if with_tstat else None
        torch.cuda.synchronize()

        def run_pass():
            comp.check(L.exmc_hip_ppc(comp.h, _lib.PredictiveOpts(1, 0, 0), x.data_ptr(), S, d, Cn, sums.data_ptr(),
                                      counts.data_ptr(), cc.data_ptr(), None if ts is None else ts.data_ptr(),
                                      t_obs.ctypes.data_as(dp), m0.ctypes.data_as(dp), y.ctypes.data_as(dp)))
            return comp.last_kernel_ms
        ms = timed(run_pass)
        return ms, torch.cuda.max_memory_allocated(dev), (sums.cpu(), counts.cpu(), cc.cpu())

    ppc_ms, ppc_peak, ppc_out = ppc_route(False)
    ppc_ts_ms, ppc_ts_peak, _ = ppc_route(True)

    # ---- predictive_kernel alone, blocks of draws into one reused buffer ----
    torch.cuda.reset_peak_memory_stats(dev)
    out = torch.empty((min(block, S), N, Cn), dtype=torch.float64, device=dev)
    state = torch.zeros((2, Cn), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def predictive_pass():
        ms = 0.0
        for s0 in range(0, S, block):
            ns = min(block, S - s0)
            comp.check(L.exmc_hip_posterior_predictive(
                comp.h, _lib.PredictiveOpts(1, 0, 1 if s0 else 0), x.data_ptr() + s0 * d * Cn * 8, ns, d, Cn,
                state.data_ptr(), out.data_ptr()))
            ms += comp.last_kernel_ms
        return ms
    pred_ms = timed(predictive_pass)
    del out, state

    # ---- today's route: the blocks of the matrix, each reduced with torch ----
    torch.cuda.reset_peak_memory_stats(dev)
    yd = torch.from_numpy(y).to(dev)
    t_obs_d = torch.from_numpy(t_obs).to(dev)
    kept = {}

    def blocks_pass():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E = torch.zeros(N, dtype=torch.float64, device=dev)
        E2 = torch.zeros(N, dtype=torch.float64, device=dev)
        n_lt = torch.zeros(N, dtype=torch.int64, device=dev)
        n_eq = torch.zeros(N, dtype=torch.int64, device=dev)
        above = torch.zeros((4, Cn), dtype=torch.int64, device=dev)
        for _, blk in PP.posterior_predictive_blocks(comp, x, block, seed=1):
            e = blk - yd[None, :, None]
            E += e.sum(dim=(0, 2))
            E2 += (e * e).sum(dim=(0, 2))
            n_lt += (blk < yd[None, :, None]).sum(dim=(0, 2))
            n_eq += (blk == yd[None, :, None]).sum(dim=(0, 2))
            T = torch.stack([blk.mean(dim=1), blk.var(dim=1, unbiased=True), blk.amin(dim=1), blk.amax(dim=1)], dim=1)
            above += (T >= t_obs_d[None, :, None]).sum(dim=0)
            del e, T, blk
        torch.cuda.synchronize()
        kept.update(n_lt=n_lt.cpu(), n_eq=n_eq.cpu(), above=above.cpu())
        return (time.perf_counter() - t0) * 1e3
    blocks_ms = timed(blocks_pass)
    blocks_peak = torch.cuda.max_memory_allocated(dev)
    # the two routes reduce the same replicates: the integer results agree exactly
    counts = ppc_out[1].sum(dim=0)
    same_counts = bool((counts[:, 0] == kept["n_lt"]).all() and (counts[:, 1] == kept["n_eq"]).all()
                       and (ppc_out[2][2:].to(torch.int64) == kept["above"][2:]).all())

    print(json.dumps(dict(
        config=a.one, chains=Cn, draws=S, n_data=N, d=d, block_draws=block, reps=a.reps, warmup=a.warmup,
        replicates=S * N * Cn, trace_bytes=S * d * Cn * 8, yrep_bytes=S * N * Cn * 8,
        ppc_kernel_ms=ppc_ms, ppc_kernel_with_tstat_ms=ppc_ts_ms, predictive_kernel_ms=pred_ms,
        ratio_ppc_to_predictive=round(ppc_ms["median"] / pred_ms["median"], 3),
        blocks_route_wall_ms=blocks_ms,
        peak_bytes=dict(ppc=ppc_peak, ppc_with_tstat=ppc_ts_peak, blocks_route=blocks_peak),
        counts_equal_between_routes=same_counts)), flush=True)
    comp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="eight_schools,logistic")
    ap.add_argument("--one", default=None, help="run this one config in this process")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chains", type=int, default=0, help="0: the config's")
    ap.add_argument("--draws", type=int, default=0)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each config's step may take")
    a = ap.parse_args()
    if a.one:
        return one(a)
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--chains", str(a.chains), "--draws", str(a.draws),
               "--block", str(a.block)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("ppc_time: step %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
