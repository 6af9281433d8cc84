"""Time PSIS-LOO-PIT (exmc_hip_loo_pit) beside the two calls whose work it joins, on the same trace in the
same process: exmc_hip_psis_stats (the pointwise matrix, the tails, the weights' log-sum-exps) and
exmc_hip_ppc (the walk that draws and transposes every replicate). The fused call does the tail pass of
the first and the walk of the second, so the sum of the two is what it is held against.

  eight_schools  4096 chains x 1000 draws
  sv_ncp         2048 chains x 1000 draws
  logistic       8192 chains x  200 draws

Without --one this is the driver: every config is a step of its own, a child process under its own
`timeout`, chained; the first that fails ends the run with its exit status. With --one CONFIG it is one
step. Kernel milliseconds come from the handle's HIP events (exmc_hip_last_kernel_ms, which enclose the
launches only). The three calls alternate: --warmup rounds of (loo_pit, psis, ppc) are thrown away, --reps
rounds are kept, median (min .. max) per call. Peak device memory is torch's allocator's for the trace and
the outputs; the library's own scratch (hipMalloc) is stated from the contract's formulas. The trace is
synthetic (0.1 * normal around the kind's default initial point). One JSON line per config."""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _configs():
    from exmc_amd import models
    # name: (spec factory, chains, draws)
    return {"eight_schools": (models.eight_schools, 4096, 1000),
            "sv_ncp": (lambda: models.sv_ncp(models.sv_returns()), 2048, 1000),
            "logistic": (models.logistic, 8192, 200)}


def _spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3))


def one(a):
    import torch

    from exmc_amd import _lib, sampler
    make, Cn, S = _configs()[a.one]
    Cn, S = a.chains or Cn, a.draws or S
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
    pit = torch.empty((4, N), dtype=torch.float64, device=dev)
    psis = torch.empty((3, N), dtype=torch.float64, device=dev)
    sums = torch.empty((B, N, 2), dtype=torch.float64, device=dev)
    counts = torch.empty((B, N, 2), dtype=torch.int64, device=dev)
    cc = torch.empty((4, Cn), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    dp = C.POINTER(C.c_double)
    t_obs, m0 = np.zeros(4), np.zeros(1)
    opts = _lib.PredictiveOpts(1, 0, 0)

    def loo_pit_pass():
        comp.check(L.exmc_hip_loo_pit(comp.h, opts, x.data_ptr(), S, d, Cn, 0, pit.data_ptr()))
        return comp.last_kernel_ms

    def psis_pass():
        comp.check(L.exmc_hip_psis_stats(comp.h, x.data_ptr(), S, d, Cn, 0, psis.data_ptr()))
        return comp.last_kernel_ms

    def ppc_pass():
        comp.check(L.exmc_hip_ppc(comp.h, opts, x.data_ptr(), S, d, Cn, sums.data_ptr(), counts.data_ptr(),
                                  cc.data_ptr(), None, t_obs.ctypes.data_as(dp), m0.ctypes.data_as(dp), None))
        return comp.last_kernel_ms

    passes = dict(loo_pit=loo_pit_pass, psis_stats=psis_pass, ppc=ppc_pass)
    ms = {k: [] for k in passes}
    for r in range(a.warmup + a.reps):
        for k, f in passes.items():       # alternating
            t = f()
            if r >= a.warmup:
                ms[k].append(t)
    out = {k: _spread(v) for k, v in ms.items()}
    both = out["psis_stats"]["median"] + out["ppc"]["median"]
    pit_h, psis_h = pit.cpu().numpy(), psis.cpu().numpy()
    n = S * Cn
    M = int(math.ceil(min(n / 5.0, 3.0 * math.sqrt(n))))
    P = 1 << max(M - 1, 0).bit_length()
    print(json.dumps(dict(
        config=a.one, chains=Cn, draws=S, n_data=N, d=d, reps=a.reps, warmup=a.warmup, samples=n, tail_max=M,
        trace_bytes=S * d * Cn * 8, tail_table_bytes=N * (20 * P + 48), state_bytes=B * N * 32,
        loo_pit_ms=out["loo_pit"], psis_stats_ms=out["psis_stats"], ppc_ms=out["ppc"],
        psis_plus_ppc_ms=round(both, 3), ratio_loo_pit_to_sum=round(out["loo_pit"]["median"] / both, 3),
        k_equals_psis=bool(pit_h[3].tobytes() == psis_h[2].tobytes()),
        pit_finite=bool(np.isfinite(pit_h[:3]).all()), pit_min=float(pit_h[2].min()), pit_max=float(pit_h[2].max()))),
        flush=True)
    comp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="eight_schools,sv_ncp,logistic")
    ap.add_argument("--one", default=None, help="run this one config in this process")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chains", type=int, default=0, help="0: the config's")
    ap.add_argument("--draws", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each config's step may take")
    a = ap.parse_args()
    if a.one:
        return one(a)
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--chains", str(a.chains), "--draws", str(a.draws)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("loo_pit_time: step %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
