"""Time the convergence diagnostics across chains (exmc_hip_convergence) on synthetic AR(1) traces at the
sizes of the BASELINE runs, eight_schools 4096 chains x 1000 draws x 10 dimensions and sv 2048 x 1000 x 102,
and beside it today's per-series diagnostics on the same trace, exmc_hip_ess_bulk plus exmc_hip_rhat.

Without --one this is the driver: every config is a step of its own, a child process under its own
`timeout`, chained; the first that fails ends the run with its exit status. With --one CONFIG it is one
step. Kernel milliseconds come from the handle's HIP events (exmc_hip_last_kernel_ms): --warmup passes are
thrown away, --reps passes are kept, median (min .. max). The trace is AR(1) with a correlation drawn per
(dimension, chain) from U(0, 0.9), made on the device. One JSON line per config."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (chains, draws, dimensions)
CONFIGS = {"eight_schools": (4096, 1000, 10), "sv": (2048, 1000, 102)}


def _spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3))


def one(a):
    import torch

    from exmc_amd import models, sampler
    Cn, S, d = CONFIGS[a.one]
    Cn, S, d = a.chains or Cn, a.draws or S, a.dims or d
    comp = sampler.compile(models.eight_schools())   # the calls are model-free: any handle serves
    L = comp.L
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    phi = 0.9 * torch.rand((d, Cn), dtype=torch.float64, device=dev, generator=gen)
    x = torch.empty((S, d, Cn), dtype=torch.float64, device=dev)
    x[0] = torch.randn((d, Cn), dtype=torch.float64, device=dev, generator=gen)
    for i in range(1, S):
        x[i] = phi * x[i - 1] + torch.randn((d, Cn), dtype=torch.float64, device=dev, generator=gen)
    out = torch.empty((6, d), dtype=torch.float64, device=dev)
    essb = torch.empty((d, Cn), dtype=torch.float64, device=dev)
    rh = torch.empty((d,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def timed(run_pass):
        for _ in range(a.warmup):
            run_pass()
        return _spread([run_pass() for _ in range(a.reps)])

    def convergence_pass():
        comp.check(L.exmc_hip_convergence(comp.h, x.data_ptr(), S, d, Cn, a.scratch, out.data_ptr()))
        return comp.last_kernel_ms

    def per_series_pass():
        comp.check(L.exmc_hip_ess_bulk(comp.h, x.data_ptr(), S, d, Cn, essb.data_ptr()))
        ms = comp.last_kernel_ms
        comp.check(L.exmc_hip_rhat(comp.h, x.data_ptr(), S, d, Cn, rh.data_ptr()))
        return ms + comp.last_kernel_ms

    conv_ms = timed(convergence_pass)
    series_ms = timed(per_series_pass)
    torch.cuda.synchronize()
    rows = out.cpu().numpy()
    print(json.dumps(dict(
        config=a.one, chains=Cn, draws=S, d=d, pooled_per_dimension=2 * Cn * (S // 2), reps=a.reps, warmup=a.warmup,
        scratch_bytes=a.scratch, trace_bytes=S * d * Cn * 8, convergence_kernel_ms=conv_ms,
        ess_bulk_plus_rhat_kernel_ms=series_ms,
        rhat_bulk_max=float(rows[0].max()), rhat_tail_max=float(rows[1].max()), ess_bulk_min=float(rows[2].min()),
        ess_tail_min=float(rows[3].min()), per_series_ess_bulk_sum_min=float(essb.sum(dim=1).min()))), flush=True)
    comp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="eight_schools,sv")
    ap.add_argument("--one", default=None, help="run this one config in this process")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chains", type=int, default=0, help="0: the config's")
    ap.add_argument("--draws", type=int, default=0)
    ap.add_argument("--dims", type=int, default=0)
    ap.add_argument("--scratch", type=int, default=0, help="scratch_bytes of the call (0: the library's default)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each config's step may take")
    a = ap.parse_args()
    if a.one:
        return one(a)
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--chains", str(a.chains), "--draws", str(a.draws),
               "--dims", str(a.dims), "--scratch", str(a.scratch)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("convergence_time: step %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
