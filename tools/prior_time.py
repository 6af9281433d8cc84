"""Time prior and prior predictive sampling (exmc_hip_prior_samples) at the sizes of the BASELINE runs:
eight_schools 4096 chains x 1000 draws in one call, and logistic 8192 chains x 1000 draws in blocks of draws
that reuse one set of output buffers (its replicates alone would be 32 GB), the generators carried from block
to block on the device.

Without --one this is the driver: every config is a step of its own, a child process under its own
`timeout`, chained; the first that fails ends the run with its exit status. With --one CONFIG it is one
step. Kernel milliseconds come from the handle's HIP events (exmc_hip_last_kernel_ms, which enclose the
launch only): --warmup passes are thrown away, --reps passes are kept, and the median and the spread (min ..
max) of a pass's total are printed, with the variates (variables and replicates) per second that makes.
--no-replicates times the walk over the free variables alone. One JSON line per config."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _configs():
    from exmc_amd import models
    # name: (spec factory, chains, draws, draws per block)
    return {"eight_schools": (models.eight_schools, 4096, 1000, 1000),
            "logistic": (models.logistic, 8192, 1000, 50)}


def one(a):
    import torch

    from exmc_amd import _lib, sampler
    make, Cn, S, block = _configs()[a.one]
    Cn, S, block = a.chains or Cn, a.draws or S, a.block or block
    comp = sampler.compile(make())
    L, d = comp.L, comp.d
    N = L.exmc_hip_model_n_data(comp.h)
    dev = torch.device("cuda", 0)
    nb = min(block, S)
    x = torch.empty((nb, d, Cn), dtype=torch.float64, device=dev)
    q = torch.empty_like(x)
    out = None if a.no_replicates else torch.empty((nb, N, Cn), dtype=torch.float64, device=dev)
    state = torch.zeros((2, Cn), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def one_pass():
        ms = []
        for s0 in range(0, S, block):
            ns = min(block, S - s0)
            comp.check(L.exmc_hip_prior_samples(
                comp.h, _lib.PredictiveOpts(1, 0, 1 if s0 else 0), ns, Cn, state.data_ptr(), x.data_ptr(), q.data_ptr(),
                None if out is None else out.data_ptr()))
            ms.append(comp.last_kernel_ms)
        return ms

    for _ in range(a.warmup):
        one_pass()
    totals, blocks = [], []
    for _ in range(a.reps):
        blocks = one_pass()
        totals.append(sum(blocks))
    med = float(np.median(totals))
    per_draw = d + (0 if a.no_replicates else N)
    print(json.dumps(dict(config=a.one, chains=Cn, draws=S, n_data=N, d=d, replicates=not a.no_replicates,
                          block_draws=block, blocks=len(blocks), reps=a.reps, warmup=a.warmup,
                          kernel_ms=dict(median=round(med, 3), min=round(min(totals), 3), max=round(max(totals), 3)),
                          block_ms=dict(median=round(float(np.median(blocks)), 3), max=round(max(blocks), 3)),
                          variates=S * per_draw * Cn, variates_per_s=round(S * per_draw * Cn / (med * 1e-3), 0),
                          out_bytes=S * (2 * d + (0 if a.no_replicates else N)) * Cn * 8)), flush=True)
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
    ap.add_argument("--no-replicates", action="store_true", help="yrep = NULL: the free variables alone")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each config's step may take")
    a = ap.parse_args()
    if a.one:
        return one(a)
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--chains", str(a.chains), "--draws", str(a.draws),
               "--block", str(a.block)] + (["--no-replicates"] if a.no_replicates else [])
        rc = subprocess.call(cmd)
        if rc != 0:
            print("prior_time: step %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
