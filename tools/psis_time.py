"""Time PSIS-LOO (exmc_hip_psis_stats) at the BASELINE configs, beside exmc_hip_ic_stats and the
sampling kernel of the same run.

Without --one this is the driver: every config is a step of its own, a child process under its own
`timeout`, and the steps are chained: the first one that fails (or runs out of time) ends the run with
its exit status. With --one CONFIG it is one step: sample (200 warmup, --draws draws) on the device, run
each call once to warm up, then time it with the handle's HIP events (exmc_hip_last_kernel_ms, which
enclose the launches only) over --reps calls, for every scratch budget of --scratch-gib. Prints one
JSON line per config and budget."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CONFIGS = ["eight_schools", "sv", "logistic", "radon"]   # the four BASELINE kinds, ic_time.py's sizes


def one(a):
    import torch

    import ic_time
    from exmc_amd import model_comparison as MC
    from exmc_amd import sampler
    make, Cn = ic_time.CONFIGS[a.one]
    comp = sampler.compile(make())
    _, stats = sampler.sample_chains_compiled(comp, Cn, dict(num_warmup=200, num_samples=a.draws, seed=1))
    sample_ms = stats[0]["extra"]["kernel_ms"]
    raw = stats[0]["extra"]["raw"]["draws"]
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(raw).transpose(1, 2, 0))).cuda()
    del raw, stats
    S, d, C = x.shape
    N = MC.n_data(comp)
    L = comp.L

    def timed(call):
        comp.check(call())
        ms = []
        for _ in range(a.reps):
            comp.check(call())
            ms.append(comp.last_kernel_ms)
        return float(np.median(ms)), [round(v, 3) for v in ms]

    st = torch.empty((4, N), dtype=torch.float64, device=x.device)
    out = torch.empty((3, N), dtype=torch.float64, device=x.device)
    torch.cuda.synchronize()
    ic_ms, _ = timed(lambda: L.exmc_hip_ic_stats(comp.h, x.data_ptr(), S, d, C, st.data_ptr()))
    n = S * C
    per = n * 8
    for gib in a.scratch_gib:
        budget = int(gib * (1 << 30))
        nb = max(1, min(N, budget // per))
        ms, all_ms = timed(lambda: L.exmc_hip_psis_stats(comp.h, x.data_ptr(), S, d, C, budget, out.data_ptr()))
        k = out[2].cpu().numpy()
        print(json.dumps(dict(config=a.one, S=S, C=C, N=N, d=d, tail_max=int(np.ceil(min(n / 5, 3 * np.sqrt(n)))),
                              scratch_gib=gib, datums_per_block=int(nb), blocks=-(-N // int(nb)),
                              psis_ms=round(ms, 3), psis_ms_all=all_ms, ic_stats_ms=round(ic_ms, 3),
                              sampling_kernel_ms=round(sample_ms, 3), psis_over_ic=round(ms / ic_ms, 2),
                              share_of_sampling=round(ms / sample_ms, 4), pairs_per_s=n * N / (ms / 1e3),
                              k_max=float(np.nanmax(k[np.isfinite(k)])) if np.any(np.isfinite(k)) else None,
                              n_k_above_0p7=int(np.sum(k > 0.7)), n_k_nan=int(np.sum(np.isnan(k))))), flush=True)
    comp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--one", default=None, help="run this one config in this process")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--scratch-gib", type=lambda s: [float(v) for v in s.split(",")], default=[1.0])
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each config's step may take")
    a = ap.parse_args()
    if a.one:
        return one(a)
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", name,
               "--reps", str(a.reps), "--draws", str(a.draws),
               "--scratch-gib", ",".join(str(v) for v in a.scratch_gib)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("psis_time: step %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
