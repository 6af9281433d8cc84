"""Time the fused model-comparison call (exmc_hip_ic_stats) at the BASELINE configs.

For each config: sample (200 warmup, 1000 draws) on the device, run the fused call once to warm up,
then time it with the handle's HIP events (exmc_hip_last_kernel_ms) over --reps calls. Prints one JSON
line per config: datum-sample pairs per second, f64 operations and bytes counted from shapes, and the
share of the f64 issue and HBM bounds (78.6 TFLOP/s f64 vector peak as bench.py uses, 6.3 TB/s), next
to the config's sampling kernel time."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from exmc_amd import model_comparison as MC  # noqa: E402
from exmc_amd import models, sampler  # noqa: E402

PEAK_F64 = 78.6e12
PEAK_BW = 6.3e12
# f64 operations per datum-sample: the kind's term (exp / log ~ 25 each, a divide ~ 10) and the online
# update (two exp, compares, Welford ~ 60)
TERM_FLOPS = {"eight_schools": 8, "simple": 35, "sv": 65, "sv_ncp": 65, "logistic": 40 + 35, "radon": 20}
UPDATE_FLOPS = 60
CONFIGS = {
    "eight_schools": (models.eight_schools, 4096),
    "sv": (lambda: models.sv(models.sv_returns()), 2048),
    "sv_ncp": (lambda: models.sv_ncp(models.sv_returns()), 2048),
    "logistic": (models.logistic, 8192),
    "radon": (models.radon, 1024),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draws", type=int, default=1000)
    a = ap.parse_args()
    import torch
    for name in a.configs.split(","):
        make, Cn = CONFIGS[name]
        comp = sampler.compile(make())
        _, stats = sampler.sample_chains_compiled(comp, Cn, dict(num_warmup=200, num_samples=a.draws, seed=1))
        sample_ms = stats[0]["extra"]["kernel_ms"]
        raw = stats[0]["extra"]["raw"]["draws"]
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(raw).transpose(1, 2, 0))).cuda()
        del raw, stats
        S, d, C = x.shape
        N = MC.n_data(comp)
        out = torch.empty((4, N), dtype=torch.float64, device=x.device)
        torch.cuda.synchronize()
        comp.check(comp.L.exmc_hip_ic_stats(comp.h, x.data_ptr(), S, d, C, out.data_ptr()))
        ms = []
        for _ in range(a.reps):
            comp.check(comp.L.exmc_hip_ic_stats(comp.h, x.data_ptr(), S, d, C, out.data_ptr()))
            ms.append(comp.last_kernel_ms)
        t = float(np.median(ms)) / 1e3
        pairs = S * C * N
        flops = pairs * (TERM_FLOPS[name] + UPDATE_FLOPS)
        nbytes = S * d * C * 8 * ((N + 511) // 512)
        print(json.dumps(dict(config=name, S=S, C=C, N=N, d=d, fused_ms=round(t * 1e3, 3),
                              fused_ms_all=[round(v, 3) for v in ms], sampling_kernel_ms=round(sample_ms, 3),
                              share_of_sampling=round(t * 1e3 / sample_ms, 4),
                              pairs_per_s=pairs / t, f64_ops=flops, bytes=nbytes,
                              f64_bound_share=round(flops / t / PEAK_F64, 4),
                              hbm_bound_share=round(nbytes / t / PEAK_BW, 4))), flush=True)
        comp.close()


if __name__ == "__main__":
    main()
