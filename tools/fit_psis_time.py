"""Time the importance diagnostics of the fits (include/exmc_hip_fit_psis.h) beside the fit launch itself:
eight_schools x 4096 Pathfinder paths x 1000 draws at 16 lanes and sv_ncp x 2048 x 1000 at 64 lanes, per fit
and pooled.

Without --one this is the driver: every config is a step of its own, a child process under its own
`timeout`, chained; the first that fails ends the run with its exit status. With --one CONFIG it is one step.
Every figure is kernel milliseconds from the handle's HIP events (exmc_hip_last_kernel_ms; the scratch is
allocated in front of them): one warm-up call is thrown away, three are kept, the median is printed with
min .. max. The three stages are differences of calls that share their front part:
    log ratio   exmc_hip_fit_log_ratio
    smoothing   exmc_hip_fit_psis without resampling, minus the log ratio (tail, weights, merge, normalise)
    resampling  exmc_hip_fit_psis with 1000 resampled draws per group, minus the call without (scan,
                search, gather)
Pooled, the paths without a finite ELBO are left out first, as importance.psis_fit does. One JSON line per
config."""
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
    return {"eight_schools": (models.eight_schools, 4096, 16),
            "sv_ncp": (lambda: models.sv_ncp(models.sv_returns()), 2048, 64)}


def one(a):
    import torch

    from exmc_amd import _lib, sampler
    make, Cn, lanes = _configs()[a.one]
    comp = sampler.compile(make())
    L, d, S, R = comp.L, comp.d, a.draws, a.resample
    dev = torch.device("cuda", 0)
    f64 = torch.float64

    def series(call):
        for _ in range(a.warmup):
            comp.check(call())
        ms = []
        for _ in range(a.reps):
            comp.check(call())
            ms.append(comp.last_kernel_ms)
        return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    dr = torch.empty((S, d, Cn), dtype=f64, device=dev)
    mu = torch.empty((d, Cn), dtype=f64, device=dev)
    sg = torch.empty((d, Cn), dtype=f64, device=dev)
    st = torch.empty(Cn, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    po = _lib.PfOpts(S, 100, 6, 1, lanes)
    out = dict(config=a.one, fits=Cn, draws=S, lanes=lanes, d=d, resample=R, reps=a.reps, warmup=a.warmup)
    out["pathfinder"] = series(lambda: L.exmc_hip_pathfinder(comp.h, po, Cn, 0, dr.data_ptr(), mu.data_ptr(),
                                                             sg.data_ptr(), None, None, None, st.data_ptr()))
    keep = torch.nonzero(st == 0).reshape(-1)
    out["failed_paths"] = Cn - int(keep.numel())
    for view in ("per_fit", "pooled"):
        pooled = view == "pooled"
        x, m, s = dr, mu, sg
        if pooled and keep.numel() < Cn:
            x, m, s = (t.index_select(t.dim() - 1, keep).contiguous() for t in (dr, mu, sg))
        F = x.shape[2]
        G = 1 if pooled else F
        lr = torch.empty((S, F), dtype=f64, device=dev)
        lw = torch.empty((S, F), dtype=f64, device=dev)
        o = torch.empty((5, G), dtype=f64, device=dev)
        idx = torch.empty((R, G), dtype=torch.int32, device=dev)
        res = torch.empty((R, d, G), dtype=f64, device=dev)
        torch.cuda.synchronize()
        head = [comp.h, x.data_ptr(), m.data_ptr(), s.data_ptr(), _lib.FIT_SIGMA, S, d, F, lanes]
        t_lr = series(lambda: L.exmc_hip_fit_log_ratio(*head, lr.data_ptr(), None))
        t_sm = series(lambda: L.exmc_hip_fit_psis(*head, int(pooled), 0, 1, o.data_ptr(), lw.data_ptr(), None, None,
                                                  lr.data_ptr(), None))
        t_rs = series(lambda: L.exmc_hip_fit_psis(*head, int(pooled), R, 1, o.data_ptr(), lw.data_ptr(), idx.data_ptr(),
                                                  res.data_ptr(), lr.data_ptr(), None))
        oh = o.cpu().numpy()
        out[view] = dict(fits=F, log_ratio=t_lr, through_smoothing=t_sm, through_resampling=t_rs,
                         smoothing_ms=round(t_sm["median_ms"] - t_lr["median_ms"], 4),
                         resampling_ms=round(t_rs["median_ms"] - t_sm["median_ms"], 4),
                         khat_median=float(np.nanmedian(oh[0])), khat_above_0_7=int(np.sum(~(oh[0] <= 0.7))),
                         nan_groups=int(np.isnan(oh[0]).sum()), tail=float(np.nanmax(oh[4])))
        del lr, lw, o, idx, res
    print(json.dumps(out), flush=True)
    comp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="eight_schools,sv_ncp")
    ap.add_argument("--one", default=None, help="run this one config in this process")
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--resample", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds each config's step may take")
    a = ap.parse_args()
    if a.one:
        return one(a)
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", name,
               "--draws", str(a.draws), "--resample", str(a.resample), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("fit_psis_time: step %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
