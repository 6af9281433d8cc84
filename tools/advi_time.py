"""Time ADVI (exmc_hip_advi) at two batch sizes of the BASELINE kinds, beside the cost of one
value-and-gradient evaluation of the same model at the same batch.

Without --one this is the driver: every config is a step of its own, a child process under its own
`timeout`, chained; the first that fails ends the run with its exit status. With --one CONFIG it is
one step. Kernel milliseconds come from the handle's HIP events (exmc_hip_last_kernel_ms, which
enclose the launch only): --warmup calls are thrown away, --reps calls are kept, median and spread
(min .. max) are printed.

Two series at the reference's defaults (10000 iterations at most, window 100, one sample): 1000 draws
and num_draws = 1, with the mean num_iters of the batch. Then the kernel's time per iteration is split
by differencing runs of a fixed length (--iters iterations, convergence_tol = 0 so that no fit stops,
one draw), never by instrumenting the kernel:
  window      (window_size 100) - (window_size 2), per iteration: the two half-window sums
  sample      (num_mc_samples 2) - (num_mc_samples 1), per iteration: one more sample, that is d variates
              walked by every lane of the group plus one evaluation
  generator   (1000 draws) - (1 draw), per draw: d variates walked by every lane of the group (and one
              store per dimension)
  evaluation  sample - generator
Two evaluation figures at the same number of chains in the same layout, as tools/pathfinder_time.py
gives them: one launch of logp_grad_kernel, and multi_step_kernel over --steps leapfrog steps divided
by the steps; the kernel's cost per iteration is given in multi_step steps. One JSON line per config."""
import argparse
import ctypes as C
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
    L, d = comp.L, comp.d
    dev = torch.device("cuda", 0)

    def series(call):
        for _ in range(a.warmup):
            comp.check(call())
        ms = []
        for _ in range(a.reps):
            comp.check(call())
            ms.append(comp.last_kernel_ms)
        return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))

    out = dict(config=a.one, fits=Cn, lanes=lanes, d=d, reps=a.reps, warmup=a.warmup)
    mu = torch.empty((d, Cn), dtype=torch.float64, device=dev)
    ls = torch.empty((d, Cn), dtype=torch.float64, device=dev)
    ni = torch.empty(Cn, dtype=torch.int32, device=dev)
    cv = torch.empty(Cn, dtype=torch.int32, device=dev)
    dr = torch.empty((1000, d, Cn), dtype=torch.float64, device=dev)

    def run(S, iters, n_mc, window, tol):
        hist = torch.empty((iters, Cn), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ao = _lib.AdviOpts(S, iters, n_mc, window, 0.01, tol, 1, lanes)
        r = series(lambda: L.exmc_hip_advi(comp.h, ao, Cn, 0, dr.data_ptr(), mu.data_ptr(), ls.data_ptr(),
                                           hist.data_ptr(), ni.data_ptr(), cv.data_ptr()))
        r["mean_num_iters"] = round(float(ni.float().mean().item()), 2)
        r["converged"] = int(cv.sum().item())
        return r

    out["default"] = run(1000, 10000, 1, 100, 1.0e-4)
    out["one_draw"] = run(1, 10000, 1, 100, 1.0e-4)
    n = a.iters
    fixed = {"base": run(1, n, 1, 100, 0.0), "window_2": run(1, n, 1, 2, 0.0), "two_samples": run(1, n, 2, 100, 0.0),
             "draws_1000": run(1000, n, 1, 100, 0.0)}
    out["fixed_length"] = dict(iters=n, **fixed)
    base = fixed["base"]["median_ms"]
    per_iter = base / n
    window = (base - fixed["window_2"]["median_ms"]) / n
    sample = (fixed["two_samples"]["median_ms"] - base) / n
    generator = (fixed["draws_1000"]["median_ms"] - base) / 999
    out["per_iteration_ms"] = dict(total=round(per_iter, 6), window=round(window, 6), sample=round(sample, 6),
                                   generator=round(generator, 6), evaluation=round(sample - generator, 6),
                                   rest=round(per_iter - window - sample, 6))

    # one evaluation: multi_step_kernel from small random points, n steps of a tiny step size
    n = a.steps
    rng = np.random.default_rng(0)
    q = torch.from_numpy(rng.normal(size=(d, Cn)) * 0.1).to(dev)
    p = torch.zeros((d, Cn), dtype=torch.float64, device=dev)
    g = torch.zeros((d, Cn), dtype=torch.float64, device=dev)
    aq, ap_, ag = (torch.empty((n, d, Cn), dtype=torch.float64, device=dev) for _ in range(3))
    al = torch.empty((n, Cn), dtype=torch.float64, device=dev)
    im = np.ones(d)
    torch.cuda.synchronize()
    ev = series(lambda: L.exmc_hip_multi_step(comp.h, q.data_ptr(), p.data_ptr(), g.data_ptr(), 1e-6,
                                              im.ctypes.data_as(C.POINTER(C.c_double)), n, Cn, lanes, aq.data_ptr(),
                                              ap_.data_ptr(), al.data_ptr(), ag.data_ptr()))
    out["multi_step"] = dict(steps=n, per_step_ms={k: round(v / n, 5) for k, v in ev.items()})
    qh = np.ascontiguousarray(rng.normal(size=(Cn, d)) * 0.1)
    lp, gr = np.zeros(Cn), np.zeros((Cn, d))
    dp = C.POINTER(C.c_double)
    out["logp_grad_kernel"] = series(lambda: L.exmc_hip_logp_grad_host(comp.h, qh.ctypes.data_as(dp), Cn, lanes,
                                                                       lp.ctypes.data_as(dp), gr.ctypes.data_as(dp)))
    out["iteration_over_multi_step"] = round(per_iter / out["multi_step"]["per_step_ms"]["median_ms"], 2)
    out["iteration_over_logp_grad_launch"] = round(per_iter / out["logp_grad_kernel"]["median_ms"], 4)
    print(json.dumps(out), flush=True)
    comp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="eight_schools,sv_ncp")
    ap.add_argument("--one", default=None, help="run this one config in this process")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=1000, help="iterations of the fixed-length runs")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each config's step may take")
    a = ap.parse_args()
    if a.one:
        return one(a)
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--steps", str(a.steps), "--iters", str(a.iters)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("advi_time: step %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
