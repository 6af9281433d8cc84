"""Time Pathfinder (exmc_hip_pathfinder) at two batch sizes of the BASELINE kinds, beside the cost of
one value-and-gradient evaluation of the same model at the same batch.

Without --one this is the driver: every config is a step of its own, a child process under its own
`timeout`, chained; the first that fails ends the run with its exit status. With --one CONFIG it is
one step. Kernel milliseconds come from the handle's HIP events (exmc_hip_last_kernel_ms, which
enclose the launch only): --warmup calls are thrown away, --reps calls are kept, median and spread
(min .. max) are printed. Two series: the default options (1000 draws, 100 iterations, history 6)
and num_draws = 1, which separates the path from the draws. Two evaluation figures at the same number
of chains in the same layout: one launch of logp_grad_kernel (exmc_hip_logp_grad_host; the events
enclose that launch, so the figure carries a launch's fixed cost: an upper bound on an evaluation
inside a longer kernel), and multi_step_kernel over --steps leapfrog steps divided by the steps (one
M::logp_grad per step plus the leapfrog update and four trace rows, the launch cost spread over the
steps). One JSON line per config."""
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

    out = dict(config=a.one, paths=Cn, lanes=lanes, d=d, reps=a.reps, warmup=a.warmup)
    mu = torch.empty((d, Cn), dtype=torch.float64, device=dev)
    sg = torch.empty((d, Cn), dtype=torch.float64, device=dev)
    el = torch.empty(Cn, dtype=torch.float64, device=dev)
    ni = torch.empty(Cn, dtype=torch.int32, device=dev)
    for key, S in (("default", 1000), ("one_draw", 1)):
        dr = torch.empty((S, d, Cn), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        po = _lib.PfOpts(S, 100, 6, 1, lanes)
        out[key] = series(lambda: L.exmc_hip_pathfinder(comp.h, po, Cn, 0, dr.data_ptr(), mu.data_ptr(), sg.data_ptr(),
                                                        el.data_ptr(), ni.data_ptr(), None, None))
        out[key]["mean_path_length"] = round(float(ni.float().mean().item()), 2)
        del dr
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
    path = out["one_draw"]["median_ms"]
    out["path_over_101_multi_steps"] = round(path / (101 * out["multi_step"]["per_step_ms"]["median_ms"]), 2)
    out["path_over_101_logp_grad_launches"] = round(path / (101 * out["logp_grad_kernel"]["median_ms"]), 3)
    print(json.dumps(out), flush=True)
    comp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="eight_schools,sv_ncp")
    ap.add_argument("--one", default=None, help="run this one config in this process")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds each config's step may take")
    a = ap.parse_args()
    if a.one:
        return one(a)
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--steps", str(a.steps)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("pathfinder_time: step %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
