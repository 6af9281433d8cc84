"""Time SMC (exmc_hip_smc) on two BASELINE kinds: eight_schools at 16 lanes and sv_ncp at 64 lanes,
64 runs x 500 particles at the reference's defaults (threshold_ratio 0.5, 5 MH steps).

Without --one this is the driver: every config is a step of its own, a child process under its own
`timeout`, chained; the first that fails ends the run with its exit status. With --one CONFIG it is
one step. Kernel milliseconds come from the handle's HIP events (exmc_hip_last_kernel_ms: for
exmc_hip_smc the sum over the call's kernels): one warm-up call is thrown away, then the median of
--reps calls (3). The split: the same run driven through exmc_hip_smc_init / _reweight / _mutate, the
mutation's share being the sum of exmc_hip_last_kernel_ms over the mutate calls (median of the same
number of runs); the rest is the whole call minus that. The stages per run are reported too.
With --bridged the same configs run in the bridged mode (exmc_hip_smc_bridge and its steps, the default
base), and the mean log evidence over the runs is reported.
One JSON line per config. None of these numbers is a pass criterion."""
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
    return {"eight_schools": (models.eight_schools, 16),
            "sv_ncp": (lambda: models.sv_ncp(models.sv_returns()), 64)}


def _stepwise(comp, co, R, d, lanes, bridged=False):
    """init, then reweight / mutate on the same device arrays; the mutation's kernel milliseconds"""
    import torch

    from exmc_amd import _lib
    N, S = co.num_particles, co.max_stages
    Cn = R * N
    dev = torch.device("cuda", comp.device)
    f8, i4, i8 = (dict(dtype=t, device=dev) for t in (torch.float64, torch.int32, torch.int64))
    q, lp, words = torch.zeros((d, Cn), **f8), torch.zeros(Cn, **f8), torch.zeros((2, Cn), **i8)
    t = dict(beta=torch.zeros(R, **f8), run_rng=torch.zeros((2, R), **i8), active=torch.zeros(R, **i4),
             scale=torch.zeros((d, R), **f8), accept=torch.zeros(Cn, **i4), betas=torch.zeros((S, R), **f8),
             ess_history=torch.zeros((S, R), **f8), acceptance_rates=torch.zeros((S, R), **f8),
             num_stages=torch.zeros(R, **i4), status=torch.zeros(R, **i4), active_count=torch.zeros(1, **i4))
    st = _lib.SmcState(*[t[k].data_ptr() for k, _ in _lib.SmcState._fields_])
    lb, le, les = torch.zeros(Cn, **f8), torch.zeros(R, **f8), torch.zeros((S, R), **f8)
    torch.cuda.synchronize(dev)
    L, h, qp, lpp, lbp, wp = comp.L, comp.h, q.data_ptr(), lp.data_ptr(), lb.data_ptr(), words.data_ptr()
    if bridged:
        comp.check(L.exmc_hip_smc_bridge_init(h, co, R, 0, None, None, qp, lpp, lbp, wp, st, le.data_ptr(), les.data_ptr()))
    else:
        comp.check(L.exmc_hip_smc_init(h, co, R, 0, qp, lpp, wp, st))
    init_ms, mutate_ms = comp.last_kernel_ms, 0.0
    for stage in range(S + 1):
        if bridged:
            comp.check(L.exmc_hip_smc_bridge_reweight(comp.device, co, R, d, stage, qp, lpp, lbp, st, le.data_ptr(),
                                                      les.data_ptr()))
        else:
            comp.check(L.exmc_hip_smc_reweight(comp.device, co, R, d, stage, qp, lpp, st))
        if int(t["active_count"].cpu()[0]) == 0:
            break
        if bridged:
            comp.check(L.exmc_hip_smc_bridge_mutate(h, co, R, None, None, qp, lpp, lbp, wp, st))
        else:
            comp.check(L.exmc_hip_smc_mutate(h, co, R, qp, lpp, wp, st))
        mutate_ms += comp.last_kernel_ms
    return init_ms, mutate_ms, t["num_stages"].cpu().numpy()


def one(a):
    import torch

    from exmc_amd import _lib, sampler
    make, lanes = _configs()[a.one]
    comp = sampler.compile(make())
    d, R, N = comp.d, a.runs, a.particles
    co = _lib.SmcOpts(N, 0.5, 5, 1, a.max_stages, lanes)
    dev = torch.device("cuda", 0)
    ns = torch.zeros(R, dtype=torch.int32, device=dev)
    status = torch.zeros(R, dtype=torch.int32, device=dev)
    le = torch.zeros(R, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def whole():
        if a.bridged:
            comp.check(comp.L.exmc_hip_smc_bridge(comp.h, co, R, 0, None, None, None, None, None, None, None, None,
                                                  ns.data_ptr(), status.data_ptr(), le.data_ptr(), None))
        else:
            comp.check(comp.L.exmc_hip_smc(comp.h, co, R, 0, None, None, None, None, None, ns.data_ptr(), status.data_ptr()))
        return comp.last_kernel_ms
    for _ in range(a.warmup):
        whole()
    ms = [whole() for _ in range(a.reps)]
    stages = ns.cpu().numpy()
    split = [_stepwise(comp, co, R, d, lanes, a.bridged) for _ in range(a.warmup + a.reps)][a.warmup:]
    assert all(np.array_equal(s[2], stages) for s in split)      # the same runs
    total, mutate = float(np.median(ms)), float(np.median([s[1] for s in split]))
    out = dict(config=a.one, mode="bridged" if a.bridged else "reference", runs=R, particles=N, lanes=lanes, d=d, reps=a.reps, warmup=a.warmup,
               kernel_ms=dict(median=round(total, 3), min=round(min(ms), 3), max=round(max(ms), 3)),
               mutate_ms=round(mutate, 3), init_ms=round(float(np.median([s[0] for s in split])), 3),
               rest_ms=round(total - mutate, 3),
               stages=dict(mean=round(float(stages.mean()), 2), min=int(stages.min()), max=int(stages.max())),
               capped=int(status.cpu().numpy().sum()))
    if a.bridged:
        ev = le.cpu().numpy()
        out["log_evidence"] = dict(mean=round(float(ev.mean()), 3), min=round(float(ev.min()), 3), max=round(float(ev.max()), 3))
    print(json.dumps(out), flush=True)
    comp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="eight_schools,sv_ncp")
    ap.add_argument("--one", default=None, help="run this one config in this process")
    ap.add_argument("--runs", type=int, default=64)
    ap.add_argument("--particles", type=int, default=500)
    ap.add_argument("--max-stages", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bridged", action="store_true", help="the bridged mode (include/exmc_hip_smc_bridge.h)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each config's step may take")
    a = ap.parse_args()
    if a.one:
        return one(a)
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one", name,
               "--runs", str(a.runs), "--particles", str(a.particles), "--max-stages", str(a.max_stages),
               "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--bridged"] if a.bridged else [])
        rc = subprocess.call(cmd)
        if rc != 0:
            print("smc_time: step %s ended with status %d; stopping" % (name, rc), file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
