"""Time model comparison of GENERATED models: the per-datum kernel of a plug-in compiled with
pointwise=True (gen_pointwise_kernel behind exmc_hip_pointwise_loglik_range), and waic / psis_loo composed
with libexmc_hip.so's model-free reductions (exmc_amd/model_comparison.py), beside the hand-written
kind's fused exmc_hip_ic_stats / exmc_hip_psis_stats on the same trace where a kind exists.

Without --one this is the driver: every leg is two child processes, each under its own `timeout` -- the
build of the leg's plug-in (--build-timeout; a cached plug-in returns at once), then the timed run
(--step-timeout) -- the steps are chained, and the first one that fails (or runs out of time) ends the run
with its exit status. With --one LEG it is one leg (--build-only: its plug-in and nothing else). Kernels are timed with HIP events (the handle's, exmc_hip_last_kernel_ms, for
the calls that have a handle; torch's around the composed Python calls), median of --reps. One JSON
line per leg.

Legs: eight_schools (codegen.eight_schools_ir, 1000 x 4096 trace sampled by the kind, the positions
in the generated flat order) and vector (a random walk of --n-obs steps observed with noise as ONE vector
obs: d = n-obs + 2, the 64-lane layout, ceil(n-obs / 16) generated functions, 1000 x 1024; it builds in
seconds, where the README model with as long an obs spends minutes in its one-lane warmup kernel)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0    # bench.py's figure (HBM3E, spec)
LEGS = ["eight_schools", "vector"]


def _median_ms(call, reps, ms_of):
    call()
    out = []
    for _ in range(reps):
        call()
        out.append(ms_of())
    return float(np.median(out)), [round(v, 3) for v in out]


def vector_ir(n):
    """noise, sigma (both :log) and a random walk of n steps observed with noise: one vector obs of n"""
    from exmc_amd import codegen as cg
    ir = cg.IR()
    ir.rv("noise", "half_normal", dict(sigma=1.0), transform="log")
    ir.rv("sigma", "exponential", {"lambda": 2.0}, transform="log")
    ir.rv("w", "gaussian_random_walk", dict(sigma="sigma", steps=n))
    ir.rv("y_rv", "normal", dict(mu="w", sigma="noise"))
    ir.obs("y", "y_rv", np.cumsum(np.random.default_rng(5).normal(size=n) * 0.3))
    return ir


def leg_spec(a):
    from exmc_amd import codegen as cg
    if a.one == "eight_schools":
        return cg.compile_ir(cg.eight_schools_ir(), name="gen_ic_es", pointwise=True)
    init = dict(noise=0.5, sigma=0.5, w=[0.0] * a.n_obs)
    return cg.compile_ir(vector_ir(a.n_obs), name="gen_ic_vec", default_init=init, pointwise=True)


def one(a):
    spec = leg_spec(a)
    if a.build_only:
        return
    import torch

    from exmc_amd import model_comparison as MC
    from exmc_amd import models, sampler
    kind = None
    if a.one == "eight_schools":
        kspec = models.eight_schools()
        kind = sampler.compile(kspec)
        comp = sampler.compile(spec)
        _, stats = sampler.sample_chains_compiled(kind, 4096, dict(num_warmup=200, num_samples=a.draws, seed=1))
        xk = np.ascontiguousarray(np.asarray(stats[0]["extra"]["raw"]["draws"]).transpose(1, 2, 0))
        del stats
        # (the kind's theta_trans_j is the generated model's non-centred theta_j)
        idx = [kspec.var_names.index(n.replace("theta_", "theta_trans_")) for n in comp.spec.var_names]
        x = torch.from_numpy(np.ascontiguousarray(xk[:, idx, :])).cuda()
        xk = torch.from_numpy(xk).cuda()
    else:
        comp = sampler.compile(spec)
        _, stats = sampler.sample_chains_compiled(comp, 1024, dict(num_warmup=200, num_samples=a.draws, seed=1))
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(stats[0]["extra"]["raw"]["draws"]).transpose(1, 2, 0))).cuda()
        del stats
    S, d, C = x.shape
    N = MC.n_data(comp)
    ll = torch.empty((S, N, C), dtype=torch.float64, device=x.device)
    torch.cuda.synchronize()
    L = comp.L
    pw_ms, pw_all = _median_ms(
        lambda: comp.check(L.exmc_hip_pointwise_loglik_range(comp.h, x.data_ptr(), S, d, C, 0, N, ll.data_ptr())),
        a.reps, lambda: comp.last_kernel_ms)
    written = 8.0 * S * N * C

    def composed(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        box = {}

        def call():
            torch.cuda.synchronize()
            ev0.record()
            box["r"] = fn(comp, x)
            ev1.record()
            torch.cuda.synchronize()
        ms, all_ms = _median_ms(call, a.reps, lambda: ev0.elapsed_time(ev1))
        return ms, all_ms, box["r"]
    waic_ms, waic_all, w = composed(MC.waic)
    psis_ms, psis_all, p = composed(MC.psis_loo)
    rec = dict(leg=a.one, S=S, C=C, d=d, N=N, lanes_per_chain=comp.spec.gen.lanes,
               generated_functions=comp.spec.gen.header.count("EXMC_GEN_PW_FN void"), pointwise_kernel_ms=round(pw_ms, 3), pointwise_kernel_ms_all=pw_all,
               matrix_bytes=written, written_gb_per_s=round(written / (pw_ms / 1e3) / 1e9, 1),
               share_of_hbm_peak=round(written / (pw_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
               waic_ms=round(waic_ms, 3), waic_ms_all=waic_all, psis_loo_ms=round(psis_ms, 3), psis_loo_ms_all=psis_all,
               elpd_waic=w["elpd_waic"], elpd_psis_loo=p["elpd_loo"], n_high_k=p["n_high_k"])
    if kind is not None:
        st = torch.empty((4, N), dtype=torch.float64, device=x.device)
        out = torch.empty((3, N), dtype=torch.float64, device=x.device)
        torch.cuda.synchronize()
        K = kind.L
        ic_ms, _ = _median_ms(lambda: kind.check(K.exmc_hip_ic_stats(kind.h, xk.data_ptr(), S, d, C, st.data_ptr())),
                              a.reps, lambda: kind.last_kernel_ms)
        kp_ms, _ = _median_ms(lambda: kind.check(K.exmc_hip_psis_stats(kind.h, xk.data_ptr(), S, d, C, 0, out.data_ptr())),
                              a.reps, lambda: kind.last_kernel_ms)
        kw = MC.waic(kind, xk)
        gap = lambda u, v: float(np.max(np.abs(u - v) / np.abs(v)))   # noqa: E731
        rec.update(kind_ic_stats_ms=round(ic_ms, 3), kind_psis_stats_ms=round(kp_ms, 3),
                   waic_over_kind=round(waic_ms / ic_ms, 2), psis_over_kind=round(psis_ms / kp_ms, 2),
                   kind_elpd_waic=kw["elpd_waic"],
                   max_rel_gap_lppd=gap(w["pointwise"]["lppd"], kw["pointwise"]["lppd"]),
                   max_rel_gap_elpd_waic_i=gap(w["pointwise"]["elpd_waic"], kw["pointwise"]["elpd_waic"]))
        kind.close()
    print(json.dumps(rec), flush=True)
    comp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--one", default=None, help="run this one leg in this process")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--n-obs", type=int, default=200, help="elements of the vector leg's obs (d = n-obs + 2 <= 256)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each leg's timed run may take")
    ap.add_argument("--build-timeout", type=int, default=900, help="seconds each leg's plug-in build may take")
    ap.add_argument("--build-only", action="store_true", help="with --one: build the leg's plug-in and return")
    a = ap.parse_args()
    if a.one:
        return one(a)
    for name in a.legs.split(","):
        step = [sys.executable, os.path.abspath(__file__), "--one", name, "--reps", str(a.reps), "--draws", str(a.draws),
                "--n-obs", str(a.n_obs)]
        for what, cmd in (("build", ["timeout", "-k", "10", str(a.build_timeout)] + step + ["--build-only"]),
                          ("run", ["timeout", "-k", "10", str(a.step_timeout)] + step)):
            rc = subprocess.call(cmd)
            if rc != 0:
                print("gen_ic_time: %s of leg %s ended with status %d; stopping" % (what, name, rc), file=sys.stderr)
                sys.exit(rc)


if __name__ == "__main__":
    main()
