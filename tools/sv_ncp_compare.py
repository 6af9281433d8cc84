"""sv centred (EXMC_MODEL_SV) against sv non-centred (EXMC_MODEL_SV_NCP) and against the generated
non-centred form (codegen.sv_ir compiled with ncp: true, the walk as scan chains) in one process: the
same returns, the same seed, the bench's protocol (one shared warmup, then N chains of S draws).
The generated form is compiled for two resident waves per SIMD, like the bench's gen_sv; with
--time-build its plug-in is rebuilt and the build's seconds go into its row. --unrolled adds the
generated text with scan=False (the walk unrolled into every lane).

Per form: sampling-kernel and warmup ms (device events, Compiled.last_kernel_ms), leapfrogs per draw
and per second, divergences, max split R-hat (the library's exmc_hip_rhat) and the minimum over
parameters of the bulk ESS per chain (exmc_hip_ess_bulk, mean over chains) with ESS per second of
the sampling kernel. The diagnostics are taken on the constrained draws (s_t, sigma, nu), which for
the non-centred form is the reconstructed walk. Prints one JSON line per form and a markdown table.

    python tools/sv_ncp_compare.py [--chains 2048] [--warmup 1000] [--samples 1000] [--seed 42] [--out FILE]
                                   [--no-gen] [--unrolled] [--time-build]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from exmc_amd import codegen, diagnostics, models, sampler  # noqa: E402


def generated(returns, scan, time_build):
    """(spec, plug-in build seconds or None) of non-centred sv from its node list"""
    ir = codegen.sv_ir(returns)
    gen = codegen.generate(ir, ncp=True, lanes=64, waves_per_simd=2, scan=scan)
    t0 = time.time()
    so = codegen.build_plugin(gen, force=time_build)
    name = "gen_sv_ncp" if scan else "gen_sv_ncp_unrolled"
    spec = codegen.GeneratedSpec(gen, so, name=name, default_init=models.sv_ncp(returns).default_init)
    return spec, (time.time() - t0) if time_build else None


def run(spec, n_chains, num_warmup, num_samples, seed, build_s=None):
    comp = sampler.compile(spec)
    try:
        opts = dict(num_warmup=num_warmup, num_samples=num_samples, seed=seed, lanes_per_chain=64)
        tuning = sampler.warmup(comp, spec.default_init, opts)
        warm_ms = comp.last_kernel_ms
        _, _, extra = sampler.sample_compiled_tuned(comp, tuning, spec.default_init, opts, num_chains=n_chains)
        samp_ms = comp.last_kernel_ms
        raw = extra["raw"]
        x = spec.constrain(raw["draws"])                       # [C][S][d]
        rhat = diagnostics.rhat(comp, x)
        eb = diagnostics.ess_bulk(comp, x)                     # [d][C]
        per_chain = eb.mean(axis=1)
        lf = int(extra["total_leapfrogs"])
        draws = n_chains * num_samples
        min_ess = float(per_chain.min())
        return dict(form=spec.name, chains=n_chains, warmup=num_warmup, samples=num_samples, seed=seed,
                    epsilon=float(tuning["epsilon"]), warmup_ms=float(warm_ms), sampling_ms=float(samp_ms),
                    leapfrogs=lf, leapfrogs_per_draw=lf / draws, leapfrogs_per_s=lf / (samp_ms / 1e3),
                    divergences=int(raw["divergent"].sum()), max_split_rhat=float(np.nanmax(rhat)),
                    min_bulk_ess_per_chain=min_ess, min_ess_param=spec.var_names[int(per_chain.argmin())],
                    ess_per_s=min_ess * n_chains / (samp_ms / 1e3), build_s=build_s)
    finally:
        comp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-gen", action="store_true", help="only the two hand-written kinds")
    ap.add_argument("--unrolled", action="store_true", help="also the generated text with scan=False")
    ap.add_argument("--time-build", action="store_true", help="rebuild the generated plug-ins and time it")
    a = ap.parse_args()
    r = models.sv_returns()
    legs = [(models.sv(r), None), (models.sv_ncp(r), None)]
    if not a.no_gen:
        legs.append(generated(r, True, a.time_build))
    if a.unrolled:
        legs.append(generated(r, False, a.time_build))
    rows = []
    for spec, build_s in legs:
        rows.append(run(spec, a.chains, a.warmup, a.samples, a.seed, build_s))
        print(json.dumps(rows[-1], sort_keys=True), flush=True)
    lines = [json.dumps(row, sort_keys=True) for row in rows]
    lines += ["", "| form | eps | warmup ms | sampling ms | leapfrogs / draw | leapfrog / s | divergent | "
              "max split R-hat | min bulk ESS / chain | ESS / s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        lines.append("| %s | %.4g | %.1f | %.1f | %.1f | %.3g | %d / %d | %.3f | %.1f (%s) | %.3g |" % (
            row["form"], row["epsilon"], row["warmup_ms"], row["sampling_ms"], row["leapfrogs_per_draw"],
            row["leapfrogs_per_s"], row["divergences"], row["chains"] * row["samples"], row["max_split_rhat"],
            row["min_bulk_ess_per_chain"], row["min_ess_param"], row["ess_per_s"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
