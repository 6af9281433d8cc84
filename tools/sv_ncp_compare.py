"""sv centred (EXMC_MODEL_SV) against sv non-centred (EXMC_MODEL_SV_NCP) in one process: the same
returns, the same seed, the bench's protocol (one shared warmup, then N chains of S draws).

Per form: sampling-kernel and warmup ms (device events, Compiled.last_kernel_ms), leapfrogs per draw
and per second, divergences, max split R-hat (the library's exmc_hip_rhat) and the minimum over
parameters of the bulk ESS per chain (exmc_hip_ess_bulk, mean over chains) with ESS per second of
the sampling kernel. The diagnostics are taken on the constrained draws (s_t, sigma, nu), which for
the non-centred form is the reconstructed walk. Prints one JSON line per form and a markdown table.

    python tools/sv_ncp_compare.py [--chains 2048] [--warmup 1000] [--samples 1000] [--seed 42] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from exmc_amd import diagnostics, models, sampler  # noqa: E402


def run(spec, n_chains, num_warmup, num_samples, seed):
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
                    ess_per_s=min_ess * n_chains / (samp_ms / 1e3))
    finally:
        comp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = models.sv_returns()
    rows = [run(spec, a.chains, a.warmup, a.samples, a.seed) for spec in (models.sv(r), models.sv_ncp(r))]
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
