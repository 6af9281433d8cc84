"""CPU only: what the lock-step walk of a sampling launch has to do, from the checker's n_steps.

The one-wave leaf-pair form of nuts_run (exmc_nuts.hpp) takes one pass for the leaf of doubling 0 and
one pass per leaf pair afterwards, so a tree of n leapfrogs costs 1 + n // 2 passes; the four 16-lane
groups of a wave (chains 4w .. 4w + 3) walk in lock step, so a wave-transition costs the maximum of its
four, and the launch ends with its slowest wave. Printed for a workload: the tree-size histogram,
passes per chain-transition and per wave-transition, the share of wave-transitions that are exactly
doublings 0-2, and the per-wave totals with their tail.

    python tools/wave_pass_account.py [--chains 4096] [--draws 1000] [--adapt 1000] [--seed 42] [--lanes 16]

The defaults are bench.py's flagship launch (eight_schools, 4096 chains x 1000 draws): the checker
reproduces its leapfrog and divergence counts exactly ("Round 9").
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def account(n_steps, groups_per_wave=4):
    """n_steps [chains][draws] -> dict of the figures printed below"""
    n = np.asarray(n_steps)
    chains, draws = n.shape
    passes = 1 + n // 2
    full = chains - chains % groups_per_wave
    wave = passes[:full].reshape(full // groups_per_wave, groups_per_wave, draws)
    wn = n[:full].reshape(full // groups_per_wave, groups_per_wave, draws)
    wmax = wave.max(axis=1)
    totals = np.sort(wmax.sum(axis=1))
    sizes, counts = np.unique(n, return_counts=True)
    return dict(
        sizes=sizes, counts=counts, total=n.size,
        passes_chain=passes.mean(), passes_wave=wmax.mean(),
        wave_exact_prefix=(wmax == 4).mean(), wave_all_seven=(wn == 7).all(axis=1).mean(),
        totals=totals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--adapt", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import oracle as O
    from exmc_amd import models

    spec = models.eight_schools()
    q0 = spec.to_unconstrained(spec.default_init)
    t, st = O.sample_chains(O.model_for(spec), a.chains, init_q=q0, num_warmup=a.adapt, num_samples=a.draws,
                            seed=a.seed, n_threads=a.threads, cfg=O.Cfg(1, a.lanes))
    n = t["n_steps"]
    r = account(n, 64 // a.lanes)
    print("step size %r, leapfrogs %d, divergences %d" % (st.step_size, int(n.sum()), int((t["divergent"] != 0).sum())))
    print("tree sizes (leapfrogs: share of transitions)")
    for s, c in zip(r["sizes"], r["counts"]):
        if c / r["total"] >= 0.001 or s >= 127:
            print("  %5d: %8.4f %%  (%d)" % (s, 100.0 * c / r["total"], c))
    n_ = np.asarray(n)
    print("exactly 7: %.2f %%   exactly 15: %.2f %%   fewer than 7: %.2f %%   more than 15: %.2f %%"
          % (100 * (n_ == 7).mean(), 100 * (n_ == 15).mean(), 100 * (n_ < 7).mean(), 100 * (n_ > 15).mean()))
    print("passes per chain-transition %.3f, per wave-transition (max of %d groups) %.3f"
          % (r["passes_chain"], 64 // a.lanes, r["passes_wave"]))
    print("wave-transitions of exactly the four passes of doublings 0-2: %.1f %%; all groups at 7 leapfrogs: %.1f %%"
          % (100 * r["wave_exact_prefix"], 100 * r["wave_all_seven"]))
    tt = r["totals"]
    print("lock-step passes per wave over the launch: mean %.0f, sd %.0f, median %d, p99 %d"
          % (tt.mean(), tt.std(), int(np.median(tt)), int(np.percentile(tt, 99))))
    print("slowest waves: %s" % ", ".join(str(int(v)) for v in tt[::-1][:6]))
    print("largest trees: %s" % ", ".join(str(int(v)) for v in np.sort(n_.ravel())[::-1][:4]))
    print("launch / mean wave = %.3f" % (tt[-1] / tt.mean()))


if __name__ == "__main__":
    main()
