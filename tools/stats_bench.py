#!/usr/bin/env python3
"""Times the statistical stage (mdx_stats_run) at the defaults — --rand 30 --adjust 10 --burn 10000 --iter 50000,
--fix-nicks, m = 24 — for 1, 64 and 900 chains in one launch, on tables drawn from the model.  One JSON line per size."""

import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, nargs="+", default=[1, 64, 900])
    ap.add_argument("--per-row", type=int, default=100_000, help="bases of every reference base in a row of a table")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import stats_model as M
    from mapdamage_amd import stats
    truth = (0.012, 1.3, 0.02, 0.6, 0.35, 0.35, 1.0)
    acgt = (0.29, 0.21, 0.22, 0.28)
    nu = np.concatenate([np.ones(12), np.zeros(12)])
    rng = np.random.default_rng(1)
    distinct = [M.simulate_table(rng, M.Options(24), acgt, nu, truth, args.per_row) for _ in range(8)]
    options = stats.StatsOptions(fix_nicks=True, seed=1)
    stats.run_chains(distinct[0][None], nu, acgt, stats.StatsOptions(fix_nicks=True, burn=10, iterations=10, rand=1))     # warm-up
    for n in args.chains:
        tables = np.stack([distinct[k % len(distinct)] for k in range(n)])
        start = time.perf_counter()
        out = stats.run_chains(tables, nu, acgt, options, device=args.device)
        seconds = time.perf_counter() - start
        mean = out[0].trace[:, :7].mean(axis=0)
        print(json.dumps({"chains": n, "seconds": round(seconds, 3), "chains_per_second": round(n / seconds, 2),
                          "iterations_per_chain": 10 * 10000 + 50000, "mean_of_chain_0": [round(float(v), 5) for v in mean]}), flush=True)


if __name__ == "__main__":
    main()
