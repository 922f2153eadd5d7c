#!/usr/bin/env python3
"""als_fold_in against the only route to the same rows without it, in ONE process with interleaved rounds.

  python tools/foldbench.py [--rounds 5] [--ks 64,128] [--queries 1,1024,65536] [--nnz 100000000]

Synthetic Netflix shape (480,189 x 17,770), factors left from 2 iterations, per k in --ks. The queries are the in-blocks
of the first 1, 1,024 and 65,536 users. Timed, wall clock around the synchronous calls (each ends in a stream sync and
includes its host <-> device copies, which is what a caller pays):
  fold_in  : engine.fold_in(user, queries) -> host rows
  baseline : a second engine bound to the same movie factor buffer (created once, outside the timed region) runs
             set_block + alloc_factors + solve_half + read_factors on those rows
One warm-up of each, then --rounds rounds with every (size, route) interleaved; medians and minima are printed as one
JSON line with the fold-in plan of each size, the largest per-row difference between the two routes and the library's
source digest.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--queries", default="1,1024,65536")
    ap.add_argument("--users", type=int, default=480_189)
    ap.add_argument("--movies", type=int, default=17_770)
    ap.add_argument("--nnz", type=int, default=100_000_000)
    args = ap.parse_args()
    import numpy as np
    import __graft_entry__
    cfk = __graft_entry__.load_package()
    from cfk_amd import _lib

    lam = 0.05
    ds = cfk.Dataset.synthetic_netflix(args.users, args.movies, args.nnz, 0xA15, nthreads=16)
    blk = ds.shard_block(1)
    sizes = [min(int(q), blk["n_rows"]) for q in args.queries.split(",")]
    out = {"shape": [args.users, args.movies, args.nnz], "rounds": args.rounds, "results": {},
           "lib_source_sha256": _lib.lib().als_build_source_sha256().decode()}
    for k in (int(x) for x in args.ks.split(",")):
        app = cfk.ALSApp(1, k, lam, 2, precision="f32", seed=42).setup(ds, check_duplicates=False)
        app.run()
        eng = app.engine
        n_movie_rows = eng.factors[0].shape[0] - 1
        base = cfk.ALSEngine(k, "f32")
        base.bind_factors(0, eng.factors[0])
        runs, entries = {}, {}
        for nq in sizes:
            end = int(blk["row_ptr"][nq])
            q = (blk["row_ptr"][:nq + 1].copy(), blk["col"][:end].copy(), blk["ratings"][:end].copy())
            entries[nq] = end

            def fold(q=q):
                return eng.fold_in(1, q, lam)

            def baseline(q=q, nq=nq):
                base.set_block(1, q[0], q[1], q[2], 0, n_movie_rows)
                base.alloc_factors(1, nq)
                base.solve_half(1, lam)
                return base.read_factors(1, 0, nq)

            runs[f"{nq}_fold_in"] = fold
            runs[f"{nq}_baseline"] = baseline
        got = {name: fn() for name, fn in runs.items()}                 # warm-up (grows the workspace, first launches)
        times = {name: [] for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
        res = {}
        for nq in sizes:
            a, b = got[f"{nq}_fold_in"].astype(np.float64), got[f"{nq}_baseline"].astype(np.float64)
            den = np.maximum(np.linalg.norm(b, axis=1), 1e-30)
            f, s = times[f"{nq}_fold_in"], times[f"{nq}_baseline"]
            res[str(nq)] = {"entries": entries[nq], "longest_query": int(np.diff(blk["row_ptr"][:nq + 1]).max()),
                            "fold_in_ms_median": round(statistics.median(f), 3),
                            "fold_in_ms_min": round(min(f), 3), "baseline_ms_median": round(statistics.median(s), 3),
                            "baseline_ms_min": round(min(s), 3),
                            "speedup": round(statistics.median(s) / statistics.median(f), 2),
                            "max_row_difference": float(np.max(np.linalg.norm(a - b, axis=1) / den)),
                            "plan": eng.fold_in_plan(nq)}
        out["results"][str(k)] = res
        base.close()
        eng.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
