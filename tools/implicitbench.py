#!/usr/bin/env python3
"""als_gram_table and als_solve_implicit against als_fold_in, in ONE process with interleaved rounds.

  python tools/implicitbench.py [--rounds 5] [--ks 64,128] [--queries 1,1024,65536] [--nnz 100000000] [--alpha 40]

Synthetic Netflix shape (480,189 x 17,770), fp32, factors left from 2 explicit iterations, per k in --ks. Timed, wall
clock around the synchronous calls (each ends in a stream sync and includes its host <-> device copies, which is what a
caller pays):
  (a) gram_table of M and of U alone
  (b) solve_implicit for the in-blocks of the first 1, 1,024 and 65,536 users against fold_in on the same queries:
      explicit fold-in is the same gather and solve without G and the weights
  (c) one full implicit_iteration (after one untimed iteration that takes the host CSR), and the pageable host -> device
      copy of both sides' CSR arrays alone -- what the per-half upload inside solve_implicit costs
One warm-up of each, then --rounds rounds with every route interleaved; medians and minima are printed as one JSON line
with the plans and the library's source digest.
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
    ap.add_argument("--alpha", type=float, default=40.0)
    args = ap.parse_args()
    import torch
    import __graft_entry__
    cfk = __graft_entry__.load_package()
    from cfk_amd import _lib

    lam, alpha = 0.05, args.alpha
    ds = cfk.Dataset.synthetic_netflix(args.users, args.movies, args.nnz, 0xA15, nthreads=16)
    blk = ds.shard_block(1)
    sizes = [min(int(q), blk["n_rows"]) for q in args.queries.split(",")]
    out = {"shape": [args.users, args.movies, args.nnz], "rounds": args.rounds, "alpha": alpha, "results": {},
           "device": torch.cuda.get_device_name(0), "lib_source_sha256": _lib.lib().als_build_source_sha256().decode()}
    for k in (int(x) for x in args.ks.split(",")):
        app = cfk.ALSApp(1, k, lam, 2, precision="f32", seed=42).setup(ds, check_duplicates=False)
        app.run()
        eng = app.engine
        runs = {"gram_M": lambda: eng.gram_table(0), "gram_U": lambda: eng.gram_table(1)}
        entries = {}
        for nq in sizes:
            end = int(blk["row_ptr"][nq])
            q = (blk["row_ptr"][:nq + 1].copy(), blk["col"][:end].copy(), blk["ratings"][:end].copy())
            entries[nq] = end
            runs[f"{nq}_implicit"] = lambda q=q: eng.solve_implicit(1, q, lam, alpha)
            runs[f"{nq}_fold_in"] = lambda q=q: eng.fold_in(1, q, lam)
        for fn in runs.values():                                        # warm-up (grows the workspace, first launches)
            fn()
        times = {name: [] for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)

        def stat(name):
            return {"ms_median": round(statistics.median(times[name]), 3), "ms_min": round(min(times[name]), 3)}

        n_m, n_u = eng.factors[0].shape[0] - 1, eng.factors[1].shape[0] - 1
        res = {"gram_M": dict(stat("gram_M"), rows=n_m, plan=eng.gram_table_plan(n_m)),
               "gram_U": dict(stat("gram_U"), rows=n_u, plan=eng.gram_table_plan(n_u))}
        for nq in sizes:
            i, f = stat(f"{nq}_implicit"), stat(f"{nq}_fold_in")
            res[str(nq)] = {"entries": entries[nq],
                            "longest_query": int((blk["row_ptr"][1:nq + 1] - blk["row_ptr"][:nq]).max()),
                            "implicit": i, "fold_in": f, "implicit_over_fold_in": round(i["ms_median"] / f["ms_median"], 2),
                            "plan": eng.solve_implicit_plan(nq)}
        # (c) the whole iteration; the first one takes both sides' host CSR and is not timed
        app.implicit_iteration(alpha)
        it, up = [], []
        csr = [a for side in (0, 1) for a in app._implicit_csr(side)[:3]]
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            app.implicit_iteration(alpha)
            it.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            dev = [torch.from_numpy(a).cuda() for a in csr]
            torch.cuda.synchronize()
            up.append((time.perf_counter() - t0) * 1e3)
            del dev
        res["iteration"] = {"ms_median": round(statistics.median(it), 3), "ms_min": round(min(it), 3),
                            "csr_bytes": int(sum(a.nbytes for a in csr)),
                            "csr_upload_ms_median": round(statistics.median(up), 3),
                            "csr_upload_share": round(statistics.median(up) / statistics.median(it), 3)}
        out["results"][str(k)] = res
        eng.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
