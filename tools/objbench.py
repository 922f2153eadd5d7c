#!/usr/bin/env python3
"""als_implicit_objective against the calls that read the same entries, in ONE process with interleaved rounds.

  python tools/objbench.py [--rounds 5] [--ks 64,128] [--nnz 100000000] [--alpha 40]

Synthetic Netflix shape (480,189 x 17,770), fp32, factors left from 2 explicit iterations, per k in --ks. Timed, wall
clock around the synchronous calls (each ends in a stream sync and includes its host <-> device copies, which is what a
caller pays):
  (a) implicit_objective over all users: the user side's whole CSR, x = each user's resident row
  (b) solve_implicit over the same CSR with return_host=False, into the users' own rows: the training half that reads
      the same entries (it runs last in a round, so (a) and (c) always see the rows the previous round left)
  (c) sq_error on the resident user block: the explicit yardstick, which reads the same entries once from the device
  (u) the pageable host -> device copy of the CSR arrays alone: what the upload inside (a) and (b) costs
One warm-up of each, then --rounds rounds with every arm interleaved; medians, minima and all rounds are printed as one
JSON line with the plans and the library's source digest.
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
    ap.add_argument("--users", type=int, default=480_189)
    ap.add_argument("--movies", type=int, default=17_770)
    ap.add_argument("--nnz", type=int, default=100_000_000)
    ap.add_argument("--alpha", type=float, default=40.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__
    cfk = __graft_entry__.load_package()
    from cfk_amd import _lib

    lam, alpha = 0.05, args.alpha
    ds = cfk.Dataset.synthetic_netflix(args.users, args.movies, args.nnz, 0xA15, nthreads=16)
    out = {"shape": [args.users, args.movies, args.nnz], "rounds": args.rounds, "alpha": alpha, "results": {},
           "device": torch.cuda.get_device_name(0), "lib_source_sha256": _lib.lib().als_build_source_sha256().decode()}
    for k in (int(x) for x in args.ks.split(",")):
        app = cfk.ALSApp(1, k, lam, 2, precision="f32", seed=42).setup(ds, check_duplicates=False)
        app.run()
        eng = app.engine
        row_ptr, col, rat, row_offset, n_rows = app._implicit_csr(1)
        rows = row_offset + np.arange(n_rows, dtype=np.int64)
        csr = (row_ptr, col, rat)

        def upload():
            dev = [torch.from_numpy(a).cuda() for a in csr]
            torch.cuda.synchronize()
            del dev

        runs = {"objective": lambda: eng.implicit_objective(1, csr, rows, lam, alpha),
                "sq_error": lambda: eng.sq_error("user"),
                "csr_upload": upload,
                "solve_implicit": lambda: eng.solve_implicit(1, csr, lam, alpha, dst_rows=rows, return_host=False)}
        for fn in runs.values():                                        # warm-up (grows the workspace, first launches)
            fn()
        times = {name: [] for name in runs}
        loss = None
        for _ in range(args.rounds):
            for name, fn in runs.items():
                t0 = time.perf_counter()
                r = fn()
                times[name].append(round((time.perf_counter() - t0) * 1e3, 3))
                if name == "objective":
                    loss = r["loss"]
        res = {name: {"ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_rounds": t}
               for name, t in times.items()}
        res["entries"] = int(row_ptr[-1])
        res["queries"] = int(n_rows)
        res["csr_bytes"] = int(sum(a.nbytes for a in csr))
        res["plan"] = eng.implicit_objective_plan(n_rows)
        res["solve_plan"] = eng.solve_implicit_plan(n_rows)
        res["objective_over_solve"] = round(res["objective"]["ms_median"] / res["solve_implicit"]["ms_median"], 3)
        res["last_loss"] = loss
        out["results"][str(k)] = res
        eng.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
