#!/usr/bin/env python3
"""als_rank_targets against its yardstick and against the only route to the same ranks without it, in ONE process with
interleaved rounds.

  python tools/evalbench.py [--rounds 5] [--targets 16384] [--top-n 10] [--nnz 100000000]

Synthetic Netflix shape (480,189 x 17,770) at k = 64, factors left from 2 iterations. One held-out target (a seeded
random movie position) for each of the first --targets users. Timed, wall clock around the synchronous calls (each ends
in a stream sync and includes its host <-> device copies, which is what a caller pays):
  (a) engine.rank_targets  --targets targets x all movies, seen movies excluded: exact scores and ranks
  (b) the yardstick: engine.recommend top 10 for the same users and exclusions -- the same scoring loop, and selecting
      the best N is strictly more work than counting what comes before one threshold
  (c) the baseline: engine.predict for the same users and movies, then the ranks in numpy on the host (no code under
      test)
  (d) engine.rank_targets with ranks=False: the scores alone (the held-out RMSE path)
One warm-up of each, then --rounds rounds with (a), (b), (c), (d) interleaved; medians and minima are printed as one JSON
line with the plan each call chose and the library's source digest. (a) and (c) are also checked to agree exactly.
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
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--users", type=int, default=480_189)
    ap.add_argument("--movies", type=int, default=17_770)
    ap.add_argument("--nnz", type=int, default=100_000_000)
    ap.add_argument("--targets", type=int, default=16_384)
    ap.add_argument("--top-n", type=int, default=10)
    args = ap.parse_args()
    import numpy as np
    import __graft_entry__
    cfk = __graft_entry__.load_package()
    from cfk_amd import _lib

    ds = cfk.Dataset.synthetic_netflix(args.users, args.movies, args.nnz, 0xA15, nthreads=16)
    app = cfk.ALSApp(1, args.k, 0.05, 2, precision="f32", seed=42).setup(ds, check_duplicates=False)
    app.run()
    eng = app.engine
    n = args.top_n
    movie_rows = ds.slots(0)
    nm = len(movie_rows)
    user_rows, ptr, idx = cfk.seen_exclusions(ds, 1, 0, movie_rows)
    na = min(args.targets, len(user_rows))
    ua, pa, ia = user_rows[:na], ptr[:na + 1], idx[:ptr[na]]
    tgt = np.random.default_rng(7).integers(0, nm, na).astype(np.int32)
    targets = (np.arange(na + 1, dtype=np.int64), tgt)

    def rank_a():
        return eng.rank_targets(ua, movie_rows, targets, (pa, ia))

    def rec_b():
        return eng.recommend(ua, movie_rows, n, (pa, ia))

    def base_c():
        P = eng.predict(ua, movie_rows)
        s = P[np.arange(na), tgt][:, None]
        before = P > s
        before |= (P == s) & (np.arange(nm)[None, :] < tgt[:, None])
        before[np.repeat(np.arange(na), np.diff(pa)), ia] = False
        return s[:, 0], np.count_nonzero(before, axis=1).astype(np.int32)

    def score_d():
        return eng.rank_targets(ua, movie_rows, targets, None, ranks=False)

    runs = {"a_rank_targets": rank_a, "b_recommend": rec_b, "c_predict_host_ranks": base_c, "d_scores_only": score_d}
    got = {name: fn() for name, fn in runs.items()}                 # warm-up (grows the workspace, first launches)
    same = bool(np.array_equal(got["a_rank_targets"][0], got["c_predict_host_ranks"][0]) and
                np.array_equal(got["a_rank_targets"][1], got["c_predict_host_ranks"][1]) and
                np.array_equal(got["d_scores_only"][0], got["a_rank_targets"][0]))
    times = {name: [] for name in runs}
    for _ in range(args.rounds):
        for name, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"shape": [args.users, args.movies, args.nnz], "k": args.k, "top_n": n, "targets": na, "rounds": args.rounds,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_all": {k: [round(x, 3) for x in v] for k, v in times.items()},
           "a_over_b": round(med["a_rank_targets"] / med["b_recommend"], 3),
           "speedup_a_over_c": round(med["c_predict_host_ranks"] / med["a_rank_targets"], 2),
           "a_equals_c": same, "excluded_entries": int(pa[na]),
           "plans": {"a_rank_targets": eng.rank_plan(na, nm), "b_recommend": eng.recommend_plan(na, nm, n)},
           "lib_source_sha256": _lib.lib().als_build_source_sha256().decode()}
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
