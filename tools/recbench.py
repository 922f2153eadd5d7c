#!/usr/bin/env python3
"""als_recommend against the only route to the same answer without it, in ONE process with interleaved rounds.

  python tools/recbench.py [--rounds 5] [--users-a 16384] [--top-n 10] [--nnz 100000000]

Synthetic Netflix shape (480,189 x 17,770) at k = 64, factors left from 2 iterations. Timed, wall clock around the
synchronous calls (each ends in a stream sync and includes its host <-> device copies, which is what a caller pays):
  (a) engine.recommend   --users-a users x all movies, top 10, seen movies excluded
  (b) the baseline: engine.predict for the same users and movies, then masking the seen movies and
      numpy.argpartition + sort on the host (no code under test)
  (c) engine.recommend   all users
  (d) engine.recommend   8 users (the segmented path, S > 1)
One warm-up of each, then --rounds rounds with (a), (b), (c), (d) interleaved; medians and minima are printed as one
JSON line with the plan each shape chose and the library's source digest. (a) and (b) are also checked to agree.
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
    ap.add_argument("--users-a", type=int, default=16_384)
    ap.add_argument("--top-n", type=int, default=10)
    ap.add_argument("--skip-all-users", action="store_true", help="leave out (c)")
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
    user_rows, ptr, idx = cfk.seen_exclusions(ds, 1, 0, movie_rows)
    na = min(args.users_a, len(user_rows))
    ua, pa, ia = user_rows[:na], ptr[:na + 1], idx[:ptr[na]]
    u8, p8, i8 = user_rows[:8], ptr[:9], idx[:ptr[8]]

    def rec_a():
        return eng.recommend(ua, movie_rows, n, (pa, ia))

    def base_b():
        P = eng.predict(ua, movie_rows)
        P[np.repeat(np.arange(na), np.diff(pa)), ia] = -np.inf
        part = np.argpartition(-P, n - 1, axis=1)[:, :n]
        sc = np.take_along_axis(P, part, 1)
        order = np.lexsort((part, -sc), axis=1)
        return np.take_along_axis(part, order, 1).astype(np.int32), np.take_along_axis(sc, order, 1)

    def rec_c():
        return eng.recommend(user_rows, movie_rows, n, (ptr, idx))

    def rec_d():
        return eng.recommend(u8, movie_rows, n, (p8, i8))

    runs = {"a_recommend": rec_a, "b_predict_host_topn": base_b, "d_recommend_8_users": rec_d}
    if not args.skip_all_users:
        runs["c_recommend_all_users"] = rec_c
    got = {name: fn() for name, fn in runs.items()}                 # warm-up (grows the workspace, first launches)
    # the baseline's argpartition breaks score ties by whatever it kept; compare the scores, and the positions wherever
    # the n-th and (n+1)-th scores differ (no tie across the cut)
    same_scores = bool(np.array_equal(got["a_recommend"][1], got["b_predict_host_topn"][1]))
    times = {name: [] for name in runs}
    for _ in range(args.rounds):
        for name, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    plans = {"a_recommend": eng.recommend_plan(na, len(movie_rows), n),
             "c_recommend_all_users": eng.recommend_plan(len(user_rows), len(movie_rows), n),
             "d_recommend_8_users": eng.recommend_plan(8, len(movie_rows), n)}
    out = {"shape": [args.users, args.movies, args.nnz], "k": args.k, "top_n": n, "users_a": na, "rounds": args.rounds,
           "ms_median": {k: round(statistics.median(v), 3) for k, v in times.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "speedup_a_over_b": round(statistics.median(times["b_predict_host_topn"]) /
                                     statistics.median(times["a_recommend"]), 2),
           "a_scores_equal_b": same_scores, "plans": {k: v for k, v in plans.items() if k in runs},
           "lib_source_sha256": _lib.lib().als_build_source_sha256().decode()}
    print(json.dumps(out))
    return 0 if same_scores and out["speedup_a_over_b"] > 1 else 1


if __name__ == "__main__":
    sys.exit(main())
