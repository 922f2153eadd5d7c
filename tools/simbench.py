#!/usr/bin/env python3
"""als_similar against the only route to the same answer without it, in ONE process with interleaved rounds.

  python tools/simbench.py [--rounds 5] [--queries-a 1024] [--top-n 10] [--nnz 100000000]

Synthetic Netflix shape (480,189 x 17,770) at k = 64, factors left from 2 iterations; the nearest movies of movies, by
cosine, self excluded. Timed, wall clock around the synchronous calls (each ends in a stream sync and includes its host
<-> device copies, which is what a caller pays):
  (a) engine.similar     --queries-a movies x all movies
  (b) engine.similar     all movies x all movies
  (c) engine.similar     8 movies (the segmented plan, S > 1)
  (d) the baseline: engine.read_factors, then a normalised matmul, numpy.argpartition and a sort on the host for (a)'s
      queries (no code under test)
  (e) the yardstick: engine.recommend with (a)'s row and candidate counts and no exclusions -- the same sweep without
      norms, scaling or the self test
  (f) (a) as a dot product: the sweep of (a) without the norm launch and the scaling, so (a) - (f) is what those cost
One warm-up of each, then --rounds rounds with the arms interleaved; medians, minima and every round are printed as one
JSON line with the plan each shape chose and the library's source digest. (a) and (d) are also checked to agree.
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
    ap.add_argument("--queries-a", type=int, default=1024)
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
    user_rows = ds.slots(1)
    na = min(args.queries_a, len(movie_rows))
    qa, q8, ua = movie_rows[:na], movie_rows[:8], user_rows[:na]

    def host_d():
        M = eng.read_factors(0)
        inv = 1.0 / np.maximum(np.linalg.norm(M, axis=1), 1e-30)
        S = (M[qa] * inv[qa, None]) @ (M[movie_rows] * inv[movie_rows, None]).T
        S[np.arange(na), np.arange(na)] = -np.inf              # position i of the candidates holds query i's row
        part = np.argpartition(-S, n - 1, axis=1)[:, :n]
        sc = np.take_along_axis(S, part, 1)
        order = np.lexsort((part, -sc), axis=1)
        return np.take_along_axis(part, order, 1).astype(np.int32), np.take_along_axis(sc, order, 1)

    runs = {"a_similar": lambda: eng.similar(0, qa, movie_rows, n),
            "b_similar_all": lambda: eng.similar(0, movie_rows, movie_rows, n),
            "c_similar_8": lambda: eng.similar(0, q8, movie_rows, n),
            "d_host_numpy": host_d,
            "e_recommend_no_excl": lambda: eng.recommend(ua, movie_rows, n),
            "f_similar_dot": lambda: eng.similar(0, qa, movie_rows, n, "dot")}
    got = {name: fn() for name, fn in runs.items()}                 # warm-up (grows the workspace, first launches)
    # the host matmul sums in another order: the neighbours agree wherever the scores are not within rounding of a tie
    ia, sa = got["a_similar"]
    id_, sd = got["d_host_numpy"]
    max_score_diff = float(np.max(np.abs(sa - sd)))
    idx_agree = float(np.mean(ia == id_))
    times = {name: [] for name in runs}
    for _ in range(args.rounds):
        for name, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"shape": [args.users, args.movies, args.nnz], "k": args.k, "top_n": n, "queries_a": na, "rounds": args.rounds,
           "ms_median": {k: round(v, 3) for k, v in med.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_rounds": {k: [round(x, 3) for x in v] for k, v in times.items()},
           "a_over_e": round(med["a_similar"] / med["e_recommend_no_excl"], 3),
           "d_over_a": round(med["d_host_numpy"] / med["a_similar"], 2),
           "a_minus_f_ms": round(med["a_similar"] - med["f_similar_dot"], 3),
           "a_vs_d_max_score_diff": max_score_diff, "a_vs_d_idx_agree": round(idx_agree, 5),
           "plans": {"a_similar": eng.similar_plan(na, len(movie_rows), n),
                     "b_similar_all": eng.similar_plan(len(movie_rows), len(movie_rows), n),
                     "c_similar_8": eng.similar_plan(8, len(movie_rows), n)},
           "lib_source_sha256": _lib.lib().als_build_source_sha256().decode()}
    print(json.dumps(out))
    return 0 if max_score_diff < 1e-4 and idx_agree > 0.99 else 1


if __name__ == "__main__":
    sys.exit(main())
