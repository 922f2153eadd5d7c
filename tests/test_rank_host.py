"""CPU side of als_rank_targets (no kernel launch): the launch plan under the sanitizers, the held-out query builder
against a brute-force dictionary, the ranking metrics against hand-computed answers, and the bindings.

tests/plan/rank_plan_check.cpp sweeps cfk::rank_plan over (n_targets 1..2^21, n_cand 1..2^21, kp in {16, 64, 128, 1024},
cu_count in {1, 256}). It is compiled with als_plan.cpp by the host C++ compiler under AddressSanitizer + UBSan and run
as a program of its own, exactly as tests/test_recommend_host.py runs recommend_plan_check: nothing is preloaded and no
Python runs in the sanitizer run.
"""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_plan_host import CSRC, FLAGS, _compilers


@pytest.fixture(scope="module")
def plan_sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rankplan") / "rank_plan_check")
    srcs = [os.path.join(ROOT, "tests", "plan", "rank_plan_check.cpp"), os.path.join(CSRC, "als_plan.cpp")]
    errors = []
    for cxx in _compilers():
        p = subprocess.run(cxx + FLAGS + ["-I", CSRC] + srcs + ["-o", exe], capture_output=True, text=True)
        if p.returncode == 0:
            break
        errors.append(" ".join(cxx) + ":\n" + p.stderr[-2000:])
    else:
        pytest.fail("no host compiler built rank_plan_check with the sanitizers:\n" + "\n".join(errors))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    return json.loads(run.stdout)


def test_plan_sweep_holds_every_invariant(plan_sweep):
    """Segments tile [0, n_cand) exactly with no overlap, all but the last are whole candidate tiles, 1 <= S <= 65535,
    LDS <= 160 KiB, the workspace arithmetic does not overflow int64 (UBSan would also stop the program), S = 1 whenever
    the target tiles alone reach cu_count."""
    assert plan_sweep["cases"] == 14 * 11 * 4 * 2
    assert plan_sweep["failed"] == {}
    assert plan_sweep["split"] > 100 and plan_sweep["single"] > 100       # both launch shapes are in the sweep


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("chunks", [1, 4])
def test_heldout_queries_against_a_dictionary(cfk, tiny_path, world, chunks):
    ds = cfk.Dataset.load_netflix(tiny_path)
    ds.set_slot_chunks(1, chunks)
    m, u, _ = ds.ratings()
    movie_ids, user_ids = ds.ids(0), ds.ids(1)
    movie_slots = ds.slots(0, world)
    slot_of_movie = dict(zip(movie_ids.tolist(), movie_slots.tolist()))
    rated = set(zip(u.tolist(), m.tolist()))
    rng = np.random.default_rng(5)
    # a shuffled candidate subset (so some movies fall outside it) with a few slots listed twice
    cand = rng.permutation(movie_slots)[: len(movie_slots) * 2 // 3]
    cand = np.concatenate([cand, cand[:7]])
    first_pos = {}
    for c, s in enumerate(cand.tolist()):
        first_pos.setdefault(s, c)
    # held-out pairs: random (movie, user) pairs -- some of them training ratings --, unknown ids, exact repeats
    n = 900
    pm = rng.choice(movie_ids, n)
    pu = rng.choice(user_ids, n)
    pm[:60], pu[:60] = m[:60], u[:60]                                  # training ratings
    pm[100:105] = movie_ids.max() + 1 + np.arange(5)                   # unknown movies
    pu[200:204] = user_ids.max() + 3 + np.arange(4)                    # unknown users
    pm[300:310], pu[300:310] = pm[310:320], pu[310:320]                # the same pair twice
    covered = 0
    for rank in range(world):
        tgt_ptr, tgt_idx, entry, seen, n_unknown, n_seen = cfk.heldout_queries(ds, pm, pu, world, rank, cand)
        mine = user_ids[user_ids % world == rank]                      # local-row order = ascending raw id
        assert tgt_ptr.dtype == np.int64 and tgt_idx.dtype == np.int32 and entry.dtype == np.int64 and seen.dtype == bool
        assert len(tgt_ptr) == len(mine) + 1 and tgt_ptr[0] == 0 and tgt_ptr[-1] == len(tgt_idx) == len(entry) == len(seen)
        want = {int(uid): [] for uid in mine}
        unknown = 0
        for i in range(n):
            if world > 1 and int(pu[i]) % world != rank:
                continue
            if int(pu[i]) not in want or int(pm[i]) not in slot_of_movie or slot_of_movie[int(pm[i])] not in first_pos:
                unknown += 1
                continue
            want[int(pu[i])].append((first_pos[slot_of_movie[int(pm[i])]], i, (int(pu[i]), int(pm[i])) in rated))
        for li, uid in enumerate(mine.tolist()):
            sl = slice(tgt_ptr[li], tgt_ptr[li + 1])
            got = list(zip(tgt_idx[sl].tolist(), entry[sl].tolist(), seen[sl].tolist()))
            assert got == want[uid], (rank, uid)
        assert n_unknown == unknown and unknown > 0
        assert n_seen == int(seen.sum()) == sum(s for v in want.values() for _, _, s in v) and n_seen > 0
        covered += len(entry) + n_unknown
    assert covered == n                                                # every pair belongs to exactly one rank


def test_ranking_metrics_by_hand(cfk):
    got = cfk.ranking_metrics(np.array([0, 1, 9, 10, 99], np.int32), 101, 10)
    assert got["n_ranked"] == 5
    assert got["hr"] == pytest.approx(0.6, rel=1e-14)
    assert got["ndcg"] == pytest.approx((1 + 1 / math.log2(3) + 1 / math.log2(11)) / 5, rel=1e-14)
    assert got["mrr"] == pytest.approx((1 + 1 / 2 + 1 / 10 + 1 / 11 + 1 / 100) / 5, rel=1e-14)
    assert got["mpr"] == pytest.approx((0 + 1 + 9 + 10 + 99) / 100 / 5, rel=1e-14)
    assert got["hr_sum"] == 3 and got["mrr_sum"] == pytest.approx(got["mrr"] * 5, rel=1e-14)
    # per-target eligible counts, and a user with one eligible candidate (rank 0 of 1: percentile 0, no division by 0)
    got = cfk.ranking_metrics(np.array([0, 4]), np.array([1, 9]), 1)
    assert got["mpr"] == pytest.approx((0 / 1 + 4 / 8) / 2, rel=1e-14) and got["hr"] == 0.5 and got["ndcg"] == 0.5
    empty = cfk.ranking_metrics(np.zeros(0, np.int32), np.zeros(0), 10)
    assert empty["n_ranked"] == 0 and empty["hr_sum"] == 0 and math.isnan(empty["hr"])


def test_headers_declare_and_python_binds_the_calls(cfk):
    from cfk_amd import _lib
    als_h = open(os.path.join(ROOT, "include", "als.h")).read()
    assert re.search(r"^int als_rank_targets\(als_engine\* e,", als_h, flags=re.M)
    assert re.search(r"^int als_rank_plan\(const als_engine\* e,", als_h, flags=re.M)
    assert "#define ALS_ABI_VERSION 3" in als_h                        # purely additive
    sigs = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sigs["als_rank_targets"]) == 11 and len(sigs["als_rank_plan"]) == 4
    L = _lib.lib()
    assert L.als_rank_targets.argtypes == sigs["als_rank_targets"] and L.als_rank_plan.argtypes == sigs["als_rank_plan"]
    assert callable(cfk.ALSEngine.rank_targets) and callable(cfk.ALSEngine.rank_plan)
    assert callable(cfk.ALSApp.evaluate) and callable(cfk.heldout_queries) and callable(cfk.ranking_metrics)
