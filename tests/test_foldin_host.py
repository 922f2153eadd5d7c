"""CPU side of als_fold_in (no kernel launch): the launch plan under the sanitizers, the query builder against a
brute-force dictionary, and the bindings.

tests/plan/foldin_plan_check.cpp sweeps cfk::foldin_plan over every kp (16, 32, 64, 128), both element sizes, cu_count in
{1, 8, 256} and n_queries from 1 to 10^7. It is compiled with als_plan.cpp by the host C++ compiler under
AddressSanitizer + UBSan and run as a program of its own, exactly as tests/test_recommend_host.py runs
recommend_plan_check: nothing is preloaded and no Python runs in the sanitizer run.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_plan_host import CSRC, FLAGS, _compilers

LDS_LIMIT = 160 * 1024


def foldin_plan(kp: int, elem_bytes: int, n_queries: int, cu_count: int) -> dict:
    """foldin_plan of als_plan.cpp restated: the dynamic LDS is the Gram's lower-triangle tiles (16 rows of pitch 17),
    `batch` staged rows of pitch kp + 16 (kp itself where that is 16 mod 32 already: 16, 80, 112), four kp-vectors and
    the batch's ratings; the batch is the largest multiple of 4 up to 64 that fits 160 KiB; the grid is what the compute
    units hold at that LDS size (at most 8 workgroups each), never more than the queries."""
    tiles = (kp // 16) * (kp // 16 + 1) // 2
    pitch = kp if kp % 32 == 16 else kp + 16

    def lds(batch):
        return elem_bytes * (tiles * 16 * 17 + batch * pitch + 4 * kp + batch)

    batch = 64
    while batch > 4 and lds(batch) > LDS_LIMIT:
        batch -= 4
    per_cu = min(8, max(1, LDS_LIMIT // lds(batch)))
    return {"threads": 256, "workgroups": max(1, min(n_queries, per_cu * max(1, cu_count))), "batch": batch,
            "lds_bytes": lds(batch)}


@pytest.fixture(scope="module")
def plan_sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("foldplan") / "foldin_plan_check")
    srcs = [os.path.join(ROOT, "tests", "plan", "foldin_plan_check.cpp"), os.path.join(CSRC, "als_plan.cpp")]
    errors = []
    for cxx in _compilers():
        p = subprocess.run(cxx + FLAGS + ["-I", CSRC] + srcs + ["-o", exe], capture_output=True, text=True)
        if p.returncode == 0:
            break
        errors.append(" ".join(cxx) + ":\n" + p.stderr[-2000:])
    else:
        pytest.fail("no host compiler built foldin_plan_check with the sanitizers:\n" + "\n".join(errors))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    generic = subprocess.run([exe, "generic"], capture_output=True, text=True, timeout=120)
    assert generic.returncode == 0 and generic.stderr == "", generic.stderr[-4000:]
    return dict(json.loads(run.stdout), generic=json.loads(generic.stdout))


def test_plan_sweep_holds_every_invariant(plan_sweep):
    """LDS <= 163,840 B and exactly what the kernel lays out, batch >= 4 and a multiple of 4, 1 <= grid <= n_queries, the
    staged rows 16-byte aligned with a conflict-free pitch: for every kp, both element sizes, n_queries 1 .. 10^7."""
    n_queries = 70 + 6 * 3 + 14
    assert plan_sweep["cases"] == 4 * 2 * 3 * n_queries
    assert plan_sweep["failed"] == {}
    assert len(plan_sweep["plans"]) == plan_sweep["cases"]
    assert any(key.endswith("/10000000/256") for key in plan_sweep["plans"])


def test_python_restatement_equals_the_plan(plan_sweep):
    seen = set()
    for key, (threads, grid, batch, lds) in plan_sweep["plans"].items():
        kp, elem, nq, cu = (int(x) for x in key.split("/"))
        assert foldin_plan(kp, elem, nq, cu) == {"threads": threads, "workgroups": grid, "batch": batch,
                                                 "lds_bytes": lds}, key
        seen.add((kp, elem))
    assert seen == {(kp, elem) for kp in (16, 32, 64, 128) for elem in (4, 8)}
    # the shapes DESIGN.md section 3.9 quotes
    assert foldin_plan(128, 8, 10 ** 7, 256) == {"threads": 256, "workgroups": 256, "batch": 64, "lds_bytes": 156672}
    assert foldin_plan(64, 4, 5000, 256) == {"threads": 256, "workgroups": 1280, "batch": 64, "lds_bytes": 32640}


def test_plan_of_the_fp64_strides_between_64_and_128(plan_sweep):
    """fp64 engines of 65..112 features are on the generic solve path, whose factor stride is the next multiple of 16:
    80, 96 or 112. als_fold_in serves them too (als.h: every stride <= 128 in both precisions); the same invariants
    hold for their plans, and the restatement equals them."""
    g = plan_sweep["generic"]
    n_queries = 70 + 6 * 3 + 14
    assert g["cases"] == 3 * 3 * n_queries == len(g["plans"]) and g["failed"] == {}
    for key, (threads, grid, batch, lds) in g["plans"].items():
        kp, elem, nq, cu = (int(x) for x in key.split("/"))
        assert elem == 8 and kp in (80, 96, 112) and batch == 64
        assert foldin_plan(kp, elem, nq, cu) == {"threads": threads, "workgroups": grid, "batch": batch,
                                                 "lds_bytes": lds}, key
    assert foldin_plan(112, 8, 22, 256) == {"threads": 256, "workgroups": 22, "batch": 64, "lds_bytes": 122368}


@pytest.mark.parametrize("world", [1, 2])
def test_foldin_queries_against_a_dictionary(cfk, tiny_path, world):
    ds = cfk.Dataset.load_netflix(tiny_path)
    movie_ids = ds.ids(0)
    movie_slots = ds.slots(0, world)
    slot_of_movie = dict(zip(movie_ids.tolist(), movie_slots.tolist()))
    rng = np.random.default_rng(11)
    # a shuffled candidate subset (so some rated movies fall outside it) with a few slots listed twice
    cand = rng.permutation(movie_slots)[: len(movie_slots) * 3 // 4]
    cand = np.concatenate([cand, cand[:5]])
    positions = {}
    for c, s in enumerate(cand.tolist()):
        positions.setdefault(s, []).append(c)
    unknown_id = int(movie_ids.max()) + 7
    users = []
    for u in range(9):
        ms = rng.choice(movie_ids, size=3 + 4 * u, replace=False).tolist()
        users.append([(int(m), int(rng.integers(1, 6))) for m in ms])
    users[2].insert(1, (unknown_id, 4))                       # an unknown movie id inside a list
    users[4].append(users[4][0])                              # the same movie twice: counts twice, excluded once
    users.append([(unknown_id, 5), (unknown_id + 1, 1)])      # a user with no known movie
    users.append([])                                          # a user with no rating at all
    q_ptr, q_idx, q_rat, excl_ptr, excl_idx, n_unknown = cfk.foldin_queries(ds, world, cand, users)
    assert q_ptr.dtype == np.int64 and q_idx.dtype == np.int32 and q_rat.dtype == np.int16
    assert excl_ptr.dtype == np.int64 and excl_idx.dtype == np.int32
    assert len(q_ptr) == len(excl_ptr) == len(users) + 1 and q_ptr[0] == 0 and excl_ptr[0] == 0
    assert q_ptr[-1] == len(q_idx) == len(q_rat) and excl_ptr[-1] == len(excl_idx)
    unknown = 0
    for i, pairs in enumerate(users):
        want = [(slot_of_movie[m], r) for m, r in pairs if m in slot_of_movie]
        unknown += len(pairs) - len(want)
        sl = slice(q_ptr[i], q_ptr[i + 1])
        assert list(zip(q_idx[sl].tolist(), q_rat[sl].tolist())) == want, i
        want_excl = sorted({c for s, _ in want for c in positions.get(s, [])})
        assert excl_idx[excl_ptr[i]:excl_ptr[i + 1]].tolist() == want_excl, i
    assert n_unknown == unknown == 3
    assert q_ptr[-2] == q_ptr[-3] == q_ptr[-1]                # the two users without a known movie: empty ranges
    assert any(len(positions.get(s, [])) == 2 for s in q_idx.tolist())    # a twice-listed slot was exercised
    assert any(s not in positions for s in q_idx.tolist())                # and a rated movie outside the candidates


def test_headers_declare_and_python_binds_the_calls(cfk):
    from cfk_amd import _lib
    als_h = open(os.path.join(ROOT, "include", "als.h")).read()
    assert re.search(r"^int als_fold_in\(als_engine\* e, int side, int64_t n_queries,", als_h, flags=re.M)
    assert re.search(r"^int als_fold_in_plan\(const als_engine\* e, int64_t n_queries, int64_t info\[4\]\);", als_h,
                     flags=re.M)
    assert "#define ALS_ABI_VERSION 3" in als_h                        # purely additive
    sigs = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sigs["als_fold_in"]) == 10 and len(sigs["als_fold_in_plan"]) == 3
    L = _lib.lib()
    assert L.als_fold_in.argtypes == sigs["als_fold_in"] and L.als_fold_in_plan.argtypes == sigs["als_fold_in_plan"]
    assert L.als_abi_version() == 3
    assert callable(cfk.ALSEngine.fold_in) and callable(cfk.ALSEngine.fold_in_plan)
    assert callable(cfk.ALSApp.fold_in) and callable(cfk.ALSApp.recommend_for) and callable(cfk.foldin_queries)
