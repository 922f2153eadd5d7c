"""CPU side of als_similar (no kernel launch): the numpy restatement against the fp64 cosine, the launch plan and the
row-range check under the sanitizers, the id-to-slot helper against a dictionary, and the bindings.

tests/plan/similar_plan_check.cpp and tests/host/similar_args_check.cpp are compiled by the host C++ compiler under
AddressSanitizer + UBSan and run as programs of their own, exactly as tests/test_recommend_host.py and
tests/test_args_host.py run theirs: nothing is preloaded and no Python runs in the sanitizer run.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import similar_ref as ref
from conftest import ROOT
from test_plan_host import CSRC, FLAGS, _compilers


def _sanitized(tmp_path_factory, name, srcs, includes):
    exe = str(tmp_path_factory.mktemp(name) / name)
    inc = [x for d in includes for x in ("-I", d)]
    errors = []
    for cxx in _compilers():
        p = subprocess.run(cxx + FLAGS + inc + srcs + ["-o", exe], capture_output=True, text=True)
        if p.returncode == 0:
            break
        errors.append(" ".join(cxx) + ":\n" + p.stderr[-2000:])
    else:
        pytest.fail(f"no host compiler built {name} with the sanitizers:\n" + "\n".join(errors))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    return run.stdout


# ---------------------------------------------------------------------------------------------------------------------
# the reference is a cosine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,k", ref.CONFIGS)
def test_restatement_is_within_rounding_of_the_fp64_cosine(precision, k):
    """(k + 8) 2^-23: k rounded products and k rounded sums of half an ulp each on a unit-scale result, plus the square
    roots, the divisions and the two products."""
    T = ref.ladder_table(precision, k)
    rng = np.random.default_rng(k)
    q, c = rng.choice(ref.N_TABLE, 64, replace=False), rng.choice(ref.N_TABLE, 2000, replace=False)
    c[:8] = q[:8]                                                    # the diagonal is in it
    S = ref.similar_scores(T, q, c, "cosine")
    err = float(np.max(np.abs(S.astype(np.float64) - ref.fp64_cosine(T, q, c))))
    assert err <= (k + 8) * 2.0 ** -23, err
    assert np.max(np.abs(S)) <= 1 + 8 * 2.0 ** -23


def test_restatement_edges():
    T = np.array([[0, 0], [3, 4], [-3, -4], [6, 8], [1e-30, 0]], np.float32)
    S = ref.similar_scores(T, np.arange(5), np.arange(5), "cosine")
    assert np.all(S[0] == 0) and np.all(S[:, 0] == 0)                # a zero row scores 0 against everything
    assert S[1, 1] == 1 and S[1, 2] == -1 and S[1, 3] == 1
    assert np.all(S[4] == 0)                                         # cell(r, r) underflows to 0: inv = 0 by definition
    assert np.array_equal(ref.similar_scores(T, [1], [3, 2], "dot"), np.array([[50, -25]], np.float32))
    idx, score = ref.expected_lists(S[1:2], [1], [1, 3, 1, 2], 4)
    assert idx.tolist() == [[1, 3, -1, -1]] and score[0, 2] == -np.inf


# ---------------------------------------------------------------------------------------------------------------------
# the plan and the argument check under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_sweep_holds_every_invariant(tmp_path_factory):
    out = json.loads(_sanitized(tmp_path_factory, "similar_plan_check",
                                [os.path.join(ROOT, "tests", "plan", "similar_plan_check.cpp"),
                                 os.path.join(CSRC, "als_plan.cpp")], [CSRC]))
    assert out["cases"] == 12 * 11 * 64 * 4 * 2
    assert out["failed"] == {}
    assert out["split"] > 1000 and out["single"] > 1000


ARG_CASES = {
    "ok": "", "ok_first_and_last_row": "", "ok_no_queries": "", "ok_no_candidates": "",
    "query_negative": "als_similar: query_rows[1] = -1 is outside [0, 7)",
    "query_at_limit": "als_similar: query_rows[2] = 7 is outside [0, 7)",
    "cand_negative": "als_similar: cand_rows[2] = -3 is outside [0, 7)",
    "cand_at_limit": "als_similar: cand_rows[0] = 7 is outside [0, 7)",
    "cand_beyond_int32": "als_similar: cand_rows[1] = 8589934592 is outside [0, 7)",
    "order_query_before_cand": "als_similar: query_rows[0] = 8 is outside [0, 7)",
    "empty_table": "als_similar: query_rows[0] = 0 is outside [0, 0)",
}


def test_row_range_check(tmp_path_factory):
    out = _sanitized(tmp_path_factory, "similar_args_check",
                     [os.path.join(ROOT, "tests", "host", "similar_args_check.cpp"), os.path.join(CSRC, "als_args.cpp"),
                      os.path.join(CSRC, "als_error.cpp")], [CSRC, os.path.join(ROOT, "include")])
    got = {c["case"]: (c["status"], c["message"]) for c in map(json.loads, out.splitlines())}
    assert got == {name: (1 if msg else 0, msg) for name, msg in ARG_CASES.items()}


# ---------------------------------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------------------------------
def test_headers_declare_and_python_binds_the_calls(cfk):
    from cfk_amd import _lib
    als_h = open(os.path.join(ROOT, "include", "als.h")).read()
    assert re.search(r"^int als_similar\(als_engine\* e, int side, int metric,", als_h, flags=re.M)
    assert re.search(r"^int als_similar_plan\(const als_engine\* e,", als_h, flags=re.M)
    assert re.search(r"enum \{ ALS_SIM_COSINE = 0, ALS_SIM_DOT = 1 \};", als_h)
    assert "#define ALS_ABI_VERSION 3" in als_h                        # purely additive
    sigs = {name: args for name, _, args in _lib.SIGNATURES}
    assert len(sigs["als_similar"]) == 11 and len(sigs["als_similar_plan"]) == 5
    L = _lib.lib()
    assert L.als_similar.argtypes == sigs["als_similar"] and L.als_similar_plan.argtypes == sigs["als_similar_plan"]
    assert L.als_abi_version() == 3
    assert callable(cfk.ALSEngine.similar) and callable(cfk.ALSEngine.similar_plan)
    assert callable(cfk.ALSApp.similar_movies) and callable(cfk.ALSApp.similar_users) and callable(cfk.ids_to_slots)


# ---------------------------------------------------------------------------------------------------------------------
# raw ids -> slots
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("side", [0, 1])
def test_ids_to_slots_against_a_dictionary(cfk, tiny_path, world, side):
    ds = cfk.Dataset.load_netflix(tiny_path)
    ids = ds.ids(side)
    slot_of = dict(zip(ids.tolist(), ds.slots(side, world).tolist()))
    rng = np.random.default_rng(17 + world)
    want = np.concatenate([rng.permutation(ids)[:50], ids[:3], ids[:3]])        # shuffled, with repeats
    got = cfk.ids_to_slots(ds, side, world, want)
    assert got.dtype == np.int64 and got.tolist() == [slot_of[i] for i in want.tolist()]
    assert cfk.ids_to_slots(ds, side, world, []).shape == (0,)
    missing = int(np.setdiff1d(np.arange(ids.min(), ids.max() + 2), ids)[0])    # a gap inside the range, or max + 1
    for bad in (missing, int(ids.max()) + 7, -5):
        with pytest.raises(ValueError, match=rf"unknown {'user' if side else 'movie'} id {bad}\b"):
            cfk.ids_to_slots(ds, side, world, [int(ids[0]), bad])
