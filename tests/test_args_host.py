"""The argument unit (csrc/als_args.cpp) on the CPU: the checks of the CSR arrays that als_recommend, als_rank_targets,
als_fold_in and als_solve_implicit take, and the pointer rebase. tests/host/args_check.cpp drives each with the smallest
input that reaches a branch. It is compiled here, together with als_args.cpp and als_error.cpp, by the host C++ compiler
under AddressSanitizer + UBSan and run as a program of its own (no Python in the sanitizer run, nothing preloaded: the
sanitizer runtime is linked into the program).

The statuses and messages below are literals copied from the checks as they stood inside als_engine_solve.cpp and
als_engine_query.cpp before they moved, so sharing more between them than was the same (the text, or which of two
faults is reported first) shows here, in milliseconds, without a GPU.
"""
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "collaborative-filtering-kafka_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
OK, INVALID = 0, 1   # ALS_OK, ALS_ERR_INVALID_ARGUMENT (include/als.h)


def _compilers():
    """Host C++ compilers to try: ROCm's clang++ (hipcc's host compiler; links the sanitizer runtimes statically),
    then g++ (told to link them statically too, so the program runs the same whatever else the loader brings in)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")
    if os.path.exists(clang):
        yield [clang]
    gxx = shutil.which("g++")
    if gxx:
        yield [gxx, "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("args") / "args_check")
    srcs = [os.path.join(ROOT, "tests", "host", "args_check.cpp"), os.path.join(CSRC, "als_args.cpp"),
            os.path.join(CSRC, "als_error.cpp")]
    errors = []
    for cxx in _compilers():
        p = subprocess.run(cxx + FLAGS + ["-I", CSRC, "-I", os.path.join(ROOT, "include")] + srcs + ["-o", exe],
                           capture_output=True, text=True)
        if p.returncode == 0:
            break
        errors.append(" ".join(cxx) + ":\n" + p.stderr[-2000:])
    else:
        pytest.fail("no host compiler built args_check with the sanitizers:\n" + "\n".join(errors))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    # a sanitizer report goes to stderr and fails the run (UBSan does not recover, ASan exits non-zero)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    out = [json.loads(line) for line in run.stdout.splitlines()]
    assert len({c["case"] for c in out}) == len(out)
    return {c.pop("case"): c for c in out}


def test_args_unit_includes_no_hip_header():
    """Only als.h, als_error.h and the standard library: what lets the unit build and run without ROCm."""
    for name in ("als_args.h", "als_args.cpp"):
        src = open(os.path.join(CSRC, name)).read()
        own = set(re.findall(r'#include\s*"([^"]+)"', src))
        assert own <= {"als.h", "als_error.h", "als_args.h"}, (name, own)
        assert not [h for h in re.findall(r"#include\s*<([^>]+)>", src) if "hip" in h or "/" in h], name


# case -> (status, message): the parent's text, with the call, array and owner names args_check passes
FAILURES = {
    "walk_negative_first": "als_fold_in: q_ptr[0] is negative",
    "walk_decrease_at_1": "als_fold_in: q_ptr decreases at query 1",
    "walk_count_2p31": "als_fold_in: the number of entries must be below 2^31",
    "queries_count_2p31": "als_fold_in: the number of entries must be below 2^31",
    "targets_count_2p31": "als_rank_targets: the number of targets must be below 2^31",
    "targets_decrease_at_1": "als_rank_targets: tgt_ptr decreases at user 1",
    "index_negative": "als_solve_implicit: index -1 of query 1 is outside [0, 7)",
    "index_at_limit": "als_solve_implicit: index 7 of query 0 is outside [0, 7)",
    "dst_negative": "als_solve_implicit: dst_rows[1] = -1 of query 1 is outside [0, 5)",
    "dst_at_limit": "als_solve_implicit: dst_rows[0] = 5 of query 0 is outside [0, 5)",
    "dst_repeat": "als_solve_implicit: dst_rows repeats row 3 at query 2",
    "excl_negative_first": "als_recommend: excl_ptr[0] is negative",
    "excl_decrease": "als_recommend: excl_ptr decreases at user 1",
    "excl_unsorted": "als_recommend: excluded positions of user 1 are not strictly ascending",
    "excl_duplicate": "als_recommend: excluded positions of user 0 are not strictly ascending",
    "excl_position_negative": "als_recommend: excluded position -1 of user 1 is outside [0, 50)",
    "excl_position_at_limit": "als_recommend: excluded position 50 of user 0 is outside [0, 50)",
    # of two faults, the one the parent reported
    "order_pointer_before_index": "als_solve_implicit: q_ptr decreases at query 1",
    "order_position_before_pointer": "als_recommend: excluded position 50 of user 0 is outside [0, 50)",
}
# case -> what it returns beside ALS_OK
PASSES = {
    "walk_ok": {"count": 7},
    "walk_no_owners": {"count": 0},
    "walk_count_2p31_minus_1": {"count": 2**31 - 1},
    "queries_ok": {"count": 3},           # the entry before q_ptr[0] is out of range and never looked at
    "queries_no_dst": {"count": 1},
    "excl_ok": {},
    "excl_empty_ranges": {},
    # the three entries before excl_ptr[0] = 3 were poisoned while the check and the rebase ran
    "excl_slice_at_3": {"poisoned": 3, "rebased": [0, 2, 3]},
    "rebase_at_0": {"same_pointer": 1, "store_size": 0},
    "rebase_at_3": {"same_pointer": 0, "in_store": 1, "rebased": [0, 2, 2, 7]},   # the n + 1-th entry included
    "rebase_no_owners": {"rebased": [0]},
}


def test_every_case_ran(cases):
    assert sorted(cases) == sorted(list(FAILURES) + list(PASSES))


@pytest.mark.parametrize("name", sorted(FAILURES))
def test_failure_status_and_text(cases, name):
    assert cases[name] == {"status": INVALID, "message": FAILURES[name]}


@pytest.mark.parametrize("name", sorted(PASSES))
def test_pass_and_result(cases, name):
    assert cases[name] == dict(PASSES[name], status=OK, message="")
