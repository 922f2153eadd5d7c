"""The work plan of a block (csrc/als_plan.cpp) on the CPU: tests/plan/plan_check.cpp builds the plans of small
synthetic blocks, checks their invariants from the plan alone and hashes every output array. It is compiled here,
together with als_plan.cpp, by the host C++ compiler under AddressSanitizer + UBSan and run as a program of its own
(no Python in the sanitizer run, nothing preloaded: the sanitizer runtime is linked into the program).

tests/golden/plan_digests.json pins the FNV-1a digest of every case. It was written from the plan arithmetic as it
stood inside als_engine.cpp's finish_block before it moved to als_plan.cpp, so a clean-up of the plan that changes any
task, slot, permutation entry or layout decision shows here, in milliseconds, without a GPU.
"""
import json
import os
import shutil
import subprocess

import pytest

import rowshapes as rs
from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "collaborative-filtering-kafka_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


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
def plan_cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    srcs = [os.path.join(ROOT, "tests", "plan", "plan_check.cpp"), os.path.join(CSRC, "als_plan.cpp")]
    errors = []
    for cxx in _compilers():
        p = subprocess.run(cxx + FLAGS + ["-I", CSRC] + srcs + ["-o", exe], capture_output=True, text=True)
        if p.returncode == 0:
            break
        errors.append(" ".join(cxx) + ":\n" + p.stderr[-2000:])
    else:
        pytest.fail("no host compiler built plan_check with the sanitizers:\n" + "\n".join(errors))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    # a sanitizer report goes to stderr and fails the run (UBSan does not recover, ASan exits non-zero)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    cases = [json.loads(line) for line in run.stdout.splitlines()]
    assert len({c["case"] for c in cases}) == len(cases)
    return {c["case"]: c for c in cases}


def test_every_case_holds_every_invariant(plan_cases):
    """perm a row-wise block permutation, every block covered once with exact nent, unique PARTIAL slots, one REDUCE
    per split row tiling the slots, lists longest first, consistent XCD queues, entry-space rows qualifying, sq_all
    complete, the chunk partition stable: one boolean per invariant and case, computed by plan_check from the plan."""
    assert len(plan_cases) >= 30
    failed = {name: [k for k, ok in c["checks"].items() if not ok]
              for name, c in plan_cases.items() if "checks" in c and not all(c["checks"].values())}
    assert not failed, failed
    assert not [name for name, c in plan_cases.items() if "error" in c]
    for name, c in plan_cases.items():
        if "checks" in c:
            assert len(c["checks"]) >= 14, (name, c["checks"])
            # a plan dealt into XCD queues gets the range checks, an aligned one the position checks on top
            assert len(c["checks"]) == 14 + (3 if c["queues"] else 0) + (2 if c["queues_aligned"] else 0), name


def test_xcd_queue_cases_are_aligned(plan_cases):
    """The position checks (workgroup w = queue w % 8, longest first per queue, chunk tasks in their range's queue)
    apply where the dealing promises the alignment: a task count that fills the last workgroup and no range with more
    chunk tasks than its share. The forced-ranges cases at kp 64 and kp 128 are built to be such plans; plans whose
    tail shifts (speed only) keep the position-free range checks."""
    for name in ("ilv_kp64_ranges", "ilv_kp128_ranges", "auto_ranges_128mib_at"):
        c = plan_cases[name]
        assert c["queues"] and c["queues_aligned"], name
        assert c["checks"]["queue_positions_longest_first"] and c["checks"]["chunk_tasks_in_their_range_queue"]
    assert any(c.get("queues") and not c["queues_aligned"] for c in plan_cases.values())


# Layout decisions either side of each measured threshold (als_plan.cpp: plan_layout), and of the forced cases.
LAYOUTS = {
    # no interleave without the pre-split Gram (VALU, f32 MFMA, kp 32) or on the generic path
    "valu_kp16": dict(chunk=64, ilv=0, ranges=0, presplit=0),
    "mfma_kp32": dict(chunk=64, ilv=0, ranges=0, presplit=0),
    "split_kp32": dict(chunk=64, ilv=0, ranges=0, presplit=0),
    "generic_k130": dict(chunk=64, ilv=0, ranges=0, presplit=0),
    "split_kp64_default_chunk": dict(chunk=1024, ilv=0, ranges=0, presplit=1),
    "ilv_kp64_noranges": dict(chunk=64, ilv=64, ranges=0, presplit=1),
    "ilv_kp64_ranges": dict(chunk=64, ilv=64, ranges=1, presplit=1),
    "ilv_kp128_noranges": dict(chunk=128, ilv=128, ranges=0, presplit=1),
    "ilv_kp128_ranges": dict(chunk=128, ilv=128, ranges=1, presplit=1),
    "ilv_kp64_presplit_off": dict(chunk=64, ilv=64, ranges=1, presplit=0),
    "ilv_kp64_ilv32_chunk64": dict(chunk=64, ilv=32, ranges=1, presplit=1),
    "ilv_off_kp128": dict(chunk=64, ilv=0, ranges=0, presplit=1),
    # auto: interleave for tables of more than 32 MB up to 256 MiB
    "auto_table_32mb_at": dict(ilv=0, ranges=0, presplit=0),
    "auto_table_32mb_over": dict(ilv=1024, ranges=1, presplit=1),
    "auto_table_256mib_at_kp64": dict(ilv=1024, ranges=0, presplit=1),
    "auto_table_256mib_over_kp64": dict(ilv=0, ranges=0, presplit=0),
    "auto_table_256mib_at_kp128": dict(ilv=1024, presplit=1),
    "auto_table_256mib_over_kp128": dict(ilv=0, presplit=1),
    # kp 64, table within 128 MiB: only with 1.5 x the resident waves of chunks
    "auto_concurrency_kp64_at": dict(ilv=1024, ranges=1, presplit=1),
    "auto_concurrency_kp64_under": dict(ilv=0, ranges=0, presplit=0),
    "auto_concurrency_kp64_big_table": dict(ilv=1024, ranges=0, presplit=1),
    # kp 128: 16,384 or 4,096
    "auto_kp128_len_at": dict(chunk=32768, ilv=16384, ranges=0, presplit=1),
    "auto_kp128_len_under": dict(chunk=32768, ilv=4096, ranges=0, presplit=1),
    # XCD ranges: kp 64 and a table within 128 MiB
    "auto_ranges_128mib_at": dict(ilv=1024, ranges=1),
    "auto_ranges_128mib_over": dict(ilv=1024, ranges=0),
    # pre-split at kp 64 without interleave: a table within 8 MB
    "auto_presplit_8mb_at": dict(ilv=0, presplit=1),
    "auto_presplit_8mb_over": dict(ilv=0, presplit=0),
    # 2^24 table rows (sentinel included) turn the pre-split gather off, whatever the knobs force
    "guard_rows_2p24_under": dict(ilv=64, presplit=1),
    "guard_rows_2p24_at": dict(ilv=0, ranges=0, presplit=0),
    # nnz_padded / 4096 rounded up to whole blocks, at most 32,768
    "layout_chunk_formula_mid": dict(chunk=3968),
    "layout_chunk_formula_top": dict(chunk=32768),
}


def test_layout_thresholds(plan_cases):
    for name, want in LAYOUTS.items():
        got = plan_cases[name]["layout"]
        assert {k: got[k] for k in want} == want, (name, got)


def _blocks(d):
    return (d + 31) // 32


def test_split_and_entry_space_counts(plan_cases):
    """Counts worked out here from the degrees: which rows split, how many slots, which rows go to entry space."""
    def expect(name, k, chunk, ilv, max_blocks):
        c = plan_cases[name]
        deg = c["deg"]
        split = [d for d in deg if d > (ilv or chunk)] if chunk else []
        assert c["n_reduce"] == len(split), name
        if not ilv:
            assert c["slots"] == sum(-(-d // chunk) for d in split), name
        dual = [sum(1 for d in deg if 0 < d <= min(k, chunk or d) and _blocks(d) == b + 1 <= max_blocks)
                for b in range(3)]
        assert c["n_dual"] == dual, (name, c["n_dual"], dual)
        assert c["n_full"] == len(deg) - len(split) - sum(dual), name

    expect("valu_kp16", 10, 64, 0, 0)
    expect("split_kp32", 32, 64, 0, 0)
    expect("split_kp64_k64", 64, 64, 0, 1)
    expect("split_kp64_k40", 40, 64, 0, 1)          # the 41-entry row is a 2-block row anyway; 33..40 never fit 1 block
    expect("split_kp128_k128", 128, 64, 0, 3)
    expect("split_kp128_k70", 70, 64, 0, 3)
    expect("split_kp128_k128_chunk128", 128, 128, 0, 3)
    expect("split_kp128_k70_chunk128", 70, 128, 0, 3)   # the 80-entry, 3-block row stays in the main launch
    expect("generic_k130", 130, 0, 0, 0)            # no split at any length
    expect("ilv_kp64_ranges", 64, 64, 64, 1)
    expect("ilv_kp128_ranges", 70, 128, 128, 3)
    assert plan_cases["split_kp64_dual_off"]["n_dual"] == [0, 0, 0]
    assert plan_cases["generic_k130"]["n_reduce"] == 0 and max(plan_cases["generic_k130"]["deg"]) == 100000
    # the rows the cases are about are there
    assert 41 in plan_cases["split_kp64_k40"]["deg"] and 80 in plan_cases["split_kp128_k70"]["deg"]


def test_generic_launch_plan(plan_cases):
    """generic_plan (the any-k path's launch geometry) for kp = 16, 32, ..., 1024 in both precisions: the invariants
    plan_check computes, the switch points from the LDS to the slab Gram with their part-full batches, the tightest
    launch, and the Python restatement (rowshapes.generic_plan, which the GPU tests use to say which variant a case
    runs) equal to the C++ on all 128 pairs."""
    c = plan_cases["generic_launch_plan"]
    assert len(c["invariants"]) == 7 and all(c["invariants"].values()), c["invariants"]
    rows = {(("f32", "f64")[r[0]], r[1]): rs.GenericPlan(bool(r[2]), r[3], r[4], r[5]) for r in c["rows"]}
    assert sorted(rows) == [(p, kp) for p in ("f32", "f64") for kp in range(16, 1025, 16)] and len(rows) == 128
    for (precision, kp), got in rows.items():
        assert rs.generic_plan(precision, kp) == got, (precision, kp, got)
    # last kp with the Gram in LDS, its batch, first slab kp
    for precision, last, batch in (("f32", 272, 10), ("f64", 176, 15)):
        assert [kp for (p, kp), g in rows.items() if p == precision and g.g_in_lds][-1] == last
        assert rows[precision, last].batch == batch and not rows[precision, last + 16].g_in_lds
    # the launch geometry test_gpu_anyk.py runs on
    want = {("f32", 144): (True, 64), ("f32", 272): (True, 10), ("f32", 288): (False, 56), ("f32", 512): (False, 32),
            ("f32", 1024): (False, 16), ("f64", 80): (True, 64), ("f64", 144): (True, 55), ("f64", 176): (True, 15),
            ("f64", 192): (False, 42), ("f64", 1024): (False, 8)}
    assert {key: (rows[key].g_in_lds, rows[key].batch) for key in want} == want
    # the tightest launch: fp64 kp = 144, 48 bytes under the 160 KiB of a compute unit
    total = {key: g.lds_bytes + rs.GENERIC_STATIC_LDS[key[0]] for key, g in rows.items()}
    assert max(total, key=total.get) == ("f64", 144) and total["f64", 144] == 163_840 - 48


def test_digests_match_golden(plan_cases):
    with open(os.path.join(GOLDEN, "plan_digests.json")) as f:
        golden = json.load(f)
    got = {name: c["digest"] for name, c in plan_cases.items()}
    assert got == golden
