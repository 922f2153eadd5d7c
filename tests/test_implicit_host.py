"""CPU side of implicit-feedback ALS (no kernel launch): the restatement against the dense formulation, the input
conditions of every GPU case of test_gpu_implicit.py re-measured with the restatement alone, the launch plans under the
sanitizers, and the bindings.

tests/plan/implicit_plan_check.cpp sweeps cfk::gram_table_plan and cfk::implicit_plan over every kp, both element sizes,
cu_count in {1, 8, 256} and 1 .. 10^7 rows / queries. It is compiled with als_plan.cpp by the host C++ compiler under
AddressSanitizer + UBSan and run as a program of its own, exactly as test_foldin_host.py runs foldin_plan_check: nothing
is preloaded and no Python runs in the sanitizer run.

Measured here (the figures implicit_ref.py records): on the five fp32 ladder cases the fp32 restatement's worst row is
4.9e-7 .. 1.15e-6 and every row's nearest mutant >= 7.6e-4; conditioning worst rows 1.15e-5 / 1.53e-5 / 2.13e-5 /
4.89e-5 with nearest mutants 6.3e-4 / 6.0e-3 / 8.7e-4 / 8.3e-4 (scaled condition numbers 2e2 .. 3.2e3); training: every
half lowers the loss by >= 3 % in both precisions, fp32 drifts 9.03e-5 from fp64 over four iterations.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import conditioning as cond
import implicit_ref as ir
import rowshapes as rs
from conftest import ROOT
from test_foldin_host import foldin_plan
from test_plan_host import CSRC, FLAGS, _compilers

LDS_LIMIT = 160 * 1024
MAX_SLABS, MIN_SLAB_ROWS, BATCH = 1024, 256, 64


def gram_table_plan(kp: int, elem_bytes: int, n_rows: int) -> dict:
    """gram_table_plan of als_plan.cpp restated: slabs of 256 rows until that would take more than 1024 of them, then
    the smallest multiple of the 64-row batch that keeps the count within 1024; the LDS is one staged batch at
    fold-in's pitch plus fold_store's rating slots. Nothing depends on the device."""
    per = -(-n_rows // MAX_SLABS)
    rows_per_slab = max(MIN_SLAB_ROWS, -(-per // BATCH) * BATCH)
    pitch = kp if kp % 32 == 16 else kp + 16
    return {"threads": 256, "slabs": max(1, -(-n_rows // rows_per_slab)), "rows_per_slab": rows_per_slab,
            "lds_bytes": elem_bytes * (BATCH * pitch + BATCH)}


def solve_implicit_plan(kp: int, elem_bytes: int, n_queries: int, cu_count: int) -> dict:
    """The implicit solve has fold-in's launch contract and LDS layout: its plan is foldin_plan's."""
    return foldin_plan(kp, elem_bytes, n_queries, cu_count)


# ---------------------------------------------------------------------------------------------------------------------
# 1: the G trick
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items,k,alpha,lam", [(7, 3, 40.0, 0.05), (12, 5, 1.0, 0.1), (40, 10, 10.0, 0.01)])
def test_restatement_equals_the_dense_formulation(n_items, k, alpha, lam):
    rng = np.random.default_rng([n_items, k])
    Y = rng.standard_normal((n_items, k))
    # rows: plain, with a zero rating, with a repeated index (different ratings), empty, every item, one entry
    rows = [([0, 2, 5], [3, 1, 5]), ([1, 3, 4], [2, 0, 4]), ([2, 6, 2], [1, 4, 3]), ([], []),
            (list(range(n_items)), list(rng.integers(0, 6, n_items))), ([n_items - 1], [5])]
    row_ptr = np.cumsum([0] + [len(c) for c, _ in rows]).astype(np.int64)
    col = np.concatenate([np.asarray(c, np.int32) for c, _ in rows])
    rat = np.concatenate([np.asarray(r, np.int16) for _, r in rows])
    got = ir.solve_rows((row_ptr, col, rat), Y, lam, alpha)
    want = ir.solve_rows_dense((row_ptr, col, rat), Y, lam, alpha)
    assert not got[3].any() and not want[3].any()
    rel = rs.row_errors(got, want)
    assert (rel <= 1e-10).all(), rel
    # the zero rating contributes nothing; the repeated index counts twice, which is not once
    without = ir.solve_rows((np.array([0, 2], np.int64), np.array([1, 4], np.int32), np.array([2, 4], np.int16)), Y, lam, alpha)
    assert rs.row_errors(got[1:2], without)[0] <= 1e-12
    once = ir.solve_rows((np.array([0, 2], np.int64), np.array([2, 6], np.int32), np.array([1, 4], np.int16)), Y, lam, alpha)
    assert rs.row_errors(got[2:3], once)[0] > 1e-3


def test_loss_is_the_dense_sum():
    rng = np.random.default_rng(3)
    U, M = rng.standard_normal((5, 3)), rng.standard_normal((4, 3))
    R = rng.integers(0, 4, (5, 4))
    want = sum((1 + 2.0 * R[u, i]) * ((R[u, i] > 0) - U[u] @ M[i]) ** 2 for u in range(5) for i in range(4))
    want += 0.25 * ((U ** 2).sum() + (M ** 2).sum())
    assert abs(ir.loss(U, M, R, 0.25, 2.0) - want) <= 1e-12 * want


# ---------------------------------------------------------------------------------------------------------------------
# 2: the input conditions of the GPU cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ir.LADDER_F32, ids=lambda c: "k%d-a%g-l%g" % c)
def test_ladder_conditions_fp32(case):
    """The fp32 restatement stays LADDER_MARGIN x inside rowshapes.BOUND on every row and every row's nearest mutant
    (an entry dropped, a rating + 1, lambda n, b without the 1 +, G left out) LADDER_MARGIN x outside it."""
    k, alpha, lam = case
    lad, F, ref64 = ir.ladder_case(*case)
    worst = rs.row_errors(ir.solve_rows(lad.side, F, lam, alpha, np.float32), ref64).max()
    near = ir.nearest_mutant(lad.side, F, lam, alpha, ref64)
    i = int(near.argmin())
    print(f"\n[implicit] ladder {case}: fp32 restatement worst row {worst:.3e}, nearest mutant {near.min():.3e} "
          f"(row of {lad.degs[i]})")
    assert worst * ir.LADDER_MARGIN <= rs.BOUND["f32"]
    assert near.min() >= ir.LADDER_MARGIN * rs.BOUND["f32"]
    assert np.isinf(near[lad.degs == 0]).all() and np.isfinite(near[lad.degs > 0]).all()


@pytest.mark.parametrize("case", ir.LADDER_F64, ids=lambda c: "k%d-a%g-l%g" % c)
def test_ladder_conditions_fp64(case):
    k, alpha, lam = case
    lad, F, ref64 = ir.ladder_case(*case)
    near = ir.nearest_mutant(lad.side, F, lam, alpha, ref64)
    print(f"\n[implicit] ladder fp64 {case}: nearest mutant {near.min():.3e}")
    assert near.min() >= ir.LADDER_MARGIN * rs.BOUND["f64"]


@pytest.mark.parametrize("case", ir.COND_CASES, ids=lambda c: "k%d-a%g-l%g" % c)
def test_conditioning_conditions(case):
    """The recorded worst fp32 row of each conditioning case is what the restatement gives; a case is in COND_F32
    exactly when every row's nearest mutant is MUTANT_MARGIN bars away; fp64 keeps that margin from 1e-8 everywhere."""
    k, alpha, lam = case
    lad, F, ref64 = ir.cond_case(*case)
    worst = rs.row_errors(ir.solve_rows(lad.side, F, lam, alpha, np.float32), ref64).max()
    near = ir.nearest_mutant(lad.side, F, lam, alpha, ref64).min()
    G = ir.gram(F)
    conds = [np.linalg.cond(_scaled(G + alpha * _wgram(lad, F, i) + lam * np.eye(k)))
             for i in range(len(lad.degs)) if lad.degs[i]]
    print(f"\n[implicit] conditioning {case}: fp32 restatement worst row {worst:.3e}, nearest mutant {near:.3e}, bar "
          f"{ir.cond_bar(case):.3e}, scaled condition {min(conds):.0f} .. {max(conds):.0f}")
    assert cond.round_up(worst) == ir.COND_REF32_WORST[case]
    assert (case in ir.COND_F32) == (near >= cond.MUTANT_MARGIN * ir.cond_bar(case))
    assert near >= cond.MUTANT_MARGIN * rs.BOUND["f64"]


def _wgram(lad, F, i):
    sl = slice(lad.side.row_ptr[i], lad.side.row_ptr[i + 1])
    Ys = F[lad.side.col[sl]]
    return (Ys * lad.side.ratings[sl].astype(np.float64)[:, None]).T @ Ys


def _scaled(A):
    d = 1.0 / np.sqrt(np.diag(A))
    return A * d[:, None] * d[None, :]


def test_training_conditions(cfk):
    """Every half of the restatement lowers the loss by >= 3 % in both precisions, the fp32 restatement stays within
    BOUND of the fp64 one after the first half, and its drift after the fourth iteration is the recorded figure."""
    t = ir.TRAIN
    R, (m, u, r) = ir.train_inputs()
    ds = cfk.Dataset.from_ratings(m, u, r)
    assert ds.counts()[:2] == (t["n_movies"], t["n_users"])
    U0 = ds.init_user_factors(t["k"], t["seed"])
    h64 = ir.train(R, U0, t["lam"], t["alpha"], t["halves"])
    h32 = ir.train(R, U0, t["lam"], t["alpha"], t["halves"], np.float32)
    for hist in (h64, h32):
        prev = ir.loss(U0, np.zeros((t["n_movies"], t["k"])), R, t["lam"], t["alpha"])
        for U, M in hist:
            cur = ir.loss(U, M, R, t["lam"], t["alpha"])
            assert cur <= 0.97 * prev
            prev = cur
    assert rs.row_errors(h32[0][1], h64[0][1]).max() <= rs.BOUND["f32"]
    drift = max(rs.row_errors(h32[-1][0], h64[-1][0]).max(), rs.row_errors(h32[-1][1], h64[-1][1]).max())
    print(f"\n[implicit] training: fp32 restatement drift after {t['halves']} halves {drift:.3e}")
    assert cond.round_up(drift) == ir.TRAIN_REF32_DRIFT


# ---------------------------------------------------------------------------------------------------------------------
# 3: the plans
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("implicitplan") / "implicit_plan_check")
    srcs = [os.path.join(ROOT, "tests", "plan", "implicit_plan_check.cpp"), os.path.join(CSRC, "als_plan.cpp")]
    errors = []
    for cxx in _compilers():
        p = subprocess.run(cxx + FLAGS + ["-I", CSRC] + srcs + ["-o", exe], capture_output=True, text=True)
        if p.returncode == 0:
            break
        errors.append(" ".join(cxx) + ":\n" + p.stderr[-2000:])
    else:
        pytest.fail("no host compiler built implicit_plan_check with the sanitizers:\n" + "\n".join(errors))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    return json.loads(run.stdout)


N_COUNTS = 70 + 6 * 3 + 17


def test_plan_sweep_holds_every_invariant(plan_sweep):
    """The slabs tile the rows exactly once, slab count and length do not depend on cu_count (nor, the length, on kp),
    LDS <= 163,840 B and what the kernels lay out, the pitch and alignment rules: every kp, both element sizes, 1 .. 10^7."""
    assert plan_sweep["cases"] == (4 * 2 + 3) * 3 * N_COUNTS
    assert plan_sweep["failed"] == {}
    assert len(plan_sweep["gram"]) == (4 * 2 + 3) * N_COUNTS and len(plan_sweep["solve"]) == plan_sweep["cases"]
    assert "128/8/10000000" in plan_sweep["gram"]


def test_python_restatements_equal_the_plans(plan_sweep):
    seen = set()
    for key, (threads, slabs, rows_per_slab, lds) in plan_sweep["gram"].items():
        kp, elem, n = (int(x) for x in key.split("/"))
        assert gram_table_plan(kp, elem, n) == {"threads": threads, "slabs": slabs, "rows_per_slab": rows_per_slab,
                                                "lds_bytes": lds}, key
        seen.add((kp, elem))
    assert seen == {(kp, elem) for kp in (16, 32, 64, 128) for elem in (4, 8)} | {(kp, 8) for kp in (80, 96, 112)}
    for key, (threads, grid, batch, lds) in plan_sweep["solve"].items():
        kp, elem, nq, cu = (int(x) for x in key.split("/"))
        assert solve_implicit_plan(kp, elem, nq, cu) == {"threads": threads, "workgroups": grid, "batch": batch,
                                                         "lds_bytes": lds}, key
    # the shapes DESIGN.md section 3.10 quotes
    assert gram_table_plan(64, 4, 17770) == {"threads": 256, "slabs": 70, "rows_per_slab": 256, "lds_bytes": 20736}
    assert gram_table_plan(128, 4, 480189) == {"threads": 256, "slabs": 938, "rows_per_slab": 512, "lds_bytes": 37120}
    assert gram_table_plan(128, 8, 10 ** 7) == {"threads": 256, "slabs": 1022, "rows_per_slab": 9792, "lds_bytes": 74240}


# ---------------------------------------------------------------------------------------------------------------------
# 4: the ABI and the bindings
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_headers_declare_and_python_binds_the_calls(cfk):
    from cfk_amd import _lib
    als_h = open(os.path.join(ROOT, "include", "als.h")).read()
    flat = re.sub(r"\s+", " ", als_h)
    for proto in ("int als_gram_table(als_engine* e, int side, void* host_out, int64_t out_ld);",
                  "int als_gram_table_plan(const als_engine* e, int64_t n_rows, int64_t info[4]);",
                  "int als_solve_implicit(als_engine* e, int side, int64_t n_queries, const int64_t* q_ptr, "
                  "const int32_t* q_idx, const int16_t* q_ratings, float lambda, float alpha, const int64_t* dst_rows, "
                  "void* host_out, int64_t out_ld);",
                  "int als_solve_implicit_plan(const als_engine* e, int64_t n_queries, int64_t info[4]);"):
        assert proto in flat, proto
    assert "#define ALS_ABI_VERSION 3" in als_h                        # purely additive
    sigs = {name: args for name, _, args in _lib.SIGNATURES}
    assert [len(sigs[n]) for n in ("als_gram_table", "als_gram_table_plan", "als_solve_implicit",
                                   "als_solve_implicit_plan")] == [4, 3, 11, 3]
    L = _lib.lib()
    for name in ("als_gram_table", "als_gram_table_plan", "als_solve_implicit", "als_solve_implicit_plan"):
        assert getattr(L, name).argtypes == sigs[name], name
    # als_solve_implicit is als_fold_in with alpha after lambda
    assert sigs["als_solve_implicit"][:7] == sigs["als_fold_in"][:7] and sigs["als_solve_implicit"][8:] == sigs["als_fold_in"][7:]
    assert sigs["als_solve_implicit"][7] is sigs["als_fold_in"][6]
    assert L.als_abi_version() == 3
    for name in ("gram_table", "gram_table_plan", "solve_implicit", "solve_implicit_plan"):
        assert callable(getattr(cfk.ALSEngine, name)), name
    for name in ("implicit_half", "implicit_iteration", "implicit_loss", "fold_in_implicit", "recommend_for"):
        assert callable(getattr(cfk.ALSApp, name)), name
    import inspect
    assert inspect.signature(cfk.ALSApp.recommend_for).parameters["implicit_alpha"].default is None
