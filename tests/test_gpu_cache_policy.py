"""The solve launches compute what the parent commit computed, bit for bit, on every path that touches a buffer with a
cache policy of its own (the streaming loads of the REDUCE launch's partial slots).

A cache policy changes no arithmetic and no order of operations, so the pin is equality, not a tolerance:
tests/golden/cache_policy_parent.npz holds the factor tables the parent commit's library left after one movie half and
one user half of every case (tools/record_cache_policy_golden.py; the user table as its sha256 and every 8th row). The
block is cache_policy_cases.py's degree ladder under ALS_CHUNK=64: 16 entry-space rows, 17 FULL rows and 46 rows of
2..9 PARTIAL slots with a REDUCE task at k = 64, 700 entry-space user rows (k = 128 under ALS_CHUNK=128, which leaves
it FULL rows: 39 entry-space rows of up to 96 entries, 5 FULL rows, 35 split rows).

    case              what it exercises
    k32               on-the-fly split, no pre-split
    k64, k128         pre-split path with FULL, PARTIAL / REDUCE and entry-space rows
    k64_on_the_fly    ALS_PRESPLIT=0: the on-the-fly path at the product width
    k64_range_guard   user rows with norms over 2^-24 .. 1: the pre-split launch stands down, the fallback launch solves
    k64_two_chunks    als_solve_half_chunk, two row ranges per half (bitwise the k64 entry)
    k64_refine        lambda = 0.005: FULL rows below the refinement gate, RowResidual runs

Each case asserts bitwise equality with the golden, the fp64-oracle envelope of the neighbouring tests (the parity bar
of test_gpu_integrity.py on both halves: p99 <= max(2 x the reference's fp32 p99, 2e-5), worst row <= max(3 x the
reference's worst, 1e-4); and rowshapes.check_rows, 1e-4 on every row, on the movie half wherever the reference's own
fp32 error stays within rowshapes' 2e-5 rule, i.e. everywhere but k64_range_guard and k64_refine), a clean integrity
record, and bitwise equality of a second run on a fresh engine.
"""
import functools
import os

import numpy as np
import pytest
import torch

import cache_policy_cases as cp
import conditioning as cd
import rowshapes as rs
from conftest import GOLDEN
from test_gpu_integrity import _check_vs_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(os.path.join(GOLDEN, "cache_policy_parent.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _movie_refs(table, k, lam):
    lad, _ = cp.blocks()
    return rs.references(lad.side, cp.user_table(table, k).astype(np.float64), lam)


@functools.lru_cache(maxsize=None)
def _user_refs(golden, lam):
    """The user half's references from the golden's movie table (which the case's own M equals bit for bit)."""
    _, (_, uside, _) = cp.blocks()
    return rs.references(uside, _golden()[f"{golden}.M"].astype(np.float64), lam)


def _full_rows_below_gate(case):
    """FULL rows whose smallest scaled pivot (fp64, conditioning.scaled_pivots) lies clear below the gate."""
    lad, _ = cp.blocks()
    F = cp.user_table(case.table, case.k).astype(np.float64)
    kinds = rs.task_kinds(lad.degs, case.k, 64)
    rows = []
    for i, kd in enumerate(kinds):
        if kd == "FULL":
            Y = F[lad.side.col[lad.side.row_ptr[i]:lad.side.row_ptr[i + 1]]]
            if cd.scaled_pivots(Y, case.lam, case.k)[0] < cd.GATE - cd.GATE_BAND:
                rows.append(i)
    return rows


@pytest.mark.parametrize("case", cp.CASES, ids=[c.name for c in cp.CASES])
def test_bitwise_the_parent(cfk, case):
    lad, (_, _, udegs) = cp.blocks()
    g = _golden()
    M, U, facts = cp.run_case(cfk, case)
    assert facts["integrity"] == [0, 0, 0, 0]
    # the intended paths ran
    presplit = case.k in (64, 128) and case.env.get("ALS_PRESPLIT") != "0"
    chunk = int(case.env["ALS_CHUNK"])
    kinds = rs.task_kinds(lad.degs, case.k, chunk)
    assert [p["presplit"] for p in facts["path"]] == [presplit, presplit], facts["path"]
    assert facts["path"][0]["gram_path"] == "mfma_split" and facts["path"][0]["chunk"] == chunk, facts["path"]
    assert facts["path"][0]["dual_rows"] == kinds.count("entry-space") and (case.k == 32 or "entry-space" in kinds)
    assert facts["path"][1]["dual_rows"] == rs.task_kinds(udegs, case.k, chunk).count("entry-space")
    assert "FULL" in kinds
    if not case.two_chunks:
        assert facts["stats"][0]["n_reduce"] == sum(kd.startswith("split") for kd in kinds) >= 34, facts["stats"]
    # 1. the parent's bits
    gM, gU_rows, gU_sha = g[f"{case.golden}.M"], g[f"{case.golden}.U_rows"], str(g[f"{case.golden}.U_sha256"])
    assert np.array_equal(M, gM), ("movie rows", np.nonzero(np.any(M != gM, axis=1))[0][:8])
    assert np.array_equal(U[::cp.U_SAMPLE], gU_rows), \
        ("user rows", cp.U_SAMPLE * np.nonzero(np.any(U[::cp.U_SAMPLE] != gU_rows, axis=1))[0][:8])
    assert cp.digest(U) == gU_sha
    # 2. the oracle envelope
    ref64, ref32 = _movie_refs(case.table, case.k, case.lam)
    uref64, uref32 = _user_refs(case.golden, case.lam)
    print(f"\n[{case.name}] movie per-row max {rs.row_errors(M, ref64)[lad.degs > 0].max():.2e} (reference fp32 "
          f"{rs.row_errors(ref32, ref64)[lad.degs > 0].max():.2e}); user {rs.row_errors(U, uref64).max():.2e} "
          f"({rs.row_errors(uref32, uref64).max():.2e})")
    _check_vs_oracle(M, ref64, ref32)
    _check_vs_oracle(U, uref64, uref32)
    if case.name not in ("k64_range_guard", "k64_refine"):
        assert rs.row_errors(ref32, ref64)[lad.degs > 0].max() <= rs.BOUND["f32"] / rs.MARGIN
        rs.check_rows(M, ref64, ref32, lad.degs, "f32", kinds)
    # 3. what the case is about
    if case.name == "k64_range_guard":   # the guard fired: bitwise the on-the-fly path's result
        M0, U0, _ = cp.run_case(cfk, case, env={**case.env, "ALS_PRESPLIT": "0"})
        assert np.array_equal(M, M0)
    if case.name == "k64_refine":
        # the step ran on the FULL rows below the gate: they are bitwise the rows of a run that refines every row
        # (a row the step skipped would differ, as the rows above the gate do); at lambda = 0.05 no FULL row is below it
        rows = _full_rows_below_gate(case)
        assert len(rows) >= 5, rows
        M0, _, _ = cp.run_case(cfk, case, env={**case.env, "ALS_REFINE_MIN_PIVOT": "2"})
        assert np.array_equal(M[rows], M0[rows]), rows
        full = [i for i, kd in enumerate(kinds) if kd == "FULL" and i not in rows]
        assert full and np.any(M[full] != M0[full])
        assert not _full_rows_below_gate(cp.CASES[1])
    # 4. a second run
    M2, U2, facts2 = cp.run_case(cfk, case)
    assert np.array_equal(M, M2) and np.array_equal(U, U2)
    assert facts2["integrity"] == [0, 0, 0, 0]
