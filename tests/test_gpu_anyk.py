"""The any-k kernels (csrc/als_generic.h) across their launch plan, every row against the fp64 oracle.

als_engine_create takes num_features up to 1024; beyond the wave-per-row kernels (fp32 k > 128, fp64 k > 64) one
workgroup solves one row, with the Gram's packed triangle in LDS or -- from the padded stride generic_plan
(als_plan.cpp) switches at -- in a per-workgroup global slab. The cases sit on that plan's edges: the first generic k of
each precision, the last stride with the Gram in LDS (fp32 272 with batches of 10 staged rows, fp64 176 with 15), the
first slab stride, fp64 kp = 144 (48 bytes under the 160 KiB of a compute unit), k with 12 and 14 padded features, and
k = 1024. rowshapes.generic_plan, held equal to the C++ by test_plan_host.py, says which variant and batch a case
runs; the any-k ladder (rowshapes.ANYK_DEGS) has a row either side of every batch and two empty rows, for k >= 1010
also a row of 1100 > k entries.

Each case asserts what test_gpu_rowshapes.py asserts of a path: the plan facts (generic, no REDUCE, one task per
row), rowshapes.check_rows on every row, als_sq_error against the oracle's, a clean integrity record, a bitwise repeat,
and exactly zero padded factor columns. The per-row bound is 1e-4 (fp32) / 1e-8 (fp64), except fp32 at k = 1010 and
1024, where the reference's own fp32 error on the one-rating row passes 2e-5 and the bound is 5 x that row's error
(rowshapes.anyk_bound; test_rowshapes_host.py proves both margins on the CPU).

Measured on an MI355X (lambda = 0.05): the largest per-row error next to the reference's own fp32 arithmetic on the
same rows, and the seconds of the case's first als_solve_half:

    precision  k     kp    Gram  batch   GPU worst row   reference fp32   bound      solve    whole case
    fp32       129   144   LDS   64      1.7e-06         7.1e-06          1e-4       <0.01 s  0.3 s
    fp32       257   272   LDS   10      1.6e-06         8.0e-06          1e-4       0.01 s   0.2 s
    fp32       273   288   slab  56      2.3e-06         1.0e-05          1e-4       0.01 s   0.2 s
    fp32       500   512   slab  32      2.5e-06         1.1e-05          1e-4       0.05 s   0.3 s
    fp32       1010  1024  slab  16      4.7e-06         2.2e-05          1.085e-4   0.50 s   3.2 s
    fp32       1024  1024  slab  16      4.5e-06         2.1e-05          1.03e-4    0.50 s   3.3 s
    fp64       65    80    LDS   64      1.0e-14         5.6e-06          1e-8       <0.01 s  0.1 s
    fp64       130   144   LDS   55      1.5e-14         6.1e-06          1e-8       <0.01 s  0.1 s
    fp64       161   176   LDS   15      1.2e-14         7.2e-06          1e-8       <0.01 s  0.1 s
    fp64       177   192   slab  42      1.2e-14         7.0e-06          1e-8       <0.01 s  0.1 s
    fp64       1024  1024  slab  8       3.2e-14         2.1e-05          1e-8       0.60 s   1.2 s
    fp32       273   288   slab  56      2.8e-06         1.1e-05          1e-4       0.03 s   1.2 s   (1100 rows)
    fp64       177   192   slab  42      1.6e-14         9.2e-06          1e-8       0.01 s   0.4 s   (1100 rows)
    fp32       129   144   LDS   64      3.3e-06         8.8e-06          1e-4       0.02 s   0.6 s   (4200 rows)

The worst row is the one-rating row in every case. A k = 1024 case spends most of its 3 s in the oracle's two k x k
inversions per row on the CPU (shared between the fp32 and the fp64 engine of one k); the module takes 11 s.
"""
import time

import numpy as np
import pytest
import torch

import rowshapes as rs

pytestmark = pytest.mark.gpu

LAM = rs.ANYK_LAM


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(cfk, precision, k, rows=0):
    """One half of the any-k ladder (rows > 0: of the grid-stride block) with every assertion of this module."""
    lad, F, ref64, ref32 = rs.anyk_inputs(k, rows)
    degs, n = lad.degs, lad.blk["n_rows"]
    kp = cfk.factor_stride(k, precision)
    plan = rs.generic_plan(precision, kp)
    bound = rs.anyk_bound(precision, k)
    with rs.knobs({}):
        eng = cfk.ALSEngine(k, precision)
    try:
        assert eng.kp == kp
        eng.alloc_factors(1, lad.n_opp)
        eng.alloc_factors(0, n)
        eng.set_block(0, lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"], 0, lad.n_opp)
        path, stats = eng.block_path(0), eng.block_stats(0)
        assert path["gram_path"] == "generic" and path["dual_rows"] == 0 and not path["presplit"], path
        # one FULL task per row at any length; a row without a rating has one too (it stores the zeros)
        assert stats["n_reduce"] == 0 and stats["n_tasks"] == n and int((degs > 0).sum()) in (n, n - 2), stats
        eng.write_factors(1, F)
        eng.factors[0].fill_(7.0)      # every row is stored by its task, the empty rows too (as zeros)
        eng.factors[0][n].zero_()      # ... but for the sentinel
        eng.synchronize()
        t0 = time.perf_counter()
        eng.solve_half(0, LAM)
        eng.synchronize()
        secs = time.perf_counter() - t0
        got = eng.read_factors(0, 0, n)
        kinds = rs.task_kinds(degs, k, 0, path="generic")
        rel = rs.check_rows(got, ref64, ref32, degs, precision, kinds, bound=bound)
        ref_rel = rs.row_errors(ref32, ref64)
        print(f"\n[anyk] {precision} k={k} kp={kp} {'LDS' if plan.g_in_lds else 'slab'} batch={plan.batch} rows={n}: "
              f"per-row max {rel.max():.2e} (row of {degs[rel.argmax()]}), reference fp32 {ref_rel.max():.2e} "
              f"(row of {degs[ref_rel.argmax()]}), bound {bound:.3e}, solve {secs:.2f} s")
        assert eng.integrity_status() == [0, 0, 0, 0]
        raw = eng.factors[0].cpu().numpy()
        assert raw.shape == (n + 1, kp)
        assert np.array_equal(raw[:n, :k], got)
        assert not raw[:n, k:].any(), np.nonzero(raw[:n, k:].any(axis=1))[0][:8]     # padded features: exactly zero
        assert not raw[n].any()                                                      # the sentinel row
        se, cnt = eng.sq_error(0)
        se_o, cnt_o = rs.oracle.sq_error(lad.side, got.astype(np.float64), F)
        assert cnt == cnt_o == int(degs.sum())
        assert se == pytest.approx(se_o, rel=1e-5 if precision == "f32" else 1e-12)
        eng.solve_half(0, LAM)
        again = eng.read_factors(0, 0, n)
        assert np.array_equal(again, got), np.nonzero(np.any(again != got, axis=1))[0][:8]
        assert eng.integrity_status() == [0, 0, 0, 0]
        return plan
    finally:
        eng.close()


@pytest.mark.parametrize("precision,k,kp,in_lds,batch", rs.ANYK_CASES,
                         ids=[f"{c[0]}-k{c[1]}" for c in rs.ANYK_CASES])
def test_generic_path_across_its_plan(cfk, precision, k, kp, in_lds, batch):
    """Every edge of generic_plan: the variant and batch the restated plan gives are the ones the case is here for."""
    assert cfk.factor_stride(k, precision) == kp
    assert rs.generic_plan(precision, kp)[:2] == (in_lds, batch)
    lad = rs.anyk_ladder(k)
    assert (lad.degs.max() > k or k == 500) and int((lad.degs == 0).sum()) == 2    # a row of d > k but at k = 500
    plan = _run(cfk, precision, k)
    assert (plan.g_in_lds, plan.batch) == (in_lds, batch)


@pytest.mark.parametrize("precision,k,rows", rs.ANYK_STRIDE_CASES,
                         ids=[f"{c[0]}-k{c[1]}-{c[2]}rows" for c in rs.ANYK_STRIDE_CASES])
def test_grid_stride_reuse(cfk, precision, k, rows):
    """More tasks than workgroups: 1100 rows over the 1024 slabs of the slab variant (a slab is zeroed and used again
    by the same workgroup), 4200 rows over the 4096 workgroups an LDS-variant launch is capped at."""
    plan = rs.generic_plan(precision, cfk.factor_stride(k, precision))
    assert plan.g_in_lds == (rows > 4096) and rows > (4096 if plan.g_in_lds else 1024)
    _run(cfk, precision, k, rows)


def test_create_time_limits(cfk):
    """num_features outside 1..1024 is refused when the engine is created: 0 as an invalid argument, 1025 as
    unsupported by this build; 1024 is accepted in both precisions (the cases above)."""
    for precision in ("f32", "f64"):
        with pytest.raises(cfk.ALSError) as e:
            cfk.ALSEngine(0, precision)
        assert e.value.status == 1 and "ALS_ERR_INVALID_ARGUMENT" in str(e.value)
        with pytest.raises(cfk.ALSError) as e:
            cfk.ALSEngine(1025, precision)
        assert e.value.status == 2 and "ALS_ERR_UNSUPPORTED" in str(e.value) and "1..1024" in str(e.value)
