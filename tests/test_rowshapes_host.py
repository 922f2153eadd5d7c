"""The power of the degree-ladder check (tests/rowshapes.py), measured with the oracle alone.

For every (k, lambda) that test_gpu_rowshapes.py solves on the GPU: the reference's own fp32 arithmetic passes the
per-row comparator, the fp64 solution of a block that differs by ONE entry in each row (first / last / middle entry
dropped, last rating off by 1) is rejected on every row of >= 2 entries, and every such row lies at least 5 bounds
away from its nearest mutant -- a condition on the inputs (signed unit-norm factors), not a measurement of a kernel.
The contrast case records why the inputs changed: on uniform [0, 1) factors the global envelope the older tests use
accepts a row that lost its last entry.

The same two facts for the any-k ladders of test_gpu_anyk.py (k = 65 .. 1024, and its grid-stride blocks): there the
reference's fp32 error on the one-rating row grows with k and passes 2e-5 at k = 1010 and 1024, so those two cases get
the bound the rule in rowshapes.py gives them (5 x the reference's worst row); the nearest mutant stays >= 9e-3 away.
"""
import numpy as np
import pytest

import rowshapes as rs

# (k, lambda) of test_gpu_rowshapes.py
CASES = [(k, 0.05) for k in (10, 20, 32, 40, 64, 70, 96, 128, 130)] + [(64, 1.0), (128, 1.0)]


@pytest.fixture(scope="module")
def ladder():
    return rs.ladder_block()


def test_ladder_block_is_what_it_says(ladder):
    blk, side, coo, degs = ladder.blk, ladder.side, ladder.coo, ladder.degs
    assert np.array_equal(np.diff(blk["row_ptr"]), degs) and blk["n_rows"] == len(degs) == 344
    assert set(range(1, 331)) | set(rs.LONG_DEGS) | {0} == set(degs.tolist()) and (degs == 0).sum() == 2
    assert 70_000 < blk["row_ptr"][-1] < 90_000          # the unforced chunk stays 1024 (als_plan.cpp chunk_entries)
    assert blk["ratings"].min() == 1 and blk["ratings"].max() == 5
    for sort_cols in (True, False):
        lad = rs.ladder_block(sort_cols=sort_cols)
        asc = []
        for i in range(len(degs)):
            c = lad.blk["col"][lad.blk["row_ptr"][i]:lad.blk["row_ptr"][i + 1]]
            assert len(np.unique(c)) == len(c) and (len(c) == 0 or (0 <= c.min() and c.max() < lad.n_opp))
            asc.append(bool(np.all(np.diff(c) > 0)))
        assert all(asc) if sort_cols else not all(asc[64:])
        # the COO arrays are the same rows in another arrival order: a stable sort by row gives the CSR back
        o = np.argsort(lad.coo["rows"], kind="stable")
        assert np.array_equal(lad.coo["cols"][o], lad.blk["col"])
        assert np.array_equal(lad.coo["ratings"][o], lad.blk["ratings"])
        assert np.array_equal(np.bincount(lad.coo["rows"], minlength=len(degs)), degs)
        assert not np.array_equal(lad.coo["rows"], np.sort(lad.coo["rows"]))
    assert np.array_equal(side.row_ptr, blk["row_ptr"]) and np.array_equal(side.col, blk["col"])
    assert coo["n_rows"] == blk["n_rows"]


def test_mutants_differ_by_one_entry_per_row(ladder):
    degs = ladder.degs
    m = rs.mutants(ladder.side)
    assert set(m) == {"drop_first", "drop_last", "drop_middle", "last_rating"}
    for name in ("drop_first", "drop_last", "drop_middle"):
        assert np.array_equal(np.diff(m[name].row_ptr), np.where(degs >= 2, degs - 1, degs)), name
    lr = m["last_rating"]
    diff = np.nonzero(lr.ratings != ladder.side.ratings)[0]
    assert np.array_equal(diff, ladder.side.row_ptr[1:][degs >= 2] - 1)
    assert np.all(np.abs(lr.ratings[diff].astype(int) - ladder.side.ratings[diff]) >= 1)
    assert lr.ratings.min() >= 1 and lr.ratings.max() <= 5


@pytest.mark.parametrize("k,lam", CASES)
def test_comparator_accepts_the_reference_and_rejects_every_mutant(ladder, k, lam):
    degs = ladder.degs
    F = rs.factors(ladder.n_opp, k)
    ref64, ref32 = rs.references(ladder.side, F, lam)
    # the reference's own fp32 arithmetic passes, and so does fp64 at the fp64 bar
    rel32 = rs.check_rows(ref32, ref64, ref32, degs, "f32")
    rs.check_rows(ref64, ref64, None, degs, "f64")
    print(f"k={k} lam={lam}: reference fp32 per-row max {rel32.max():.2e}", rs.bucket_max(rel32, degs))
    two = degs >= 2
    nearest = np.full(len(degs), np.inf)
    for name, mside in rs.mutants(ladder.side).items():
        mut = rs.oracle.update_side(mside, F, lam, "f64")
        for precision in ("f32", "f64"):
            bad = rs.rejected_rows(mut, ref64, degs, precision)
            assert bad[two].all(), (name, precision, np.nonzero(two & ~bad)[0][:8], degs[two & ~bad][:8])
            assert not bad[~two].any()                 # rows of 0 or 1 entries are the same rows
            with pytest.raises(AssertionError, match=f"{int(two.sum())} of {len(degs)} rows beyond"):
                rs.check_rows(mut, ref64, ref32, degs, precision)
        nearest = np.minimum(nearest, rs.row_errors(mut, ref64))
    worst = int(np.argmin(np.where(two, nearest, np.inf)))
    print(f"k={k} lam={lam}: nearest mutant {nearest[worst]:.2e} away (row of {degs[worst]} entries)")
    assert nearest[worst] >= rs.MARGIN * rs.BOUND["f32"], (k, lam, degs[worst], nearest[worst])


ANYK = [(k, 0) for k in sorted({c[1] for c in rs.ANYK_CASES})] + [(k, rows) for _, k, rows in rs.ANYK_STRIDE_CASES]


def test_anyk_ladders_are_what_they_say():
    small, wide, stride = rs.anyk_ladder(129), rs.anyk_ladder(1010), rs.anyk_ladder(273, 1100)
    assert sorted(small.degs.tolist()) == sorted((1, 2, 3, 9, 10, 11, 15, 16, 31, 32, 33, 55, 56, 64, 65, 97, 130, 257,
                                                  330, 0, 0)) and small.n_opp == 512
    assert wide.degs.tolist() == small.degs.tolist() + [1100] and wide.n_opp == 1280
    assert np.array_equal(rs.anyk_ladder(1024).blk["col"], wide.blk["col"])
    assert np.array_equal(rs.anyk_ladder(500).blk["col"], small.blk["col"])
    assert stride.degs.tolist() == [1 + i % 40 for i in range(1100)] and stride.n_opp == 512
    # every batch of the launch plans the cases run on has a row one short of it, at it and (<= 64) one over it or
    # a row that fills several: 8, 10, 15, 16, 55, 64 staged rows, and the 32-entry block
    for b in (10, 15, 16, 32, 55, 64):
        assert {b, b + 1} <= set(small.degs.tolist()) or {b - 1, b} <= set(small.degs.tolist()), b
    for precision, k, kp, in_lds, batch in rs.ANYK_CASES:
        assert kp == -(-k // 16) * 16 and k > (64 if precision == "f64" else 128)
        assert rs.generic_plan(precision, kp)[:2] == (in_lds, batch), (precision, k)
        assert rs.anyk_ladder(k).degs.max() > k or k < 1010


@pytest.mark.parametrize("k,rows", ANYK, ids=lambda v: str(v))
def test_anyk_reference_margin_and_mutant_margin(k, rows):
    """The yardstick of test_gpu_anyk.py, settled with the oracle alone: on the any-k ladders the reference's own fp32
    arithmetic stays at or below bound / MARGIN on every row, and every one-entry mutant is at least MARGIN x bound
    away -- at the bound rowshapes.anyk_bound gives that k (1e-4, or 5 x the reference's worst row where that is
    more: k = 1010 and 1024, whose recorded figures are re-measured here)."""
    lad, F, ref64, ref32 = rs.anyk_inputs(k, rows)
    degs = lad.degs
    bound = rs.anyk_bound("f32", k)
    rel32 = rs.row_errors(ref32, ref64)
    worst = float(rel32[degs > 0].max())
    print(f"k={k} rows={len(degs)}: reference fp32 per-row max {worst:.3e} (row of {degs[rel32.argmax()]} entries), "
          f"bound {bound:.3e}")
    if k in rs.ANYK_REF32_WORST:     # the recorded figure is this measurement, rounded up in its third digit
        assert rs.BOUND["f32"] / rs.MARGIN < worst <= rs.ANYK_REF32_WORST[k] <= 1.01 * worst
        assert bound == rs.MARGIN * rs.ANYK_REF32_WORST[k]
    else:
        assert bound == rs.BOUND["f32"]
    assert worst <= bound / rs.MARGIN
    rs.check_rows(ref32, ref64, ref32, degs, "f32", bound=bound)
    rs.check_rows(ref64, ref64, None, degs, "f64")
    two = degs >= 2
    nearest = np.full(len(degs), np.inf)
    for name, mside in rs.mutants(lad.side).items():
        mut = rs.oracle.update_side(mside, F, rs.ANYK_LAM, "f64")
        for precision in ("f32", "f64"):
            bad = rs.rejected_rows(mut, ref64, degs, precision, rs.anyk_bound(precision, k))
            assert bad[two].all() and not bad[~two].any(), (name, precision, degs[two & ~bad][:8])
        nearest = np.minimum(nearest, rs.row_errors(mut, ref64))
    i = int(np.argmin(np.where(two, nearest, np.inf)))
    print(f"k={k}: nearest mutant {nearest[i]:.2e} away (row of {degs[i]} entries)")
    assert nearest[i] >= rs.MARGIN * bound, (k, degs[i], nearest[i])


WIDTH_KS = sorted(set(rs.WIDTH_KS["f32"]) | set(rs.WIDTH_KS["f64"]) | set(rs.WIDTH_KS_F64_STRIDES))
REPEAT_KS = sorted(set(rs.REPEAT_KS["f32"]) | set(rs.REPEAT_KS["f64"]))


def test_width_and_repeat_ladders_are_what_they_say():
    lad, rep, ext = rs.width_ladder(), rs.repeat_ladder(), rs.repeat_ladder(True)
    degs = lad.degs
    assert degs.tolist() == list(rs.WIDTH_DEGS) and lad.n_opp == 512 and degs[-1] == 0 and (degs == 0).sum() == 1
    b = rs.FOLDIN_BATCH
    # the zero-filled tail of a 4-entry MFMA step, both sides of the first two batch boundaries, five batches
    assert {1, 2, 3, 4, 5, b - 1, b, b + 1, b + 2, 2 * b - 1, 2 * b, 2 * b + 1, 2 * b + 2} <= set(degs.tolist())
    assert -(-200 // b) == 4 and -(-257 // b) == 5
    assert set(rs.WIDTH_KS["f64"]) <= set(rs.WIDTH_KS["f32"]) and max(WIDTH_KS) <= 128
    for s in (16, 32, 64):                        # a width either side of every stride edge
        assert {s - 1, s + 1} <= set(WIDTH_KS)
    assert {1, 127} <= set(WIDTH_KS)
    # fp64 engines above 64 features: every stride between 64 and 128 filled, and entered by one feature
    assert {-(-k // 16) * 16 for k in rs.WIDTH_KS_F64_STRIDES + (65,)} == {80, 96, 112}
    assert {80, 96, 112, 81, 97} <= set(rs.WIDTH_KS_F64_STRIDES)
    rp = lad.blk["row_ptr"]
    for other in (rep, ext):
        assert np.array_equal(other.blk["row_ptr"], rp) and other.coo is None
        assert np.array_equal(other.side.col, other.blk["col"]) and np.array_equal(other.side.ratings, other.blk["ratings"])
        for i, d in enumerate(degs):
            c, c0 = other.blk["col"][rp[i]:rp[i + 1]], lad.blk["col"][rp[i]:rp[i + 1]]
            changed = np.nonzero(c != c0)[0].tolist()
            assert changed == ([] if d < 2 else [d - 1] if d < b + 2 else [b, d - 1]), (i, d)
            if d >= 2:
                assert c[-1] == c[0]
            if d >= b + 2:
                assert c[b] == c[b - 1]
            assert len(np.unique(c)) == d - len(changed)
    assert np.array_equal(rep.blk["ratings"], lad.blk["ratings"])
    # the extreme draw: every value of the int16 range's ends, 0 and a value beyond one byte; it holds a query whose
    # ratings are all 0 (its solution is exactly zero): the one-entry row
    r = ext.blk["ratings"]
    assert r.dtype == np.int16 and set(r.tolist()) == set(rs.EXTREME_RATINGS)
    all_zero = [int(d) for i, d in enumerate(degs) if d > 0 and not r[rp[i]:rp[i + 1]].any()]
    assert all_zero == [1], all_zero
    once = rs.counted_once(rep.side)
    assert np.array_equal(np.diff(once.row_ptr), np.where(degs >= b + 2, degs - 2, np.where(degs >= 2, degs - 1, degs)))
    same = rs.counted_once(lad.side)
    assert np.array_equal(same.col, lad.side.col) and np.array_equal(same.row_ptr, lad.side.row_ptr)


@pytest.mark.parametrize("k", WIDTH_KS)
def test_width_ladder_reference_margin_and_mutant_margin(k):
    """The yardstick of test_gpu_foldin_edges.py's width cases, settled with the oracle alone: on the width ladder, for
    every width next to a stride edge, the reference's own fp32 arithmetic stays at or below BOUND / MARGIN on every
    row and every one-entry mutant is at least MARGIN x BOUND away on every row of >= 2 entries. Measured: the
    reference's worst row 1.2e-5 (k = 17, the one-entry row; every other width <= 7.2e-6) against the 2e-5 allowed;
    the nearest mutant 9.6e-4 away (k = 1, the 128-entry row; every other width >= 4.2e-3) against the 5e-4 required."""
    lad, F, ref64, ref32 = rs.width_inputs(k)
    degs = lad.degs
    bound = rs.BOUND["f32"]
    rel32 = rs.row_errors(ref32, ref64)
    worst = float(rel32[degs > 0].max())
    print(f"k={k}: reference fp32 per-row max {worst:.3e} (row of {degs[rel32.argmax()]} entries)")
    assert worst <= bound / rs.MARGIN
    rs.check_rows(ref32, ref64, ref32, degs, "f32")
    rs.check_rows(ref64, ref64, None, degs, "f64")
    two = degs >= 2
    nearest = np.full(len(degs), np.inf)
    for name, mside in rs.mutants(lad.side).items():
        mut = rs.oracle.update_side(mside, F, rs.WIDTH_LAM, "f64")
        for precision in ("f32", "f64"):
            bad = rs.rejected_rows(mut, ref64, degs, precision)
            assert bad[two].all() and not bad[~two].any(), (name, precision, degs[two & ~bad][:8])
        nearest = np.minimum(nearest, rs.row_errors(mut, ref64))
    i = int(np.argmin(np.where(two, nearest, np.inf)))
    print(f"k={k}: nearest mutant {nearest[i]:.2e} away (row of {degs[i]} entries)")
    assert nearest[i] >= rs.MARGIN * bound, (k, degs[i], nearest[i])


@pytest.mark.parametrize("k", REPEAT_KS)
def test_repeated_index_counts_twice_and_counted_once_is_rejected(k):
    """include/als.h: an index a query lists twice counts twice. On the repeat ladder the reference's own fp32
    arithmetic stays at or below BOUND / MARGIN on every row, with ratings 1..5 (measured: <= 7.1e-6) and with the
    extreme int16 ratings (<= 6.3e-6), and the "counted once" mutant -- the CSR with the repeats removed -- is
    rejected on every row of >= 2 entries, MARGIN bounds away or more (measured: >= 3.0e-2)."""
    for entries in ("repeat", "extreme"):
        lad, F, ref64, ref32 = rs.width_inputs(k, entries)
        worst = float(rs.row_errors(ref32, ref64)[lad.degs > 0].max())
        print(f"k={k} {entries}: reference fp32 per-row max {worst:.3e}")
        assert worst <= rs.BOUND["f32"] / rs.MARGIN
        rs.check_rows(ref32, ref64, ref32, lad.degs, "f32")
        rs.check_rows(ref64, ref64, None, lad.degs, "f64")
    lad, F, ref64, ref32 = rs.width_inputs(k, "repeat")
    degs = lad.degs
    two = degs >= 2
    mut = rs.oracle.update_side(rs.counted_once(lad.side), F, rs.WIDTH_LAM, "f64")
    for precision in ("f32", "f64"):
        bad = rs.rejected_rows(mut, ref64, degs, precision)
        assert bad[two].all() and not bad[~two].any(), (precision, degs[two & ~bad][:8])
    away = rs.row_errors(mut, ref64)
    i = int(np.argmin(np.where(two, away, np.inf)))
    print(f"k={k}: counted-once mutant {away[i]:.2e} away at the nearest (row of {degs[i]} entries)")
    assert away[i] >= rs.MARGIN * rs.BOUND["f32"], (k, degs[i], away[i])
    # an all-zero query of the extreme draw has an exactly zero solution, which row_errors then demands of the kernel
    ext, _, ext64, _ = rs.width_inputs(k, "extreme")
    rp, r = ext.blk["row_ptr"], ext.blk["ratings"]
    zero_q = np.array([d > 0 and not r[rp[j]:rp[j + 1]].any() for j, d in enumerate(degs)])
    assert zero_q.sum() >= 1 and not ext64[zero_q].any() and ext64[(degs > 0) & ~zero_q].any(axis=1).all()


def test_comparator_rejects_other_damage(ladder):
    """Nonzero output on a row without a rating, a NaN, and a wrong shape are failures too; the report names the
    row, its degree and its task kind."""
    degs = ladder.degs
    F = rs.factors(ladder.n_opp, 64)
    ref64, ref32 = rs.references(ladder.side, F, 0.05)
    kinds = rs.task_kinds(degs, 64, 64)
    assert kinds[0] == kinds[31] == "entry-space" and kinds[32] == kinds[63] == "FULL"
    assert kinds[64] == "split into 2 slots" and kinds[128] == "split into 3 slots" and kinds[330] == "empty"
    assert kinds[list(degs).index(4000)] == "split into 63 slots"
    assert rs.task_kinds([96, 97, 70, 71], 70, 1024) == ["FULL", "FULL", "entry-space", "FULL"]       # n <= k only
    assert rs.task_kinds([96, 97], 128, 1024) == ["entry-space", "FULL"]
    assert rs.task_kinds([32, 4000], 130, 64, path="generic") == ["FULL", "FULL"]
    empty = int(np.nonzero(degs == 0)[0][0])
    got = ref32.copy()
    got[empty, 3] = 1e-30
    with pytest.raises(AssertionError, match=f"row {empty} deg 0 empty"):
        rs.check_rows(got, ref64, ref32, degs, "f32", kinds)
    got = ref32.copy()
    got[100, 0] = np.nan
    with pytest.raises(AssertionError, match="row 100 deg 101 split into 2 slots: err inf"):
        rs.check_rows(got, ref64, ref32, degs, "f32", kinds)
    got = ref32.astype(np.float64)
    got[40] = ref64[40] * (1 + 2e-4)
    with pytest.raises(AssertionError, match="1 of 344 rows beyond 0.0001 .f32.: row 40 deg 41 FULL: err 2.000e-04"):
        rs.check_rows(got, ref64, ref32, degs, "f32", kinds)
    with pytest.raises(AssertionError):
        rs.check_rows(ref32[:-1], ref64, ref32, degs, "f32", kinds)


def test_contrast_old_global_criterion_accepts_a_dropped_entry(ladder):
    """Uniform [0, 1) factors, k = 128, lambda = 0.05, as the older oracle comparisons draw them: the reference's fp32
    error on one-rating rows sets the global bound max(3 * rel_ref.max(), 1e-4), and under it the fp64 solution of a
    row of >= 129 entries that LOST ITS LAST ENTRY passes. The per-row comparator rejects the same row even on these
    inputs only while the row is short; the ladder's signed factors make every row sensitive."""
    degs = ladder.degs
    F = np.random.default_rng(128).random((ladder.n_opp, 128)).astype(np.float32).astype(np.float64)
    ref64, ref32 = rs.references(ladder.side, F, 0.05)
    mut = rs.oracle.update_side(rs.mutants(ladder.side)["drop_last"], F, 0.05, "f64")
    old_bound = max(3 * rs.row_errors(ref32, ref64)[degs > 0].max(), 1e-4)
    rel = rs.row_errors(mut, ref64)
    accepted = (degs >= 129) & (rel <= old_bound)
    print(f"old bound {old_bound:.2e}; dropped-last-entry mutant accepted on {int(accepted.sum())} rows of >= 129 "
          f"entries, e.g. degree {degs[accepted][:5]}, error {rel[accepted][:5]}")
    assert accepted.any(), (old_bound, rel[degs >= 129].min())
