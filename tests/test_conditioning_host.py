"""The conditions on the inputs of test_gpu_conditioning.py (tests/conditioning.py), proved with the oracle alone.

For every (k, family, lambda) the GPU module solves: the block is what it says; rows sit on both sides of the
refinement gate of the tile solve and close to it, FULL, split and entry-space rows go below a pivot of 0.3, every
populated pivot bucket holds at least 3 rows and few rows lie within 0.01 of the gate (the band the gate test exempts);
the reference's own fp32 arithmetic passes conditioning.check_case and stays within the recorded table the bounds are
made of; the fp64 oracle is within a fifth of the fp64 bar of an extended-precision solution; and the fp64 solution of
a block that differs by ONE entry in each row is rejected on every row of >= 2 entries, with every such row's nearest
mutant at least 3 of its bounds away. These are facts about the inputs, not measurements of a kernel.
"""
import numpy as np
import pytest

import conditioning as cd
import rowshapes as rs

GATED = [(k, fam) for k in cd.MFMA_KS for fam in cd.FAMILIES]
CASES = cd.all_cases()


def _ids(v):
    return str(v)


def test_block_and_tables_are_what_they_say():
    lad = cd.block()
    degs = lad.degs
    assert np.array_equal(np.diff(lad.blk["row_ptr"]), degs) and lad.blk["n_rows"] == len(degs) == 79
    want = set(range(1, 131, 3)) | {2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 200, 257, 330, 0}
    want |= {5, 6, 8, 9, 12}                      # the further short rows (with more of 1, 2, 3, 4)
    assert set(degs.tolist()) == want and (degs == 0).sum() == 1 and (degs == 1).sum() == 5
    assert lad.n_opp == cd.N_OPP == 1024 and lad.blk["col"].max() < 1024
    # under the forced 64-entry chunk: entry-space, FULL and split rows at k = 64, no FULL row left at k = 128
    kinds = cd.kinds_of(64)
    assert kinds[list(degs).index(32)] == "entry-space" and kinds[list(degs).index(33)] == "FULL"
    assert kinds[list(degs).index(64)] == "FULL" and kinds[list(degs).index(65)] == "split into 2 slots"
    assert kinds[list(degs).index(330)] == "split into 6 slots" and kinds[-1] == "empty"
    assert "FULL" not in cd.kinds_of(128) and "FULL" in cd.kinds_of(128, dual=False)
    assert "entry-space" not in cd.kinds_of(32) and "entry-space" in cd.kinds_of(40)
    for k in (10, 64):
        S, Off = cd.table("signed", k), cd.table("offset", k)
        assert np.array_equal(S, rs.factors(1024, k))
        for F in (S, Off):
            assert np.array_equal(F, F.astype(np.float32).astype(np.float64)) and not F.flags.writeable
        # the shared direction: the mean row of `offset` is 0.9 / sqrt(k) in every feature, that of `signed` ~0
        assert abs(Off.mean() * np.sqrt(k) - 0.9) < 0.02 and abs(S.mean() * np.sqrt(k)) < 0.02
    assert set(cd.LAMBDAS_OF) == {(k, f) for k in cd.MFMA_KS + (10, 20, 130) for f in cd.FAMILIES}
    assert cd.LAMBDAS_OF[(64, "signed")] == cd.LAMBDAS == (0.05, 0.01, 0.005, 0.002)
    assert all(len(cd.lambdas(k, f)) == 4 and list(cd.lambdas(k, f)) == sorted(cd.lambdas(k, f), reverse=True)
               for k, f in GATED)
    assert set(cd.REF32_WORST) == set(CASES)


def test_scaled_pivots_known_systems():
    """One rating: the scaled k x k system is I + (1 - eps) v v^T-like with a single small pivot lam / (lam + max
    y_f^2-ish); checked against a direct elimination in the kernel's order, and the dual pivot of a single entry is 1.
    Orthonormal rows: every pivot is 1."""
    rng = np.random.default_rng(0)
    for k in (32, 40, 64, 128, 10, 130):
        Y = rng.standard_normal((7, k)) / np.sqrt(k)
        kp = cd.padded_k(k)
        A = np.eye(kp)
        A[:k, :k] = Y.T @ Y + float(np.float32(0.01)) * 7 * np.eye(k)
        if kp in (32, 64, 128):
            C = kp // 16
            order = [C * i + b for b in range(C) for i in range(16)]      # position 16 b + i holds feature C i + b
            A = A[np.ix_(order, order)]
        d = 1 / np.sqrt(np.diag(A))
        S = A * d[:, None] * d[None, :]
        piv = []
        for p in range(kp):                                               # plain Gaussian elimination, no pivoting
            piv.append(S[p, p])
            S[p + 1:, p + 1:] -= np.outer(S[p + 1:, p], S[p, p + 1:]) / S[p, p]
        got, cond = cd.scaled_pivots(Y, 0.01, k)
        assert got == pytest.approx(min(piv), rel=1e-10) and 0 < got <= 1 and cond >= 1
    assert cd.scaled_pivots(Y[:1], 0.01, 130, dual=True)[0] == pytest.approx(1.0)
    Q = np.linalg.qr(rng.standard_normal((64, 64)))[0]
    assert cd.scaled_pivots(Q, 0.05, 64)[0] == pytest.approx(1.0) == cd.scaled_pivots(Q[:20], 0.05, 64, True)[0]
    # the dual system is eliminated in the physical entry order: 33 entries pad to 64 positions
    Y = rng.standard_normal((33, 64)) / 8
    B = Y @ Y.T + float(np.float32(0.01)) * 33 * np.eye(33)
    pos = [rs.BLOCK_ENTRIES * (e // 32) + (e % 32 % 4) * 8 + e % 32 // 4 for e in range(33)]
    o = np.argsort(pos)
    d = 1 / np.sqrt(np.diag(B))
    L = np.linalg.cholesky((B * d[:, None] * d[None, :])[np.ix_(o, o)])
    assert cd.scaled_pivots(Y, 0.01, 64, True)[0] == pytest.approx((np.diag(L) ** 2).min(), rel=1e-10)
    assert list(cd.bucket_of([1.0, 0.45, 0.449, 0.3, 0.1, 0.03, 0.01, 0.0099])) == [0, 0, 1, 1, 2, 3, 4, -1]


@pytest.mark.parametrize("k,family", GATED, ids=_ids)
def test_gate_population(k, family):
    """Rows on both sides of the gate and next to it, on the pivot the gate sees (the dual one for entry-space rows),
    under the default plan and with the entry-space solve off."""
    degs = cd.block().degs
    n = len(degs)
    for dual in (True, False):
        kinds = cd.kinds_of(k, dual=dual)
        above = below = 0
        for lam in cd.lambdas(k, family):
            c = cd.case(k, family, lam)
            gp = cd.gate_pivots(c, kinds)
            above += int(((gp >= 0.45) & (gp < 0.50)).sum())
            below += int(((gp >= 0.40) & (gp < 0.45)).sum())
            band = int(((gp >= cd.GATE - cd.GATE_BAND) & (gp <= cd.GATE + cd.GATE_BAND)).sum())
            print(f"k={k} {family} lam={lam} dual={dual}: {int((gp >= 0.46).sum())} rows above the band, "
                  f"{int((gp < 0.44).sum())} below, {band} in it; smallest pivot {np.nanmin(gp):.3f}, "
                  f"largest condition number {np.nanmax(c.cond):.0f}")
            assert band <= 0.10 * n, (lam, dual, band)
            # every bucket that holds a row holds at least 3, and no row lies below the last bucket
            cnt = np.bincount(c.bucket[degs > 0], minlength=len(cd.BUCKET_NAMES))
            assert (c.bucket[degs > 0] >= 0).all() and all(x == 0 or x >= 3 for x in cnt), (lam, cnt)
        if k in (32, 64, 128):
            assert above >= 3 and below >= 3, (dual, above, below)


@pytest.mark.parametrize("k", cd.MFMA_KS)
def test_every_task_kind_goes_below_0_3(k):
    """One (family, lambda) of each k puts rows of every task kind its plans have -- FULL, split (REDUCE) and
    entry-space under the default knobs, FULL and split with the entry-space solve off -- below a pivot of 0.3."""
    def low_kinds(c, kinds):
        gp = cd.gate_pivots(c, kinds)
        return {kd.split(" ")[0] for kd, p in zip(kinds, gp) if p < 0.3}
    hits = []
    for family in cd.FAMILIES:
        for lam in cd.lambdas(k, family):
            c = cd.case(k, family, lam)
            ok = all({kd.split(" ")[0] for kd in kinds} - {"empty"} <= low_kinds(c, kinds)
                     for kinds in (cd.kinds_of(k), cd.kinds_of(k, dual=False)))
            if ok:
                hits.append((family, lam))
    print(f"k={k}: every task kind below 0.3 at {hits}")
    assert hits and all(f == "offset" for f, _ in hits)      # on `signed`, split rows (n > k) stay well conditioned


@pytest.mark.parametrize("k", (10, 20, 130))
def test_ungated_cases_are_populated(k):
    degs = cd.block().degs
    for family in cd.FAMILIES:
        assert len(cd.ungated_lambdas(k, family)) == 2
        for lam in cd.ungated_lambdas(k, family):
            c = cd.case(k, family, lam)
            cnt = np.bincount(c.bucket[degs > 0], minlength=len(cd.BUCKET_NAMES))
            assert (c.bucket[degs > 0] >= 0).all() and all(x == 0 or x >= 3 for x in cnt), (family, lam, cnt)
    for prec, kk in cd.UNGATED:
        assert (kk, "signed") in cd.LAMBDAS_OF


def _exact_solution(side, F, lam):
    """(Y^T Y + lambda n I)^{-1} Y^T r per row to ~extended precision: fp64 solves refined twice against residuals
    formed in long double from the rows themselves (test_gpu_parity._exact_solution)."""
    ld = np.longdouble
    lam = ld(np.float64(np.float32(lam)))
    k = F.shape[1]
    out = np.zeros((len(side.row_ptr) - 1, k), np.float64)
    for i in range(len(side.row_ptr) - 1):
        lo, hi = side.row_ptr[i], side.row_ptr[i + 1]
        if hi == lo:
            continue
        Y = F[side.col[lo:hi]].astype(np.float64)
        r = side.ratings[lo:hi].astype(np.float64)
        A = Y.T @ Y + float(lam) * (hi - lo) * np.eye(k)
        YL, rL = Y.astype(ld), r.astype(ld)
        bL = YL.T @ rL
        x = np.linalg.solve(A, Y.T @ r).astype(ld)
        for _ in range(2):
            res = bL - YL.T @ (YL @ x) - lam * ld(hi - lo) * x
            x = x + np.linalg.solve(A, res.astype(np.float64)).astype(ld)
        out[i] = x.astype(np.float64)
    return out


@pytest.mark.parametrize("k,family,lam", CASES, ids=_ids)
def test_reference_and_mutants(k, family, lam):
    lad = cd.block()
    degs = lad.degs
    c = cd.case(k, family, lam)
    rated = degs > 0
    # the reference's fp32 arithmetic passes, within the recorded table (the figures are this measurement, rounded
    # up in the third digit); fp64 passes at the fp64 bar
    rel32 = cd.check_case(c.ref32, c, "f32")
    cd.check_case(c.ref64, c, "f64")
    worst = cd.bucket_worst(rel32, c.bucket)
    print(f"k={k} {family} lam={lam}: reference fp32 worst per bucket {['%.2e' % w for w in worst]}, median "
          f"{np.median(rel32[rated]):.2e}; condition number up to {np.nanmax(c.cond):.0f}")
    for w, rec in zip(worst, cd.REF32_WORST[(k, family, lam)]):
        assert w <= rec <= 1.01 * w + 1e-300, (w, rec)
    assert np.array_equal(cd.bounds(c, "f64"), np.full(len(degs), rs.BOUND["f64"]))
    assert (cd.bounds(c, "f32") >= rs.BOUND["f32"]).all()
    # the oracle against an extended-precision solution: the fp64 bar is about the kernel, not the oracle's LU
    exact = _exact_solution(lad.side, c.F, lam)
    err = rs.row_errors(c.ref64, exact)
    assert err.max() <= rs.BOUND["f64"] / 5, (int(err.argmax()), err.max())
    # one-entry mutants
    two = degs >= 2
    nearest = np.full(len(degs), np.inf)
    for name, mside in rs.mutants(lad.side).items():
        mut = rs.oracle.update_side(mside, c.F, lam, "f64")
        for precision in ("f32", "f64"):
            bad = cd.rejected_rows(mut, c, precision)
            assert bad[two].all(), (name, precision, degs[two & ~bad][:8])
            assert not bad[~two].any()
            with pytest.raises(AssertionError, match=f"{int(two.sum())} of {len(degs)} rows beyond"):
                cd.check_case(mut, c, precision)
        nearest = np.minimum(nearest, rs.row_errors(mut, c.ref64))
    margin = np.where(two, nearest / cd.bounds(c, "f32"), np.inf)
    i = int(margin.argmin())
    print(f"k={k} {family} lam={lam}: nearest mutant {margin[i]:.1f} bounds away (row of {degs[i]} entries, bucket "
          f"{cd.BUCKET_NAMES[c.bucket[i]]}, error {nearest[i]:.2e})")
    assert margin[i] >= cd.MUTANT_MARGIN, (degs[i], nearest[i], cd.bounds(c, "f32")[i])


def test_check_case_reports_and_rejects_other_damage():
    c = cd.case(64, "offset", 0.005)
    degs = cd.block().degs
    kinds = cd.kinds_of(64)
    empty = int(np.nonzero(degs == 0)[0][0])
    got = c.ref32.copy()
    got[empty, 3] = 1e-30
    with pytest.raises(AssertionError, match=f"row {empty} deg 0 empty bucket empty"):
        cd.check_case(got, c, "f32", kinds)
    i = list(degs).index(130)
    got = c.ref32.astype(np.float64)
    got[i] = c.ref64[i] * (1 + 1.5 * cd.bounds(c, "f32")[i])
    with pytest.raises(AssertionError, match=rf"1 of 79 rows beyond their bound .k=64 offset lam=0.005 f32.: row {i} "
                                             rf"deg 130 split into 3 slots bucket \[0\.\d+, 0\.\d+\) pivot 0\.\d+: "):
        cd.check_case(got, c, "f32", kinds)
    got = c.ref32.copy()
    got[5, 0] = np.nan
    with pytest.raises(AssertionError, match="err inf"):
        cd.check_case(got, c, "f32", kinds)
    # a solve that is uniformly 2.5 x worse than the reference's median fails the median check though no row is out
    rel32 = rs.row_errors(c.ref32, c.ref64)
    med = np.median(rel32[degs > 0])
    assert 2 * med > 2e-5
    got = c.ref64 * (1 + 2.5 * med)
    assert not cd.rejected_rows(got, c, "f32").any()
    with pytest.raises(AssertionError, match="median"):
        cd.check_case(got, c, "f32", kinds)
    with pytest.raises(AssertionError):
        cd.check_case(c.ref32[:-1], c, "f32", kinds)
