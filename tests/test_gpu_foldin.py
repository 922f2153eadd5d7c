"""als_fold_in on the GPU: factor rows of queries that were never in a block, every row against the fp64 oracle.

The yardstick is the degree ladder of rowshapes.py (344 rows as 344 queries: degrees 1..330, the twelve rows around 1k
to 4k entries, two empty rows, 77,143 entries over 4,096 opposite rows) with rowshapes.check_rows: 1e-4 per row in fp32,
1e-8 in fp64, empty rows exactly zero, fp32 p99 <= max(2 x the reference's own fp32 p99, 2e-5). test_rowshapes_host.py
proves on the CPU that the reference's fp32 arithmetic stays 5 x inside that bound on this ladder and every one-entry
mutant 5 x outside it, for exactly the (k, lambda) pairs used here: a kernel that drops a batch's last entry, mis-zeroes
a tail or leaks LDS between queries fails. Every case prints its worst row before it asserts.

Measured on an MI355X, largest per-row error (the reference's own fp32 arithmetic on the same rows in brackets): fp32
k = 32 1.9e-6 (2.7e-6), k = 128 1.7e-6 (5.6e-6), k = 64 / 128 at lambda = 1 1.2e-6 (1.2e-6 / 1.3e-6); fp64 k = 10 / 64 /
128 4.2e-15 / 8.2e-15 / 1.1e-14; the 5,000-query case 2.0e-6. The module takes 2 s.

Reference semantics: include/als.h (als_fold_in). The launch plan is restated in test_foldin_host.py.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rowshapes as rs
from test_foldin_host import foldin_plan
from test_gpu_recommend import expected_topn

pytestmark = pytest.mark.gpu

SIDE_MOVIE, SIDE_USER = 0, 1
F32_CASES = [(10, 0.05), (32, 0.05), (40, 0.05), (64, 0.05), (128, 0.05), (64, 1.0), (128, 1.0)]
F64_KS = [10, 64, 128]
# rows of the default ladder: degree d at row d - 1, the empty rows at 330 and 343, the long rows from 331
ALONE_ROWS = (0, 31, 32, 329, 331 + rs.LONG_DEGS.index(1025), 331 + rs.LONG_DEGS.index(4000), 330, 343)


@pytest.fixture(scope="module")
def gpu(cfk):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return cfk


@functools.lru_cache(maxsize=None)
def inputs(k, lam, sort_cols=True, rows=0):
    """(ladder, opposite factors, fp64 oracle, the reference's fp32 result): computed once per case, read-only."""
    lad = rs.anyk_ladder(k, rows) if rows else rs.ladder_block(sort_cols=sort_cols)
    F = rs.factors(lad.n_opp, k)
    ref64, ref32 = rs.references(lad.side, F, lam)
    for a in (F, ref64, ref32):
        a.setflags(write=False)
    return lad, F, ref64, ref32


_engines = {}


def engine(cfk, precision, k, n_opp=rs.N_OPP):
    """One engine per (precision, k, table) with the movie factors of rowshapes.factors resident; never modified."""
    key = (precision, k, n_opp)
    if key not in _engines:
        with rs.knobs({}):
            eng = cfk.ALSEngine(k, precision)
        eng.alloc_factors(SIDE_MOVIE, n_opp)
        eng.write_factors(SIDE_MOVIE, rs.factors(n_opp, k))
        _engines[key] = eng
    return _engines[key]


def queries(lad, rows=None):
    """The ladder's rows (or the given ones, in that order) as a fold-in CSR."""
    blk = lad.blk
    if rows is None:
        return blk["row_ptr"], blk["col"], blk["ratings"]
    rp = blk["row_ptr"]
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([rp[r + 1] - rp[r] for r in rows])
    idx = np.concatenate([blk["col"][rp[r]:rp[r + 1]] for r in rows] + [np.zeros(0, np.int32)])
    rat = np.concatenate([blk["ratings"][rp[r]:rp[r + 1]] for r in rows] + [np.zeros(0, np.int16)])
    return ptr, idx.astype(np.int32), rat.astype(np.int16)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check_ladder(eng, precision, k, lam, sort_cols=True):
    lad, _, ref64, ref32 = inputs(k, lam, sort_cols)
    got = eng.fold_in(SIDE_USER, queries(lad), lam)
    assert got.shape == (len(lad.degs), k) and got.dtype == eng.np_dtype
    rel = rs.row_errors(got, ref64)
    ref_rel = rs.row_errors(ref32, ref64)
    rated = lad.degs > 0
    print(f"\n[foldin] {precision} k={k} lam={lam} sorted={sort_cols}: per-row max {rel[rated].max():.2e} (row of "
          f"{lad.degs[rated][rel[rated].argmax()]}), p99 {np.percentile(rel[rated], 99):.2e}; reference fp32 max "
          f"{ref_rel[rated].max():.2e}, p99 {np.percentile(ref_rel[rated], 99):.2e}; buckets {rs.bucket_max(rel, lad.degs)}")
    rs.check_rows(got, ref64, ref32, lad.degs, precision)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the ladder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort_cols", [True, False], ids=["sorted", "drawn"])
@pytest.mark.parametrize("k,lam", F32_CASES, ids=[f"k{k}-lam{lam:g}" for k, lam in F32_CASES])
def test_ladder_fp32(gpu, k, lam, sort_cols):
    eng = engine(gpu, "f32", k)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert eng.fold_in_plan(344) == foldin_plan(eng.kp, 4, 344, cu)
    check_ladder(eng, "f32", k, lam, sort_cols)


@pytest.mark.parametrize("k", F64_KS)
def test_ladder_fp64(gpu, k):
    eng = engine(gpu, "f64", k)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert eng.fold_in_plan(344) == foldin_plan(eng.kp, 8, 344, cu)
    check_ladder(eng, "f64", k, 0.05)


# ---------------------------------------------------------------------------------------------------------------------
# 3: a query's bits do not depend on the call it is in
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,k", [("f32", 64), ("f32", 128), ("f64", 64)])
def test_batch_independence(gpu, precision, k):
    eng = engine(gpu, precision, k)
    lad, _, _, _ = inputs(k, 0.05)
    n = len(lad.degs)
    assert [int(lad.degs[r]) for r in ALONE_ROWS] == [1, 32, 33, 330, 1025, 4000, 0, 0]
    whole = eng.fold_in(SIDE_USER, queries(lad), 0.05)
    for r in ALONE_ROWS:
        alone = eng.fold_in(SIDE_USER, queries(lad, [r]), 0.05)
        assert np.array_equal(bits(alone[0]), bits(whole[r])), (r, int(lad.degs[r]))
    rev = eng.fold_in(SIDE_USER, queries(lad, list(range(n - 1, -1, -1))), 0.05)
    assert np.array_equal(bits(rev[::-1]), bits(whole))
    again = eng.fold_in(SIDE_USER, queries(lad), 0.05)
    assert np.array_equal(bits(again), bits(whole))


def test_more_queries_than_workgroups(gpu):
    """5,000 queries of degrees 1..40 cycling over 512 opposite rows at k = 64: the grid-stride loop reuses a
    workgroup's LDS for several queries."""
    k, rows = 64, 5000
    lad, _, ref64, ref32 = inputs(k, 0.05, True, rows)
    eng = engine(gpu, "f32", k, lad.n_opp)
    assert eng.fold_in_plan(rows)["workgroups"] < rows
    got = eng.fold_in(SIDE_USER, queries(lad), 0.05)
    rel = rs.check_rows(got, ref64, ref32, lad.degs, "f32")
    print(f"\n[foldin] 5000 queries: per-row max {rel.max():.2e}")
    first = eng.fold_in(SIDE_USER, queries(lad, list(range(344))), 0.05)
    assert np.array_equal(bits(first), bits(got[:344]))


# ---------------------------------------------------------------------------------------------------------------------
# 4: device rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 40])
def test_device_rows(gpu, k):
    n_trained, n_spare = 30, 20
    lad = rs.ladder_block((1, 2, 3, 9, 16, 31, 32, 0, 33, 64, 65, 130), n_opp=512, seed=5)
    F = rs.factors(lad.n_opp, k)
    with rs.knobs({}):
        eng = gpu.ALSEngine(k, "f32")
    try:
        assert eng.kp == (16 if k == 10 else 64)
        eng.alloc_factors(SIDE_MOVIE, lad.n_opp)
        eng.write_factors(SIDE_MOVIE, F)
        U = eng.alloc_factors(SIDE_USER, n_trained + n_spare)
        n_rows = n_trained + n_spare
        pattern = (1000.0 + torch.arange(n_rows * eng.kp, dtype=torch.float32, device=U.device)).reshape(n_rows, eng.kp)
        U[:n_rows].copy_(pattern)                  # every row but the sentinel, padded columns included
        torch.cuda.synchronize()
        before = U.cpu().numpy().copy()
        rng = np.random.default_rng(8)
        nq = len(lad.degs)
        dst = (n_trained + rng.permutation(n_spare)[:nq]).astype(np.int64)
        got = eng.fold_in(SIDE_USER, queries(lad), 0.05, dst_rows=dst)
        ref64, ref32 = rs.references(lad.side, F, 0.05)
        rs.check_rows(got, ref64, ref32, lad.degs, "f32")
        after = U.cpu().numpy()
        assert np.array_equal(bits(after[dst, :k]), bits(got))
        assert not after[dst, k:].any()
        others = np.setdiff1d(np.arange(n_rows + 1), dst)
        assert np.array_equal(bits(after[others]), bits(before[others]))
        assert not after[n_rows].any()                                          # the sentinel row
        # device rows only: other destinations, no host result
        dst2 = rng.permutation(n_trained)[:nq].astype(np.int64)
        assert eng.fold_in(SIDE_USER, queries(lad), 0.05, dst_rows=dst2, return_host=False) is None
        after2 = U.cpu().numpy()
        assert np.array_equal(bits(after2[dst2, :k]), bits(got)) and not after2[dst2, k:].any()
        others = np.setdiff1d(np.arange(n_rows + 1), dst2)
        assert np.array_equal(bits(after2[others]), bits(after[others]))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5: the serving path on the tiny sample
# ---------------------------------------------------------------------------------------------------------------------
def test_serving_path(gpu, tiny_path, oracle_mod):
    k, lam, n_new, top_n = 10, 0.05, 3, 10
    full = gpu.Dataset.load_netflix(tiny_path)
    m, u, r = full.ratings()
    user_ids = full.ids(SIDE_USER)
    new_ids = user_ids[[5, 100, 250]]
    held = np.isin(u, new_ids)
    ds = gpu.Dataset.from_ratings(m[~held], u[~held], r[~held])
    users = [[(int(mm), int(rr)) for mm, rr in zip(m[u == uid], r[u == uid])] for uid in new_ids]
    assert all(len(x) > 0 for x in users)
    app = gpu.ALSApp(4, k, lam, 2, precision="f32", seed=42).setup(ds, spare_user_rows=n_new)
    app.run()
    eng = app.engine
    movie_ids, movie_rows = ds.ids(SIDE_MOVIE), ds.slots(SIDE_MOVIE, 1)
    base = app.info[SIDE_USER]["n_slots"]
    assert eng.factors[SIDE_USER].shape[0] == base + n_new + 1

    # fold-in against the oracle on the M read back
    q_ptr, q_idx, q_rat, excl_ptr, excl_idx, n_unknown = gpu.foldin_queries(ds, 1, movie_rows, users)
    M = eng.read_factors(SIDE_MOVIE).astype(np.float64)
    side = oracle_mod.Side(np.arange(1, n_new + 1, dtype=np.int64), q_ptr.copy(), q_idx.copy(), q_rat.copy())
    ref64 = oracle_mod.update_side(side, M, lam, "f64")
    X = app.fold_in(users)
    rel = rs.row_errors(X, ref64)
    print(f"\n[foldin] serving: per-row errors {rel}, unknown movie ids {n_unknown}")
    assert X.shape == (n_new, k) and (rel <= rs.BOUND["f32"]).all()

    # recommend over the spare rows = host top-N of predict's cells under the documented order
    rows = base + np.arange(n_new, dtype=np.int64)
    X2 = eng.fold_in(SIDE_USER, (q_ptr, q_idx, q_rat), app.ALS_LAMBDA, dst_rows=rows)
    assert np.array_equal(bits(X2), bits(X))
    P = eng.predict(rows, movie_rows)
    for excl in ((excl_ptr, excl_idx), None):
        idx, score = eng.recommend(rows, movie_rows, top_n, excl)
        want_idx, want_score = expected_topn(P, top_n, excl)
        assert np.array_equal(idx, want_idx) and np.array_equal(bits(score), bits(want_score))
        mids, sc = app.recommend_for(users, top_n, exclude_seen=excl is not None)
        assert np.array_equal(mids, np.where(want_idx >= 0, movie_ids[np.maximum(want_idx, 0)], -1))
        assert np.array_equal(bits(sc), bits(want_score))
        if excl is not None:
            for i, pairs in enumerate(users):
                assert not set(mids[i].tolist()) & {mm for mm, _ in pairs}
    # the trained users are where they were
    U, _ = app.factors()
    assert U.shape == (len(ds.ids(SIDE_USER)), k)


# ---------------------------------------------------------------------------------------------------------------------
# 6: a call between two chunks of a half
# ---------------------------------------------------------------------------------------------------------------------
def test_fold_in_between_two_chunks_of_a_half(gpu):
    k, lam, n_spare = 64, 0.05, 20
    lad, F, _, _ = inputs(k, lam)
    n = len(lad.degs)
    out = []
    for with_fold_in in (False, True):
        with rs.knobs({}):
            eng = gpu.ALSEngine(k, "f32")
        try:
            eng.alloc_factors(SIDE_MOVIE, lad.n_opp)
            eng.alloc_factors(SIDE_USER, n + n_spare)
            eng.write_factors(SIDE_MOVIE, F)
            eng.set_block(SIDE_USER, lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"], 0, lad.n_opp)
            assert eng.block_stats(SIDE_USER)["n_reduce"] > 0           # split rows: partial slots are in flight
            eng.set_chunks(SIDE_USER, [0, n // 2, n])
            eng.solve_half_chunk(SIDE_USER, lam, 0)
            if with_fold_in:
                rows = list(range(0, n, 18))
                x = eng.fold_in(SIDE_USER, queries(lad, rows), lam, dst_rows=n + np.arange(len(rows)))
                assert x.shape == (len(rows), k) and len(rows) <= n_spare
            eng.solve_half_chunk(SIDE_USER, lam, 1)
            out.append(eng.read_factors(SIDE_USER, 0, n))
            assert eng.integrity_status() == [0, 0, 0, 0]
        finally:
            eng.close()
    assert np.array_equal(bits(out[0]), bits(out[1])) and np.any(out[0][n // 2:] != 0)


# ---------------------------------------------------------------------------------------------------------------------
# 7: errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(gpu):
    from cfk_amd import _lib
    L = _lib.lib()
    k, lam = 32, 0.05
    lad, F, _, _ = inputs(k, lam)
    n_user_rows = 8
    with rs.knobs({}):
        eng = gpu.ALSEngine(k, "f32")
        bare = gpu.ALSEngine(k, "f32")
        wide = gpu.ALSEngine(130, "f32")
    qp = np.array([0, 2, 3], np.int64)
    qi = np.array([5, 6, 7], np.int32)
    qr = np.array([1, 2, 3], np.int16)
    out = np.full((2, k), 7.0, np.float32)
    dst = np.array([1, 3], np.int64)

    def p(a, ct):
        return None if a is None else a.ctypes.data_as(ctypes.POINTER(ct))

    def raw(e, side=SIDE_USER, n=2, ptr=qp, idx=qi, rat=qr, dst_rows=None, host=out, ld=k):
        st = L.als_fold_in(e._h, side, n, p(ptr, ctypes.c_int64), p(idx, ctypes.c_int32), p(rat, ctypes.c_int16),
                           ctypes.c_float(lam), p(dst_rows, ctypes.c_int64),
                           None if host is None else host.ctypes.data_as(ctypes.c_void_p), ld)
        return st, L.als_last_error().decode()

    try:
        eng.alloc_factors(SIDE_MOVIE, lad.n_opp)
        eng.write_factors(SIDE_MOVIE, F)
        assert raw(eng)[0] == 0 and not (out == 7.0).any()                      # the valid call the cases vary
        out.fill(7.0)
        # state: dst_rows without this side's factors; no opposite factors at all
        st, msg = raw(eng, dst_rows=dst)
        assert st == 5 and "side 1" in msg, msg
        assert raw(bare)[0] == 5
        eng.alloc_factors(SIDE_USER, n_user_rows)
        INVALID = [
            ("bad side", dict(side=2), None),
            ("negative n_queries", dict(n=-1), None),
            ("NULL q_ptr", dict(ptr=None), None),
            ("NULL q_idx", dict(idx=None), None),
            ("NULL q_ratings", dict(rat=None), None),
            ("decreasing q_ptr", dict(ptr=np.array([0, 2, 1], np.int64)), "query 1"),
            ("index past the table", dict(idx=np.array([5, 6, lad.n_opp], np.int32)), "query 1"),
            ("negative index", dict(idx=np.array([5, -1, 7], np.int32)), "query 0"),
            ("2^31 entries", dict(ptr=np.array([0, 2, 1 << 31], np.int64)), "2^31"),
            ("both outputs NULL", dict(host=None), None),
            ("out_ld < num_features", dict(ld=k - 1), "out_ld"),
            ("dst row past the table", dict(dst_rows=np.array([1, n_user_rows], np.int64)), "query 1"),
            ("negative dst row", dict(dst_rows=np.array([-1, 2], np.int64)), "query 0"),
            ("repeated dst row", dict(dst_rows=np.array([4, 4], np.int64)), "query 1"),
        ]
        U_before = eng.factors[SIDE_USER].cpu().numpy().copy()
        for name, kw, needle in INVALID:
            st, msg = raw(eng, **kw)
            assert st == 1, (name, st, msg)
            assert needle is None or needle in msg, (name, msg)
            assert (out == 7.0).all(), name                                     # a failed call writes nothing
            assert np.array_equal(eng.factors[SIDE_USER].cpu().numpy(), U_before), name
            check_ladder(eng, "f32", k, lam)                                    # and leaves the engine usable
        # widths
        wide.alloc_factors(SIDE_MOVIE, 16)
        st, msg = raw(wide, host=np.zeros((2, 130), np.float32), ld=130)
        assert st == 2 and "128" in msg, msg
        info = (ctypes.c_int64 * 4)()
        assert L.als_fold_in_plan(wide._h, 2, info) == 2 and L.als_fold_in_plan(eng._h, -1, info) == 1
        assert L.als_fold_in_plan(eng._h, 2, None) == 1
        check_ladder(eng, "f32", k, lam)
        # nothing to do
        assert raw(eng, n=0, dst_rows=dst)[0] == 0 and raw(eng, n=0, ptr=None, idx=None, rat=None)[0] == 0
        assert (out == 7.0).all() and np.array_equal(eng.factors[SIDE_USER].cpu().numpy(), U_before)
        # a rebased q_ptr: the same two queries behind three unused entries
        st, _ = raw(eng, ptr=qp + 3, idx=np.concatenate([np.array([9, 9, 9], np.int32), qi]),
                    rat=np.concatenate([np.array([5, 5, 5], np.int16), qr]))
        rebased = out.copy()
        assert st == 0 and raw(eng)[0] == 0 and np.array_equal(bits(rebased), bits(out))
        # the Python wrapper raises the same statuses
        with pytest.raises(gpu.ALSError) as e:
            eng.fold_in(SIDE_USER, (qp, np.array([5, 6, lad.n_opp], np.int32), qr), lam)
        assert e.value.status == 1 and "query 1" in str(e.value)
    finally:
        for e in (eng, bare, wide):
            e.close()
