"""als_recommend on the GPU: fused top-N from the resident factors, compared EXACTLY with numpy.

Expected values come from numpy only: java_float_dots (the Java-float restatement of FeatureCollector.java:90-101 in
test_host.py), a mask for the exclusions, np.lexsort((position, -score)) per user -- never from als_predict or any code
under test. idx is compared with array_equal, scores with array_equal on the floats, padding is -1 / -inf.
Reference semantics: include/als.h (als_recommend).
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_host import java_float_dots

pytestmark = pytest.mark.gpu

SIDE_MOVIE, SIDE_USER = 0, 1
N_U_TABLE, N_M_TABLE = 160, 20_100       # factor tables larger than any queried set


@pytest.fixture(scope="module")
def gpu(cfk):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return cfk


def make_engine(cfk, k, precision, U, M):
    eng = cfk.ALSEngine(k, precision)
    eng.alloc_factors(SIDE_USER, U.shape[0])
    eng.alloc_factors(SIDE_MOVIE, M.shape[0])
    eng.write_factors(SIDE_USER, U)
    eng.write_factors(SIDE_MOVIE, M)
    return eng


def expected_topn(S, n, excl=None):
    """numpy top-n of a score matrix S [users, candidates]: higher score first, ties by the smaller position."""
    nu, nc = S.shape
    idx = np.full((nu, n), -1, np.int32)
    score = np.full((nu, n), -np.inf, np.float32)
    for u in range(nu):
        keep = np.ones(nc, bool)
        if excl is not None:
            keep[excl[1][excl[0][u]:excl[0][u + 1]]] = False
        pos = np.nonzero(keep)[0]
        order = pos[np.lexsort((pos, -S[u, pos]))][:n]
        idx[u, :len(order)] = order
        score[u, :len(order)] = S[u, order]
    return idx, score


def check(eng, S, urows, mrows, n, excl=None):
    idx, score = eng.recommend(urows, mrows, n, excl)
    want_idx, want_score = expected_topn(S, n, excl)
    assert idx.dtype == np.int32 and score.dtype == np.float32 and idx.shape == (len(urows), n)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(score, want_score)


def csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.concatenate([np.asarray(x, np.int32) for x in lists]) if lists else np.zeros(0, np.int32)
    return ptr, idx.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# parity ladder
# ---------------------------------------------------------------------------------------------------------------------
CONFIGS = [("f32", 1), ("f32", 5), ("f32", 64), ("f32", 128), ("f32", 200), ("f64", 10)]
SHAPES = [(1, 1, 1), (3, 7, 10), (70, 333, 10), (130, 1000, 64), (5, 5000, 1), (16, 20000, 33)]
_tables = {}


def tables(cfk, precision, k):
    """One engine and one pair of factor tables per (precision, k), shared by every shape; never modified."""
    key = (precision, k)
    if key not in _tables:
        rng = np.random.default_rng(1000 + k)
        dt = np.float32 if precision == "f32" else np.float64
        U = rng.standard_normal((N_U_TABLE, k)).astype(dt)
        M = rng.standard_normal((N_M_TABLE, k)).astype(dt)     # f64: not float-representable, narrowed by the engine
        _tables[key] = (make_engine(cfk, k, precision, U, M), U, M)
    return _tables[key]


def query_rows(rng, n_table, n, repeats):
    """A shuffled subset of the table's rows with `repeats` of them listed twice (when n allows)."""
    repeats = min(repeats, n // 2)
    rows = rng.choice(n_table, n - repeats, replace=False)
    rows = np.concatenate([rows, rng.choice(rows, repeats, replace=False)]) if repeats else rows
    return rng.permutation(rows).astype(np.int64)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("precision,k", CONFIGS)
def test_parity_ladder(gpu, precision, k, shape):
    n_users, n_cand, top_n = shape
    eng, U, M = tables(gpu, precision, k)
    rng = np.random.default_rng(n_users * 7 + n_cand)
    urows = query_rows(rng, N_U_TABLE, n_users, 1)
    mrows = query_rows(rng, N_M_TABLE, n_cand, 5)             # repeats: equal scores at different positions
    check(eng, java_float_dots(U[urows], M[mrows]), urows, mrows, top_n)


def test_ladder_runs_both_launch_shapes(gpu):
    eng, _, _ = tables(gpu, "f32", 5)
    S = [eng.recommend_plan(nu, nc, n)["segments"] for nu, nc, n in SHAPES]
    assert any(s > 1 for s in S) and any(s == 1 for s in S), S
    p = eng.recommend_plan(16, 20000, 33)
    assert p["user_tile"] >= 1 and p["segment_len"] * p["segments"] >= 20000 and 0 < p["lds_bytes"] <= 160 * 1024


def test_single_segment_sweep_over_many_tiles(gpu):
    """Enough query users that the plan keeps S = 1 (the user tiles fill the device): one workgroup sweeps every candidate
    tile, the queues overflow and merge along the way, and the last user tile is ragged."""
    eng, U, M = tables(gpu, "f32", 5)
    rng = np.random.default_rng(11)
    n_users = 64 * 1100 + 5
    assert eng.recommend_plan(n_users, 333, 10)["segments"] == 1
    urows = rng.integers(0, N_U_TABLE, n_users).astype(np.int64)
    mrows = query_rows(rng, N_M_TABLE, 333, 5)
    idx, score = eng.recommend(urows, mrows, 10)
    want_idx, want_score = expected_topn(java_float_dots(U, M[mrows]), 10)      # per table row, then per query user
    assert np.array_equal(idx, want_idx[urows]) and np.array_equal(score, want_score[urows])


# ---------------------------------------------------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------------------------------------------------
def test_all_zero_user_row_takes_the_first_positions(gpu):
    rng = np.random.default_rng(3)
    U = np.zeros((2, 5), np.float32)
    U[1] = 1.0
    M = rng.standard_normal((500, 5)).astype(np.float32)
    eng = make_engine(gpu, 5, "f32", U, M)
    mrows = rng.permutation(500).astype(np.int64)
    for n in (1, 10, 64):
        idx, score = eng.recommend([0, 1], mrows, n)
        assert np.array_equal(idx[0], np.arange(n)) and np.all(score[0] == 0)
        check(eng, java_float_dots(U, M[mrows]), np.array([0, 1]), mrows, n)


def test_three_distinct_movie_rows_repeated(gpu):
    rng = np.random.default_rng(4)
    U = rng.standard_normal((9, 10)).astype(np.float32)
    M = np.tile(rng.standard_normal((3, 10)).astype(np.float32), (100, 1))
    eng = make_engine(gpu, 10, "f32", U, M)
    urows, mrows = np.arange(9), np.arange(300)
    for n in (7, 64):
        check(eng, java_float_dots(U, M), urows, mrows, n)


def test_signed_zero_products_are_one_tie_class(gpu):
    """Products of both zero signs (1 * -0 = -0, -1 * -0 = +0, 1 * 0 = +0): the comparison is a float comparison, so
    +0.0 and -0.0 are one tie class ordered by position alone. (The score itself is always +0.0 here, as in als_predict:
    the chain starts from +0.0f and +0 + -0 = +0 in round-to-nearest, so a -0.0 total cannot arise; the returned sign
    bits are compared all the same.)"""
    U1 = np.array([[1.0], [-1.0], [0.0], [-0.0]], np.float32)
    M1 = np.zeros((40, 1), np.float32)
    M1[::3, 0] = -0.0
    M1[5, 0] = 2.0
    M1[6, 0] = -2.0
    prod = np.outer(U1[:, 0], M1[:, 0])
    assert np.any(np.signbit(prod) & (prod == 0)) and np.any(~np.signbit(prod) & (prod == 0))
    S = java_float_dots(U1, M1)
    eng1 = make_engine(gpu, 1, "f32", U1, M1)
    check(eng1, S, np.arange(4), np.arange(40), 12)
    _, score = eng1.recommend(np.arange(4), np.arange(40), 12)
    assert np.array_equal(np.signbit(score), np.signbit(expected_topn(S, 12)[1]))     # predict's bits, sign included
    # two features, so that a -0 product meets a running +0 and a running negative total
    U2 = np.array([[1.0, -1.0], [-1.0, 0.0]], np.float32)
    M2 = np.zeros((30, 2), np.float32)
    M2[::2, 0] = -0.0
    M2[1::4, 1] = -0.0
    eng2 = make_engine(gpu, 2, "f32", U2, M2)
    check(eng2, java_float_dots(U2, M2), np.arange(2), np.arange(30), 10)


# ---------------------------------------------------------------------------------------------------------------------
# insertion stress
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 10, 64])
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_insertion_stress(gpu, order, n):
    """k = 1, U = [1]: ascending candidates all beat the threshold (most merges and queue flushes), descending ones
    never do after the first n."""
    vals = np.sort(np.random.default_rng(6).standard_normal(3000).astype(np.float32))
    M = (vals if order == "ascending" else vals[::-1]).reshape(-1, 1).copy()
    U = np.ones((1, 1), np.float32)
    eng = make_engine(gpu, 1, "f32", U, M)
    check(eng, java_float_dots(U, M), np.zeros(1, np.int64), np.arange(3000), n)
    # the same through one workgroup per user tile (S = 1): many users, each sweeping all 47 tiles
    urows = np.zeros(64 * 300, np.int64)
    assert eng.recommend_plan(len(urows), 3000, n)["segments"] == 1
    idx, score = eng.recommend(urows, np.arange(3000), n)
    want_idx, want_score = expected_topn(java_float_dots(U, M), n)
    assert np.array_equal(idx, np.repeat(want_idx, len(urows), 0)) and np.array_equal(score, np.repeat(want_score, len(urows), 0))


# ---------------------------------------------------------------------------------------------------------------------
# exclusions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def excl_case(gpu):
    eng, U, M = tables(gpu, "f32", 5)
    rng = np.random.default_rng(8)
    out = {}
    for name, (nu, nc) in {"small": (70, 333), "split": (6, 5000)}.items():
        urows = query_rows(rng, N_U_TABLE, nu, 1)
        mrows = query_rows(rng, N_M_TABLE, nc, 5)
        out[name] = (urows, mrows, java_float_dots(U[urows], M[mrows]))
    return eng, out


@pytest.mark.parametrize("case", ["small", "split"])
def test_exclusions(excl_case, case):
    eng, cases = excl_case
    urows, mrows, S = cases[case]
    nu, nc = S.shape
    n = 10
    rng = np.random.default_rng(9)
    check(eng, S, urows, mrows, n, csr([[] for _ in range(nu)]))                       # empty sets
    idx, score = eng.recommend(urows, mrows, n, csr([np.arange(nc)] * nu))              # everything excluded
    assert np.all(idx == -1) and np.all(np.isneginf(score))
    top = expected_topn(S, n)[0]
    check(eng, S, urows, mrows, n, csr([np.sort(t) for t in top]))                     # exactly the top n: the next n
    big = [np.sort(rng.choice(nc, int(rng.integers(n + 1, nc // 2)), replace=False)) for _ in range(nu)]
    check(eng, S, urows, mrows, n, csr(big))                                           # random sets larger than n
    mixed = [b if u % 2 else [] for u, b in enumerate(big)]                            # some users without any
    check(eng, S, urows, mrows, n, csr(mixed))
    almost = [np.setdiff1d(np.arange(nc), t[:3]) for t in top]                         # 3 eligible: padding
    check(eng, S, urows, mrows, n, csr(almost))


def test_exclusions_confined_to_one_segment(excl_case):
    eng, cases = excl_case
    urows, mrows, S = cases["split"]
    plan = eng.recommend_plan(len(urows), len(mrows), 10)
    assert plan["segments"] > 2
    lo, hi = plan["segment_len"], min(2 * plan["segment_len"], len(mrows))             # the second segment, whole
    check(eng, S, urows, mrows, 10, csr([np.arange(lo, hi)] * len(urows)))


def test_rebased_exclusion_pointers(gpu):
    """excl_ptr[0] = 3: the ranges index a slice behind three entries the call never reads (invalid positions here).
    Positions and score bits are those of the same exclusions given from excl_ptr[0] = 0, and numpy's."""
    eng, U, M = tables(gpu, "f32", 5)
    rng = np.random.default_rng(12)
    urows, mrows = query_rows(rng, N_U_TABLE, 3, 0), query_rows(rng, N_M_TABLE, 50, 5)
    S = java_float_dots(U[urows], M[mrows])
    top = expected_topn(S, 5)[0]
    excl = csr([np.unique(np.append(top[0, :2], 49)), [], np.sort(top[2])])             # part of a top 5, none, all of one
    assert excl[0][0] == 0
    at3 = (excl[0] + 3, np.concatenate([np.array([-3, 50, 7000], np.int32), excl[1]]))
    idx0, score0 = eng.recommend(urows, mrows, 5, excl)
    idx3, score3 = eng.recommend(urows, mrows, 5, at3)
    assert np.array_equal(idx0, idx3) and np.array_equal(score0.view(np.uint32), score3.view(np.uint32))
    want_idx, want_score = expected_topn(S, 5, excl)
    assert np.array_equal(idx3, want_idx) and np.array_equal(score3, want_score)
    assert not np.array_equal(want_idx, top)                                             # the exclusions took effect


# ---------------------------------------------------------------------------------------------------------------------
# the workspace every synchronous call shares
# ---------------------------------------------------------------------------------------------------------------------
def _a256(n):
    return (n + 255) // 256 * 256


def test_shared_workspace_across_every_call(gpu):
    """recommend, rank_targets, fold_in, gram_table, solve_implicit and the first recommend again on one engine (k = 16,
    f32): all five lay their parts out in the one grow-only workspace, each call here needs more of it than the one
    before (the byte counts below restate the layouts of als_plan.cpp and the calls, every part 256-byte aligned), and
    every result is bit for bit that of the same call on an engine that has made no other call."""
    k, row_b = 16, 64
    rng = np.random.default_rng(13)
    U = rng.standard_normal((60, k)).astype(np.float32)
    M = rng.standard_normal((2100, k)).astype(np.float32)               # 9 slabs of 256 rows for the table Gram
    nu, nc, top_n, nt, nq, nnz = 20, 40, 5, 70, 40, 400
    urows, mrows = query_rows(rng, 60, nu, 1), query_rows(rng, 2100, nc, 2)
    excl = csr([np.sort(rng.choice(nc, 6, replace=False)) for _ in range(nu)])
    targets = csr(np.array_split(rng.integers(0, nc, nt).astype(np.int32), nu))
    qptr = np.zeros(nq + 1, np.int64)
    qptr[1:] = np.cumsum(rng.multinomial(nnz, np.ones(nq) / nq))
    qidx = np.concatenate([rng.choice(2100, c, replace=False) for c in np.diff(qptr)]).astype(np.int32)
    queries = (qptr, qidx, rng.integers(1, 6, nnz).astype(np.int16))
    slabs = -(-2100 // 256)
    excl_b = _a256((nu + 1) * 8) + _a256(len(excl[1]) * 4)
    need = [
        _a256(nu * 8) + _a256(nc * 8) + 2 * _a256(nu * top_n * 4) + excl_b,                      # recommend (1 segment)
        _a256(nt * 8) + 4 * _a256(nt * 4) + _a256(nc * 8) + excl_b,                              # rank_targets
        _a256((nq + 1) * 8) + _a256(nnz * 4) + _a256(nnz * 2) + _a256(nq * row_b),               # fold_in
        _a256(k * row_b) + slabs * 256 * 4,                                                      # gram_table
        _a256((nq + 1) * 8) + _a256(nq * 8) + _a256(nnz * 4) + _a256(nnz * 2) + _a256(k * row_b) + slabs * 256 * 4 +
        _a256(nq * row_b),                                                                       # solve_implicit
    ]
    assert need == sorted(set(need)), need
    calls = [
        lambda e: e.recommend(urows, mrows, top_n, excl),
        lambda e: e.rank_targets(urows, mrows, targets, excl),
        lambda e: (e.fold_in(SIDE_USER, queries, 0.05),),
        lambda e: (e.gram_table(SIDE_MOVIE),),
        lambda e: (e.solve_implicit(SIDE_USER, queries, 0.1, 2.0),),
    ]
    shared = make_engine(gpu, k, "f32", U, M)
    assert shared.recommend_plan(nu, nc, top_n)["segments"] == 1
    got = [call(shared) for call in calls + calls[:1]]
    for call, g in zip(calls + calls[:1], got):
        want = call(make_engine(gpu, k, "f32", U, M))
        assert len(g) == len(want)
        for a, b in zip(g, want):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], got[-1]))
    assert np.array_equal(got[0][0], expected_topn(java_float_dots(U[urows], M[mrows]), top_n, excl)[0])
    assert all(np.all(np.isfinite(g[0])) and np.any(g[0] != 0) for g in got[2:5])


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(gpu):
    from cfk_amd._lib import ALSError
    import ctypes
    from cfk_amd import _lib
    eng, _, _ = tables(gpu, "f32", 5)
    u, m = np.arange(3), np.arange(50)
    bad = "ALS_ERR_INVALID_ARGUMENT"
    with pytest.raises(ALSError, match=bad):
        eng.recommend(u, m, 5, (np.array([0, 2, 2, 2]), np.array([7, 3], np.int32)))    # unsorted
    with pytest.raises(ALSError, match=bad):
        eng.recommend(u, m, 5, (np.array([0, 2, 2, 2]), np.array([3, 3], np.int32)))    # duplicate
    with pytest.raises(ALSError, match=bad):
        eng.recommend(u, m, 5, (np.array([0, 0, 1, 1]), np.array([50], np.int32)))      # position >= n_movies
    with pytest.raises(ALSError, match=bad):
        eng.recommend(u, m, 5, (np.array([0, 0, 1, 1]), np.array([-1], np.int32)))
    for n in (0, 65):
        with pytest.raises(ALSError, match=bad):
            eng.recommend(u, m, n)
        with pytest.raises(ALSError, match=bad):
            eng.recommend_plan(3, 50, n)
    with pytest.raises(ALSError, match=bad):
        eng.recommend([N_U_TABLE], m, 5)                                                # row index out of range
    with pytest.raises(ALSError, match=bad):
        eng.recommend(u, [-1], 5)
    # exactly one NULL exclusion pointer
    ur, mr = u.astype(np.int64), m.astype(np.int64)
    idx, score = np.zeros((3, 5), np.int32), np.zeros((3, 5), np.float32)
    ep, ei = np.zeros(4, np.int64), np.zeros(1, np.int32)
    L = _lib.lib()
    args = (eng._h, _lib.ptr(ur, ctypes.c_int64), 3, _lib.ptr(mr, ctypes.c_int64), 50, 5)
    outs = (_lib.ptr(idx, ctypes.c_int32), _lib.ptr(score, ctypes.c_float))
    assert L.als_recommend(*args, _lib.ptr(ep, ctypes.c_int64), None, *outs) == 1
    assert L.als_recommend(*args, None, _lib.ptr(ei, ctypes.c_int32), *outs) == 1
    # nothing to do: ALS_OK, outputs untouched
    idx[:] = 77
    assert L.als_recommend(eng._h, _lib.ptr(ur, ctypes.c_int64), 0, _lib.ptr(mr, ctypes.c_int64), 50, 5, None, None, *outs) == 0
    assert L.als_recommend(eng._h, _lib.ptr(ur, ctypes.c_int64), 3, _lib.ptr(mr, ctypes.c_int64), 0, 5, None, None, *outs) == 0
    assert np.all(idx == 77)
    fresh = gpu.ALSEngine(5, "f32")
    with pytest.raises(ALSError, match="ALS_ERR_STATE"):
        fresh.recommend(u, m, 5)                                                        # before alloc_factors


# ---------------------------------------------------------------------------------------------------------------------
# end to end on the tiny sample
# ---------------------------------------------------------------------------------------------------------------------
def _tiny_app(cfk, tiny_path, precision, k=10, iters=2):
    ds = cfk.Dataset.load_netflix(tiny_path)
    app = cfk.ALSApp(4, k, 0.05, iters, 426, 302, precision=precision, seed=42).setup(ds)
    app.run()
    return ds, app


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_app_recommend_end_to_end(gpu, tiny_path, precision):
    ds, app = _tiny_app(gpu, tiny_path, precision)
    U, M = app.factors()                                                # ascending raw ids
    S = java_float_dots(U, M)
    movie_ids, user_ids = ds.ids(SIDE_MOVIE), ds.ids(SIDE_USER)
    m, u, _ = ds.ratings()
    seen = [np.sort(np.searchsorted(movie_ids, m[u == uid])) for uid in user_ids]
    P = app.prediction_matrix()
    for exclude, excl in ((True, csr(seen)), (False, None)):
        uid, mid, score = app.recommend(10, exclude_seen=exclude)
        want_idx, want_score = expected_topn(S, 10, excl)
        assert np.array_equal(uid, user_ids)
        assert np.array_equal(mid, np.where(want_idx >= 0, movie_ids[np.maximum(want_idx, 0)], -1))
        assert np.array_equal(score, want_score)
        rows = np.arange(len(user_ids))[:, None]
        assert np.array_equal(score.view(np.uint32), P[rows, want_idx].view(np.uint32))      # predict's cells bitwise


# ---------------------------------------------------------------------------------------------------------------------
# non-interference with the solves
# ---------------------------------------------------------------------------------------------------------------------
def test_solve_half_after_recommend_is_unchanged(gpu, tiny_path):
    out = []
    for with_recommend in (False, True):
        ds = gpu.Dataset.load_netflix(tiny_path)
        app = gpu.ALSApp(4, 64, 0.05, 1, precision="f32", seed=7).setup(ds)
        app.movie_half()
        if with_recommend:
            app.recommend(10)
        app.user_half()
        out.append(app.factors())
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_recommend_between_two_chunks_of_a_half(gpu, tiny_path):
    """k = 64 (the half gathers the pre-split table chunk 0 prepared): a recommend call between chunk 0 and chunk 1 of
    the movie half leaves chunk 1's output bitwise unchanged."""
    out = []
    for with_recommend in (False, True):
        ds = gpu.Dataset.load_netflix(tiny_path)
        app = gpu.ALSApp(4, 64, 0.05, 1, precision="f32", seed=7).setup(ds)
        eng = app.engine
        n = app.info[SIDE_MOVIE]["n_rows"]
        eng.set_chunks(SIDE_MOVIE, [0, n // 2, n])
        assert eng.split_info(SIDE_MOVIE)["presplit"]          # the table chunk 0 prepares and chunk 1 reuses
        eng.solve_half_chunk(SIDE_MOVIE, 0.05, 0)
        if with_recommend:
            idx, _ = eng.recommend(np.arange(302), np.arange(426), 64)
            assert idx.shape == (302, 64)
        eng.solve_half_chunk(SIDE_MOVIE, 0.05, 1)
        out.append(eng.read_factors(SIDE_MOVIE))
    assert np.array_equal(out[0], out[1]) and np.any(out[0][n // 2:] != 0)


# ---------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------
def _cli(tiny_path, out, *flags):
    app_bin = os.path.join(ROOT, "collaborative-filtering-kafka_amd", "build", "als_app")
    res = subprocess.run([app_bin, "4", "10", "0.05", "2", tiny_path, "426", "302", "--gpus", "1", "--out", str(out),
                          *flags], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return sorted(os.listdir(out))


def test_cli_top_n_and_no_matrix(gpu, tiny_path, tmp_path):
    files = _cli(tiny_path, tmp_path / "rec", "--top-n", "5", "--no-matrix")
    assert len(files) == 1 and files[0].startswith("recommendations_")       # no prediction_matrix_* file
    lines = [ln.split(",") for ln in (tmp_path / "rec" / files[0]).read_text().splitlines()]
    _, app = _tiny_app(gpu, tiny_path, "f32")
    uid, mid, score = app.recommend(5)
    cells = [(i, j) for i in range(len(uid)) for j in range(5) if mid[i, j] >= 0]
    assert [(int(a), int(b)) for a, b, _ in lines] == [(int(uid[i]), int(mid[i, j])) for i, j in cells]
    assert [np.float32(float(s)) for _, _, s in lines] == [score[i, j] for i, j in cells]


def test_cli_without_the_new_flags_writes_what_it_wrote(gpu, tiny_path, tmp_path):
    files = _cli(tiny_path, tmp_path / "plain")
    assert len(files) == 1 and files[0].startswith("prediction_matrix_")


# ---------------------------------------------------------------------------------------------------------------------
# JNI: AlsNative.recommend's native through the mock JVM
# ---------------------------------------------------------------------------------------------------------------------
def test_jni_recommend_equals_the_engine(gpu):
    from test_jni_shim import JavaException, MockJVM
    from test_recommend_host import bind_recommend0
    eng, U, M = tables(gpu, "f32", 5)
    jvm = MockJVM()
    bind_recommend0(jvm)
    rng = np.random.default_rng(21)
    urows, mrows, n = query_rows(rng, N_U_TABLE, 9, 1), query_rows(rng, N_M_TABLE, 700, 5), 7
    excl = csr([np.sort(rng.choice(700, 40, replace=False)) for _ in range(9)])
    for ex in (excl, None):
        want_idx, want_score = eng.recommend(urows, mrows, n, ex)
        out_idx, out_score = jvm.array_zeros(np.int32, 9 * n), jvm.array_zeros(np.float32, 9 * n)
        ja = [jvm.array(urows), jvm.array(mrows)]
        je = [jvm.array(ex[0]), jvm.array(ex[1])] if ex else [None, None]
        jvm.call("recommend0", eng._h.value, ja[0], ja[1], n, je[0], je[1], out_idx, out_score)
        assert np.array_equal(jvm.read(out_idx, np.int32).reshape(9, n), want_idx)
        assert np.array_equal(jvm.read(out_score, np.float32).reshape(9, n), want_score)
        check(eng, java_float_dots(U[urows], M[mrows]), urows, mrows, n, ex)          # and both equal numpy
        with pytest.raises(JavaException) as ei:                                       # a wrong-length outIdx
            jvm.call("recommend0", eng._h.value, ja[0], ja[1], n, je[0], je[1], jvm.array_zeros(np.int32, 9 * n - 1),
                     out_score)
        assert ei.value.cls == "java/lang/IllegalArgumentException" and "outIdx" in ei.value.msg
    with pytest.raises(JavaException, match="als_recommend: als_status 1"):            # the ABI's checks surface too
        jvm.call("recommend0", eng._h.value, jvm.array(urows), jvm.array(mrows), 65, None, None,
                 jvm.array_zeros(np.int32, 9 * 65), jvm.array_zeros(np.float32, 9 * 65))
    st = jvm.stats()
    assert st["violations"] == 0 and st["open_critical"] == 0
