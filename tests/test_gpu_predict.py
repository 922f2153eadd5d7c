"""als_predict on the GPU: the collector's U M^T cells, compared EXACTLY with numpy.

Expected values come only from java_float_dots (the Java-float restatement of FeatureCollector.java:90-101 in
test_host.py: every product and every partial sum rounded to float, features in ascending order), fp64 tables narrowed
to float first -- never from any code under test. The tables hold signed standard-normal values, so the sums cancel and
a fused multiply-add or another summation order shows in the last bit; they are larger than any queried set, and the
queries are shuffled, repeat rows, and name row 0 and the last row of each table.

Shapes: one cell, tiles of 16 x 16 with and without ragged edges, one user or one movie against many. k: the tile
kernel at 1, 5, 16, 17, 64, 127 and 128 (its 129-float row pitch), fp64 engines at a stride of 64, 96 (a generic-solve
engine whose predict still uses the tile kernel) and 128, and als_predict_generic at fp32 129, 200, 1024 and fp64 200.
include/als.h defines a recommend score as exactly als_predict's cell: one case holds als_recommend to the same numpy
cells. The 110 cases of the module together take 1 s on an MI355X.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_host import java_float_dots

pytestmark = pytest.mark.gpu

SIDE_MOVIE, SIDE_USER = 0, 1
N_U_TABLE, N_M_TABLE = 389, 467          # factor tables larger than any queried set, no multiple of 16
CONFIGS = [("f32", k) for k in (1, 5, 16, 17, 64, 127, 128, 129, 200, 1024)] + \
          [("f64", k) for k in (10, 64, 96, 128, 200)]
SHAPES = [(1, 1), (15, 17), (16, 16), (17, 33), (1, 300), (300, 1), (70, 333)]
_tables = {}


@pytest.fixture(scope="module")
def gpu(cfk):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return cfk


def tables(cfk, precision, k):
    """One engine and one pair of factor tables per (precision, k), shared by every shape; never modified."""
    key = (precision, k)
    if key not in _tables:
        rng = np.random.default_rng(2000 + k)
        dt = np.float32 if precision == "f32" else np.float64
        U = rng.standard_normal((N_U_TABLE, k)).astype(dt)
        M = rng.standard_normal((N_M_TABLE, k)).astype(dt)     # f64: not float-representable, narrowed by the kernel
        eng = cfk.ALSEngine(k, precision)
        eng.alloc_factors(SIDE_USER, N_U_TABLE)
        eng.alloc_factors(SIDE_MOVIE, N_M_TABLE)
        eng.write_factors(SIDE_USER, U)
        eng.write_factors(SIDE_MOVIE, M)
        for a in (U, M):
            a.setflags(write=False)
        _tables[key] = (eng, U, M)
    return _tables[key]


def query_rows(rng, n_table, n, repeats, ends):
    """n rows of the table, shuffled, `repeats` of them listed twice, row 0 and the last row among them (n >= 4); a
    single row: the table's last row or row 0 (`ends`)."""
    if n < 4:
        return np.array(([n_table - 1, 0] if ends else [0, n_table - 1])[:n] + [n_table // 2] * max(n - 2, 0), np.int64)
    repeats = min(repeats, n // 2)
    rows = np.concatenate([[0, n_table - 1], 1 + rng.choice(n_table - 2, n - repeats - 2, replace=False)])
    rows = np.concatenate([rows, rng.choice(rows, repeats, replace=False)])
    return rng.permutation(rows).astype(np.int64)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("precision,k", CONFIGS)
def test_cells_equal_the_java_float_dots(gpu, precision, k, shape):
    n_users, n_movies = shape
    eng, U, M = tables(gpu, precision, k)
    assert eng.kp == gpu.factor_stride(k, precision)
    rng = np.random.default_rng(n_users * 11 + n_movies)
    urows = query_rows(rng, N_U_TABLE, n_users, 3, ends=True)
    mrows = query_rows(rng, N_M_TABLE, n_movies, 5, ends=False)
    assert len(urows) == n_users and len(mrows) == n_movies
    if n_users >= 4:
        assert {0, N_U_TABLE - 1} <= set(urows.tolist()) and len(set(urows.tolist())) < n_users
        assert not np.array_equal(urows, np.sort(urows))
    if n_movies >= 4:
        assert {0, N_M_TABLE - 1} <= set(mrows.tolist()) and len(set(mrows.tolist())) < n_movies
    want = java_float_dots(U[urows], M[mrows])
    got = eng.predict(urows, mrows)
    assert got.dtype == np.float32 and got.shape == (n_users, n_movies)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:4], np.abs(got - want).max())


def test_strides_the_cases_run_on(gpu):
    """fp64 k = 96 and 128 are generic-solve engines (row strides 96 and 128) whose predict is the tile kernel; from
    k = 129 on the cells come from als_predict_generic."""
    assert [gpu.factor_stride(k, "f64") for k in (10, 64, 96, 128, 200)] == [16, 64, 96, 128, 208]
    assert [gpu.factor_stride(k, "f32") for k in (17, 127, 128, 129, 200, 1024)] == [32, 128, 128, 144, 208, 1024]


def _raw_predict(eng, urows, mrows, out):
    from cfk_amd import _lib
    ur = np.ascontiguousarray(urows, np.int64)
    mr = np.ascontiguousarray(mrows, np.int64)
    return _lib.lib().als_predict(eng._h, _lib.ptr(ur, ctypes.c_int64), len(ur), _lib.ptr(mr, ctypes.c_int64), len(mr),
                                  _lib.ptr(out, ctypes.c_float))


@pytest.mark.parametrize("precision,k", [("f32", 64), ("f32", 200)])
def test_contract(gpu, precision, k):
    """No users or no movies: ALS_OK and the output untouched. A row index equal to the table size:
    ALS_ERR_INVALID_ARGUMENT. 1,048,561 users: ALS_ERR_UNSUPPORTED on the host, before any allocation or launch; the
    output is untouched in every refused call."""
    eng, U, M = tables(gpu, precision, k)
    out = np.full(8, -5.0, np.float32)
    some_u, some_m = np.array([3, 0], np.int64), np.array([1, 2, 2, 9], np.int64)
    assert _raw_predict(eng, np.zeros(0, np.int64), some_m, out) == 0 and np.all(out == -5.0)
    assert _raw_predict(eng, some_u, np.zeros(0, np.int64), out) == 0 and np.all(out == -5.0)
    assert _raw_predict(eng, np.array([3, N_U_TABLE], np.int64), some_m, out) == 1 and np.all(out == -5.0)
    assert _raw_predict(eng, some_u, np.array([1, N_M_TABLE, 2, 9], np.int64), out) == 1 and np.all(out == -5.0)
    assert _raw_predict(eng, np.array([-1, 3], np.int64), some_m, out) == 1 and np.all(out == -5.0)
    with pytest.raises(gpu.ALSError) as e:
        eng.predict([N_U_TABLE], [0])
    assert e.value.status == 1 and "ALS_ERR_INVALID_ARGUMENT" in str(e.value)
    assert np.array_equal(eng.predict([N_U_TABLE - 1], [N_M_TABLE - 1]), java_float_dots(U[-1:], M[-1:]))
    big = np.full(1_048_561, -5.0, np.float32)
    assert _raw_predict(eng, np.zeros(1_048_561, np.int64), np.array([0], np.int64), big) == 2
    assert np.all(big == -5.0)
    # the call after the refusals is an ordinary one
    assert _raw_predict(eng, some_u, some_m, out) == 0
    assert np.array_equal(out.reshape(2, 4), java_float_dots(U[some_u], M[some_m]))


@pytest.mark.parametrize("shape,top_n", [((17, 33), 33), ((70, 333), 10)], ids=["17x33-all", "70x333-top10"])
def test_recommend_scores_are_the_same_cells(gpu, shape, top_n):
    """als.h: a recommend score is exactly als_predict's cell. Both against the same numpy cells at fp32 k = 64; with
    top_n = every candidate, each cell of the matrix comes back once through als_recommend."""
    eng, U, M = tables(gpu, "f32", 64)
    rng = np.random.default_rng(shape[0] * 11 + shape[1])
    urows = query_rows(rng, N_U_TABLE, shape[0], 3, ends=True)
    mrows = query_rows(rng, N_M_TABLE, shape[1], 5, ends=False)
    S = java_float_dots(U[urows], M[mrows])
    assert np.array_equal(eng.predict(urows, mrows), S)
    idx, score = eng.recommend(urows, mrows, top_n)
    assert idx.shape == score.shape == (shape[0], top_n) and idx.min() >= 0 and idx.max() < shape[1]
    for u in range(shape[0]):
        pos = np.arange(shape[1])
        order = pos[np.lexsort((pos, -S[u]))][:top_n]      # higher score first, ties toward the smaller position
        assert np.array_equal(idx[u], order), u
        assert np.array_equal(score[u], S[u, order]), u
    if top_n == shape[1]:
        assert np.array_equal(np.sort(idx, axis=1), np.tile(np.arange(top_n), (shape[0], 1)))
