"""The numpy restatement of als_similar (include/als.h): scores and expected top-N lists, from numpy only.

cell(a, b) is als_predict's cell on two rows of one table (test_host.java_float_dots: fp32, every product and every
partial sum rounded, features in order, f64 factors narrowed to float first). Cosine applies, each as one float32
operation of numpy's (IEEE: correctly rounded), the square root of the diagonal cell, the division 1 / that, and the two
products (cell * inv(q)) * inv(c); inv = 0 where the diagonal cell is 0. Nothing here calls the code under test.
"""
import numpy as np

from test_host import java_float_dots


def self_cells(rows):
    """cell(r, r) of every row of `rows` [n, k], float32."""
    R = np.asarray(rows).astype(np.float32)
    total = np.zeros(len(R), np.float32)
    for f in range(R.shape[1]):
        total = (total + (R[:, f] * R[:, f]).astype(np.float32)).astype(np.float32)
    return total


def inv_norms(rows):
    """inv(r) = float32(1) / sqrt(cell(r, r)) in float32, 0 where cell(r, r) == 0."""
    d = self_cells(rows)
    inv = np.zeros(len(d), np.float32)
    nz = d != 0
    root = np.sqrt(d[nz], dtype=np.float32)
    inv[nz] = (np.float32(1.0) / root).astype(np.float32)
    return inv


def similar_scores(table, query_rows, cand_rows, metric="cosine"):
    """score(q, c) of als_similar for rows of `table` [rows, k] (float32 or float64): float32 [n_queries, n_cand]."""
    Q = np.asarray(table)[np.asarray(query_rows, np.int64)]
    C = np.asarray(table)[np.asarray(cand_rows, np.int64)]
    S = java_float_dots(Q, C)
    if metric == "dot":
        return S
    assert metric == "cosine"
    S = (S * inv_norms(Q)[:, None]).astype(np.float32)
    return (S * inv_norms(C)[None, :]).astype(np.float32)


def expected_lists(S, query_rows, cand_rows, n, exclude_self=True):
    """Top-n of the score matrix S under als_recommend's order: a self mask (every position that holds the query's
    slot), then np.lexsort((position, -score)); padded with -1 / -inf."""
    q = np.asarray(query_rows, np.int64)
    c = np.asarray(cand_rows, np.int64)
    idx = np.full((len(q), n), -1, np.int32)
    score = np.full((len(q), n), -np.inf, np.float32)
    for i in range(len(q)):
        pos = np.nonzero(c != q[i])[0] if exclude_self else np.arange(len(c))
        order = pos[np.lexsort((pos, -S[i, pos]))][:n]
        idx[i, :len(order)] = order
        score[i, :len(order)] = S[i, order]
    return idx, score


def fp64_cosine(table, query_rows, cand_rows):
    """The cosine in float64 from the table as given (no narrowing), 0 for a zero row."""
    Q = np.asarray(table, np.float64)[np.asarray(query_rows, np.int64)]
    C = np.asarray(table, np.float64)[np.asarray(cand_rows, np.int64)]
    nq, ncn = np.linalg.norm(Q, axis=1), np.linalg.norm(C, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (Q @ C.T) / nq[:, None] / ncn[None, :]
    return np.where((nq[:, None] == 0) | (ncn[None, :] == 0), 0.0, out)


# the ladder of tests/test_gpu_similar.py: one table per (precision, k)
CONFIGS = [("f32", 1), ("f32", 5), ("f32", 32), ("f32", 33), ("f32", 64), ("f32", 128), ("f32", 200), ("f64", 10)]
N_TABLE = 20_100


def ladder_table(precision, k):
    rng = np.random.default_rng(3000 + k)
    return rng.standard_normal((N_TABLE, k)).astype(np.float32 if precision == "f32" else np.float64)
