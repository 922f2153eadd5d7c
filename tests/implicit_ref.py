"""Implicit-feedback ALS (Hu, Koren, Volinsky 2008) restated in numpy: the oracle of test_gpu_implicit.py, measured by
test_implicit_host.py.

    G = Y^T Y,   A = G + alpha sum_e r_e y_e y_e^T + lambda I,   b = sum_{e: r_e > 0} (1 + alpha r_e) y_e,   x = A^-1 b

solve_rows in float64 is the oracle. In float32 it is the restatement's own fp32 arithmetic: G summed in fp32 in
256-row pieces, the weighted Gram and right-hand side fp32 products, np.linalg.cholesky on the Jacobi-scaled fp32 system
and fp32 substitutions -- the yardstick for "how far does a correct fp32 implementation land from the oracle". The
`mutant` argument builds the wrong models a kernel could compute instead (lambda n for lambda, b without the 1 +, G left
out); rowshapes.mutants supplies the one-entry mutants. solve_rows_dense is the textbook formulation (an explicit
confidence and preference per item, np.linalg.solve) used only to prove the G trick on tiny shapes.

The recorded figures at the end were measured on the CPU with this file alone; test_implicit_host.py re-measures them.
No figure here comes from a GPU result.
"""
from __future__ import annotations

import functools

import numpy as np

import conditioning as cond
import rowshapes as rs

GRAM_PIECE = 256
MUTANTS = ("lambda_n", "no_one", "no_G")

# (k, alpha, lambda) of the ladder cases (rowshapes.ladder_block over rowshapes.factors(4096, k)). The fp32 cases were
# picked on the CPU so that every row's nearest mutant stays LADDER_MARGIN bounds away: at alpha = 40 and k >= 64 the
# model all but interpolates its observed entries and single entries of the rows of 200..1023 entries stop mattering
# (nearest one-entry mutant 3e-6 at (128, 40, 0.05), 1e-4 at (64, 40, 0.05)), and against G ~ 4096 / k a lambda of 0.05
# is too small for the lambda n mutant to show on the two-entry row (8e-5 at (10, 40, 0.05), 2.8e-4 at (32, 10, 0.05)).
# Hence the smaller alphas at k >= 64 and the larger lambdas. fp64 keeps (40, 0.05): its bound of 1e-8 is 300 x below
# the nearest of those mutants.
LADDER_F32 = ((10, 40.0, 0.5), (32, 10.0, 0.2), (64, 10.0, 0.1), (128, 1.0, 0.1), (128, 4.0, 0.1))
LADDER_F64 = ((10, 40.0, 0.05), (64, 40.0, 0.05), (128, 40.0, 0.05))
LADDER_MARGIN = 5.0        # the restatement's fp32 worst row and every row's nearest mutant keep this from rs.BOUND
# (k, alpha, lambda) of the conditioning cases (conditioning.block over conditioning.table("offset", k)); every one runs
# in fp64, in fp32 those whose nearest mutant is >= cond.MUTANT_MARGIN bars away (COND_F32)
COND_CASES = ((64, 1.0, 0.002), (128, 1.0, 0.01), (32, 10.0, 0.01), (64, 40.0, 0.05))
# training: users x movies, density, features, alpha, lambda, halves (four iterations)
TRAIN = dict(n_users=96, n_movies=48, density=0.15, k=10, alpha=40.0, lam=0.05, seed=42, halves=8)


def _csr(side):
    """(row_ptr, col, ratings) of an oracle.Side, a block dict or a tuple."""
    if isinstance(side, dict):
        return side["row_ptr"], side["col"], side["ratings"]
    if isinstance(side, tuple):
        return side
    return side.row_ptr, side.col, side.ratings


def gram(Y, dtype=np.float64):
    """Y^T Y in `dtype`: float64 directly, float32 summed in fp32 in GRAM_PIECE-row pieces."""
    Y = np.asarray(Y, dtype)
    if dtype == np.float64:
        return Y.T @ Y
    G = np.zeros((Y.shape[1], Y.shape[1]), np.float32)
    for lo in range(0, len(Y), GRAM_PIECE):
        G = G + Y[lo:lo + GRAM_PIECE].T @ Y[lo:lo + GRAM_PIECE]
    return G


def _solve_spd(A, b, dtype):
    """x of A x = b for one symmetric positive definite system in `dtype`: Jacobi scaling, Cholesky, substitutions."""
    if dtype == np.float64:
        return np.linalg.solve(A, b)
    s = (1.0 / np.sqrt(np.diag(A))).astype(dtype)
    L = np.linalg.cholesky((A * s[:, None] * s[None, :]).astype(dtype))
    y = np.zeros_like(b)
    rhs = (b * s).astype(dtype)
    k = len(b)
    for j in range(k):                       # forward, in the working precision
        y[j] = (rhs[j] - np.dot(L[j, :j], y[:j])) / L[j, j]
    x = np.zeros_like(b)
    for j in range(k - 1, -1, -1):           # backward
        x[j] = (y[j] - np.dot(L[j + 1:, j], x[j + 1:])) / L[j, j]
    return (x * s).astype(dtype)


def solve_rows(side, Y, lam, alpha, dtype=np.float64, mutant=None):
    """The implicit-feedback solution of every row of `side` against the opposite table Y, in `dtype` arithmetic.
    lam and alpha are rounded through float32 as the C ABI takes them. mutant: None or one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    row_ptr, col, rat = _csr(side)
    Y = np.asarray(Y, dtype)
    k = Y.shape[1]
    lam, alpha = dtype(np.float32(lam)), dtype(np.float32(alpha))
    G = np.zeros((k, k), dtype) if mutant == "no_G" else gram(Y, dtype)
    out = np.zeros((len(row_ptr) - 1, k), dtype)
    for i in range(len(row_ptr) - 1):
        lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
        if hi == lo:
            continue
        Ys = Y[np.asarray(col[lo:hi])]
        r = np.asarray(rat[lo:hi]).astype(dtype)
        w = alpha * r
        reg = lam * dtype(hi - lo) if mutant == "lambda_n" else lam
        A = G + (Ys * w[:, None]).T @ Ys + reg * np.eye(k, dtype=dtype)
        c = np.where(r > 0, (w if mutant == "no_one" else dtype(1) + w), dtype(0)).astype(dtype)
        out[i] = _solve_spd(A.astype(dtype), (c @ Ys).astype(dtype), dtype)
    return out


def solve_rows_dense(side, Y, lam, alpha):
    """The same solutions from the dense formulation in float64: per row a confidence c_i = 1 + alpha (the ratings the
    row gives item i, summed) for EVERY item of the table and the confidence-weighted preference, A = Y^T diag(c) Y +
    lambda I, b = Y^T (c p). An item a row lists twice is two observations: its (1 + alpha r) terms add in c p."""
    row_ptr, col, rat = _csr(side)
    Y = np.asarray(Y, np.float64)
    lam, alpha = float(np.float32(lam)), float(np.float32(alpha))
    out = np.zeros((len(row_ptr) - 1, Y.shape[1]))
    for i in range(len(row_ptr) - 1):
        lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
        if hi == lo:
            continue
        c, cp = np.ones(len(Y)), np.zeros(len(Y))
        for e in range(lo, hi):
            c[col[e]] += alpha * float(rat[e])
            if rat[e] > 0:
                cp[col[e]] += 1.0 + alpha * float(rat[e])
        out[i] = np.linalg.solve(Y.T @ (c[:, None] * Y) + lam * np.eye(Y.shape[1]), Y.T @ cp)
    return out


def loss(U, M, R, lam, alpha) -> float:
    """sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + lambda (|U|^2 + |M|^2) over the dense grid R (users x movies, 0 =
    unobserved), in float64."""
    U, M, R = np.asarray(U, np.float64), np.asarray(M, np.float64), np.asarray(R, np.float64)
    err = (R > 0) - U @ M.T
    return float(np.sum((1.0 + float(np.float32(alpha)) * R) * err * err)
                 + float(np.float32(lam)) * (np.sum(U * U) + np.sum(M * M)))


def dense_to_csr(R):
    """(row_ptr, col, ratings) of the nonzeros of a dense grid, columns ascending."""
    R = np.asarray(R)
    rows, cols = np.nonzero(R)
    row_ptr = np.zeros(R.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=R.shape[0]), out=row_ptr[1:])
    return row_ptr, cols.astype(np.int32), R[rows, cols].astype(np.int16)


def train(R, U0, lam, alpha, halves, dtype=np.float64):
    """Implicit ALS from U0 over the dense grid R: movie half, user half, ... `halves` of them. Returns the list of
    (U, M) after each half, in `dtype` arithmetic."""
    user_csr, movie_csr = dense_to_csr(R), dense_to_csr(np.asarray(R).T)
    U, M = np.asarray(U0, dtype), np.zeros((np.asarray(R).shape[1], np.asarray(U0).shape[1]), dtype)
    out = []
    for h in range(halves):
        if h % 2 == 0:
            M = solve_rows(movie_csr, U, lam, alpha, dtype)
        else:
            U = solve_rows(user_csr, M, lam, alpha, dtype)
        out.append((U.copy(), M.copy()))
    return out


def nearest_mutant(side, Y, lam, alpha, ref64):
    """Per row the smallest norm-relative distance from the oracle to any mutant that changes the row: the one-entry
    mutants of rowshapes.mutants (rows of >= 2 entries), lambda n (n != 1), b without the 1 +, G left out. inf on rows
    without a rating."""
    row_ptr, _, _ = _csr(side)
    degs = np.diff(row_ptr)
    near = np.full(len(degs), np.inf)
    for name, mut in rs.mutants(side).items():
        d = rs.row_errors(solve_rows(mut, Y, lam, alpha), ref64)
        near = np.where(degs >= 2, np.minimum(near, d), near)
    for name in MUTANTS:
        d = rs.row_errors(solve_rows(side, Y, lam, alpha, mutant=name), ref64)
        changes = (degs > 1) if name == "lambda_n" else (degs > 0)
        near = np.where(changes, np.minimum(near, d), near)
    return near


@functools.lru_cache(maxsize=None)
def ladder_case(k, alpha, lam):
    """(ladder, table, fp64 oracle) of a ladder case: computed once, read-only."""
    lad = rs.ladder_block()
    F = rs.factors(lad.n_opp, k)
    ref64 = solve_rows(lad.side, F, lam, alpha)
    for a in (F, ref64):
        a.setflags(write=False)
    return lad, F, ref64


@functools.lru_cache(maxsize=None)
def cond_case(k, alpha, lam):
    """(block, table, fp64 oracle) of a conditioning case: computed once, read-only."""
    lad = cond.block()
    F = cond.table("offset", k)
    ref64 = solve_rows(lad.side, F, lam, alpha)
    ref64.setflags(write=False)
    return lad, F, ref64


def cond_bar(case) -> float:
    """The fp32 bar of a conditioning case: max(BOUND, ENVELOPE x the restatement's recorded worst fp32 row)."""
    return max(rs.BOUND["f32"], cond.ENVELOPE * COND_REF32_WORST[case])


@functools.lru_cache(maxsize=None)
def train_inputs():
    """(R dense int16 grid, ratings as (movie ids, user ids, ratings) with 1-based ids) of the training case."""
    t = TRAIN
    rng = np.random.default_rng(t["seed"])
    R = np.where(rng.random((t["n_users"], t["n_movies"])) < t["density"],
                 rng.integers(1, 6, (t["n_users"], t["n_movies"])), 0).astype(np.int16)
    R[np.arange(t["n_users"]), np.arange(t["n_users"]) % t["n_movies"]] = 3     # no user and no movie without a rating
    u, m = np.nonzero(R)
    R.setflags(write=False)
    return R, (m.astype(np.int32) + 1, u.astype(np.int32) + 1, R[u, m].astype(np.int16))


# ---- recorded on the CPU (test_implicit_host.py re-measures every figure) -------------------------------------------
# worst row of the fp32 restatement per conditioning case, rounded up in the third digit (conditioning.round_up)
COND_REF32_WORST = {
    (64, 1.0, 0.002): 1.15e-05,
    (128, 1.0, 0.01): 1.53e-05,
    (32, 10.0, 0.01): 2.13e-05,
    (64, 40.0, 0.05): 4.89e-05,
}
# the conditioning cases whose every row keeps its nearest mutant >= cond.MUTANT_MARGIN bars away: the fp32 cases
COND_F32 = COND_CASES      # nearest mutants 6.3e-4, 6.0e-3, 8.7e-4, 8.3e-4 against bars of 1e-4, 1e-4, 1e-4, 1.47e-4
# per-row drift of the fp32 restatement from the fp64 one after the fourth iteration (largest over U and M), rounded up
TRAIN_REF32_DRIFT = 9.03e-05
