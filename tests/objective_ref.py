"""The implicit-feedback objective (als_implicit_objective) restated in numpy: the oracle of test_gpu_objective.py,
measured by test_objective_host.py.

For a row x with entries e (opposite rows y_e, ratings r_e >= 0) and G = Y^T Y of the whole opposite table:

    f(x) = x^T G x  +  sum_e [ (1 + alpha r_e)(p_e - s_e)^2 - s_e^2 ]  +  lambda x^T x,     s_e = y_e . x,  p_e = [r_e > 0]

parts() evaluates the three terms per query from float64 inputs with every product and sum in extended precision
(np.longdouble: 64 mantissa bits where it is the x87 type, which test_objective_host.py asserts), and with them the
absolute sums the error bounds are made of. With u = 2^-53:

    quad     (2k + 2) u |x|^T |G| |x|                       the classical bound of the k-term dots, any order
    ridge    (k + 2) u lambda x^T x
    observed (2k + n + 8) u sum_e [(1 + alpha r_e)(p_e + a_e)^2 + a_e^2],  a_e = sum_f |x_f| |y_ef|
                                                            s_e's error carried through the term, plus the sum over n

The bounds are derived, not measured; no figure here comes from a GPU result. `mutant` builds the wrong models a kernel
could compute instead (MUTANTS); closed_form() is c - b^T x, the value of f at the minimiser of als_solve_implicit.
"""
from __future__ import annotations

import numpy as np

import implicit_ref as ir
import rowshapes as rs

U = 2.0 ** -53
LD = np.longdouble
MUTANTS = ("drop_first", "drop_middle", "drop_last", "rating_plus_1", "no_minus_s2", "p_one_for_zero", "alpha_r", "no_G",
           "lambda_n", "G_diagonal")
MUTANT_MARGIN = 100.0       # every mutant moves every row it changes by at least this many bounds of the row
PERTURB = 1e-2              # relative size of the perturbations around the minimiser
# the (k, alpha, lambda) of implicit_ref's ladder whose every row keeps every mutant MUTANT_MARGIN bounds away, at the
# solved rows and at random rows (test_objective_host.py re-measures it): all of them
LADDER_F32 = ir.LADDER_F32
LADDER_F64 = ir.LADDER_F64


def _csr(q):
    ptr, idx, rat = ir._csr(q)
    return np.asarray(ptr, np.int64), np.asarray(idx), np.asarray(rat)


def parts(queries, X, Y, G, lam, alpha, mutant=None):
    """(parts [n, 3], bounds [n, 3]) of the queries (ptr, idx, ratings) at the rows X [n, k] against the table Y and its
    Gram G [k, k] (the caller's: the device's own G on the GPU, Y^T Y here). lam and alpha are rounded through float32 as
    the C ABI takes them. parts = {x^T G x, sum_e [...], lam x^T x} as float64 roundings of the extended sums."""
    assert mutant is None or mutant in MUTANTS
    ptr, idx, rat = _csr(queries)
    X, Y, G = np.asarray(X, np.float64), np.asarray(Y, np.float64), np.asarray(G, np.float64)
    n, k = X.shape
    lam, alpha = LD(np.float32(lam)), LD(np.float32(alpha))
    Gl, aG = G.astype(LD), np.abs(G).astype(LD)
    if mutant == "no_G":
        Gl = np.zeros_like(Gl)
    elif mutant == "G_diagonal":
        Gl = np.diag(np.diag(Gl))
    Yl = Y.astype(LD)
    out, bound = np.zeros((n, 3), LD), np.zeros((n, 3), LD)
    for q in range(n):
        x = X[q].astype(LD)
        ax = np.abs(x)
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        cols, r = idx[lo:hi], rat[lo:hi].astype(LD)
        if mutant in ("drop_first", "drop_middle", "drop_last") and hi > lo:
            d = hi - lo
            keep = np.ones(d, bool)
            keep[{"drop_first": 0, "drop_middle": d // 2, "drop_last": d - 1}[mutant]] = False
            cols, r = cols[keep], r[keep]
        if mutant == "rating_plus_1" and hi > lo:
            r = r.copy()
            r[-1] += 1
        nq = len(cols)
        out[q, 0] = x @ Gl @ x
        bound[q, 0] = (2 * k + 2) * U * (ax @ aG @ ax)
        reg = lam * (hi - lo) if mutant == "lambda_n" else lam
        out[q, 2] = reg * (x @ x)
        bound[q, 2] = (k + 2) * U * lam * (x @ x)
        if nq:
            Ys = Yl[cols]
            s, a = Ys @ x, np.abs(Ys) @ ax
            p = (r > 0).astype(LD)
            if mutant == "p_one_for_zero":
                p = np.ones_like(p)
            c = alpha * r if mutant == "alpha_r" else 1 + alpha * r
            t = c * (p - s) ** 2
            if mutant != "no_minus_s2":
                t = t - s * s
            out[q, 1] = t.sum()
            bound[q, 1] = (2 * k + nq + 8) * U * ((1 + alpha * r) * (p + a) ** 2 + a * a).sum()
    return out.astype(np.float64), bound.astype(np.float64)


def closed_form(queries, X, Y, alpha):
    """c_q - b^T x per query: c = sum_{r > 0} (1 + alpha r), b = sum_{r > 0} (1 + alpha r) y -- f at the minimiser."""
    ptr, idx, rat = _csr(queries)
    alpha = LD(np.float32(alpha))
    Yl = np.asarray(Y, np.float64).astype(LD)
    out = np.zeros(len(ptr) - 1, LD)
    for q in range(len(ptr) - 1):
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        r = rat[lo:hi].astype(LD)
        c = np.where(r > 0, 1 + alpha * r, LD(0))
        out[q] = c.sum() - (c @ Yl[idx[lo:hi]]) @ np.asarray(X[q], np.float64).astype(LD)
    return out.astype(np.float64)


def system(queries, q, Y, G, lam, alpha):
    """(A, b) of query q in float64: A = G + alpha sum r y y^T + lam I, b = sum_{r > 0} (1 + alpha r) y."""
    ptr, idx, rat = _csr(queries)
    lam, alpha = float(np.float32(lam)), float(np.float32(alpha))
    lo, hi = int(ptr[q]), int(ptr[q + 1])
    Ys, r = np.asarray(Y, np.float64)[idx[lo:hi]], rat[lo:hi].astype(np.float64)
    A = np.asarray(G, np.float64) + (Ys * (alpha * r)[:, None]).T @ Ys + lam * np.eye(Ys.shape[1])
    return A, np.where(r > 0, 1 + alpha * r, 0.0) @ Ys


def random_rows(n, k, seed=3):
    """The second x set: random rows of the scale of trained factors, exactly representable in fp32."""
    rng = np.random.default_rng([seed, k])
    return (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32).astype(np.float64)


def perturbations(X, seed=5):
    """Seeded perturbations of relative size PERTURB, one per row (fp32-exact sums are the caller's concern)."""
    rng = np.random.default_rng([seed, X.shape[1]])
    D = rng.standard_normal(X.shape)
    D *= PERTURB * np.linalg.norm(X, axis=1, keepdims=True) / np.linalg.norm(D, axis=1, keepdims=True)
    return D


def with_zero_ratings(lad, seed=12):
    """The ladder's queries with every third rating set to 0 (at least one per row of >= 2 entries): the inputs of the
    p_one_for_zero mutant and of the special-entries test."""
    ptr, idx, rat = _csr((lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"]))
    rat = rat.copy()
    for q in range(len(ptr) - 1):
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        if hi - lo >= 2:
            rat[lo + 1:hi:3] = 0
    return ptr, idx.astype(np.int32), rat.astype(np.int16)


def mutant_margins(queries, X, Y, G, lam, alpha):
    """{mutant: (rows it changes, the smallest |f_mutant - f| / (sum of the row's three bounds) over them)}."""
    base, bound = parts(queries, X, Y, G, lam, alpha)
    f, b = base.sum(axis=1), bound.sum(axis=1)
    out = {}
    for m in MUTANTS:
        moved = np.abs(parts(queries, X, Y, G, lam, alpha, mutant=m)[0].sum(axis=1) - f)
        changed = moved > 0
        out[m] = (int(changed.sum()), float((moved[changed] / b[changed]).min()) if changed.any() else np.inf)
    return out


FIT_ITERATIONS, FIT_STOP = 4, 2     # the relative drops of iterations 1 and 2 are 0.97 and 0.20: the widest gap


def train_losses(U0, iterations=FIT_ITERATIONS):
    """The fp64 restatement's training run on implicit_ref.TRAIN from the user factors U0: [loss before training (the
    movie factors zero), after iteration 1, ...]."""
    t = ir.TRAIN
    R, _ = ir.train_inputs()
    steps = ir.train(R, U0, t["lam"], t["alpha"], 2 * iterations)
    out = [ir.loss(U0, np.zeros((t["n_movies"], t["k"])), R, t["lam"], t["alpha"])]
    out += [ir.loss(*steps[2 * i + 1], R, t["lam"], t["alpha"]) for i in range(iterations)]
    return out


def fit_stop(losses, stop):
    """rel_tol that stops implicit_fit after iteration `stop` of a run with these losses: the geometric mean of the
    relative drops of iterations stop - 1 and stop. Asserts that every earlier drop is above it and that one below."""
    drops = [(losses[i - 1] - losses[i]) / losses[i - 1] for i in range(1, len(losses))]
    tol = float(np.sqrt(drops[stop - 2] * drops[stop - 1]))
    assert all(d > tol for d in drops[:stop - 1]) and drops[stop - 1] < tol, (drops, tol)
    return tol
