"""Conditioning cases shared by test_conditioning_host.py (CPU) and test_gpu_conditioning.py (GPU): one small degree
block solved over two factor families and a ladder of lambdas, so that rows sit on both sides of the tile solve's
refinement gate (als_tile_solve.h: refine when the smallest pivot of the Jacobi-scaled system is < 0.45) and reach
condition numbers the strict per-row tests (rowshapes.py: signed factors, lambda 0.05 / 1) never see.

The block: a row of every third degree 1..130, of the degrees round the 32-entry block and the entry-space cut-offs
(2, 3, 31..33, 63..65, 95..97, 127..129), four longer rows, two to four more rows of some degrees up to 12 (the rows
that populate the low pivot buckets) and one row without a rating: 79 rows over 1024 opposite rows. The
GPU cases force a 64-entry chunk: rows above 64 entries are PARTIAL slots summed by a REDUCE task, rows up to 64 one
FULL task, short rows solved in entry space by the plan's own rule (rowshapes.task_kinds).

The families, both rounded through fp32: `signed`, the zero-mean unit-norm rows of rowshapes.factors (small pivots come
from rank deficiency only, n < k), and `offset`, sqrt(1 - t^2) * signed + t / sqrt(k) with t = 0.9 -- every row shares
a direction, as trained factors do, which puts small pivots on every row, split rows included, and is the only family
that takes the entry-space system below the gate.

The bar: per-row norm-relative error against the fp64 oracle within max(rowshapes.BOUND, 3 x the worst row of the
reference's own fp32 arithmetic in the same pivot bucket of the same case) -- the project's envelope factor applied per
bucket instead of over the whole block. REF32_WORST holds those worst rows, measured on the CPU with the oracle alone
(test_conditioning_host.py re-measures them); no figure here comes from a GPU result.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import rowshapes as rs

oracle = rs.oracle

N_OPP = 1024
CHUNK = 64
# two to four more rows of the degrees 1..12 that fall into the thinly populated pivot buckets (five one-rating rows)
_MORE_SHORT = (1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 8, 8, 9, 9, 12, 12)
_BASE_DEGS = set(range(1, 131, 3)) | {2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 200, 257, 330}
DEGS = tuple(sorted(tuple(_BASE_DEGS) + _MORE_SHORT)) + (0,)
FAMILIES = ("signed", "offset")
OFFSET_T = 0.9
LAMBDAS = (0.05, 0.01, 0.005, 0.002)
GATE = 0.45            # SolveArgs::refine_min_pivot of the product build
GATE_BAND = 0.01       # the kernel's pivots are fp32: rows within this of the gate may fall on either side
# pivot buckets [lo, hi) by a row's smallest primal pivot (the first includes 1)
BUCKET_EDGES = (1.0, 0.45, 0.3, 0.1, 0.03, 0.01)
BUCKET_NAMES = ("[0.45, 1]", "[0.3, 0.45)", "[0.1, 0.3)", "[0.03, 0.1)", "[0.01, 0.03)")
ENVELOPE = 3.0         # bound = ENVELOPE x the reference's worst fp32 row of the bucket (test_gpu_parity.py's factor)
MUTANT_MARGIN = 3.0    # every row's nearest one-entry mutant is at least this many bounds away

# The fp32 MFMA tile-solve widths, and the lambdas of every (k, family), largest first. LAMBDAS is the default; the
# others were picked on the CPU from 0.05 .. 0.002 so that every input condition of test_conditioning_host.py holds
# (each populated bucket >= 3 rows, no pivot below 0.01, <= 10 % of the rows within 0.01 of the gate, both windows
# next to the gate populated over the ladder). No (k, family) is left out; the conditions fail at, and the ladders
# therefore avoid, e.g. lambda = 0.01 on `offset` at k = 64 (more than 10 % of the rows within 0.01 of the gate) and
# lambda = 0.002 on `signed` at k = 10 and 20 (one-rating rows with a pivot below 0.01).
MFMA_KS = (32, 40, 64, 128)
LAMBDAS_OF = {
    (32, "signed"): (0.05, 0.025, 0.008, 0.0025), (32, "offset"): (0.05, 0.025, 0.008, 0.002),
    (40, "signed"): (0.04, 0.012, 0.006, 0.002), (40, "offset"): (0.05, 0.02, 0.007, 0.002),
    (64, "signed"): LAMBDAS, (64, "offset"): (0.04, 0.012, 0.005, 0.0025),
    (128, "signed"): (0.04, 0.012, 0.005, 0.003), (128, "offset"): (0.05, 0.01, 0.007, 0.0025),
    # the widths of the paths without a gate (VALU Cholesky, generic): a largest and a smallest lambda only
    (10, "signed"): (0.05, 0.004), (10, "offset"): (0.05, 0.002),
    (20, "signed"): (0.05, 0.006), (20, "offset"): (0.03, 0.002),
    (130, "signed"): (0.05, 0.002), (130, "offset"): (0.05, 0.0025),
}
# paths without a gate: (precision, k); fp64 at k = 64 takes the two ends of the k = 64 ladders
UNGATED = (("f32", 10), ("f32", 20), ("f64", 10), ("f64", 64), ("f32", 130), ("f64", 130))


def lambdas(k: int, family: str) -> tuple:
    """The lambdas of a (k, family), largest first."""
    return LAMBDAS_OF[(k, family)]


def ungated_lambdas(k: int, family: str) -> tuple:
    """Largest and smallest lambda of the (k, family)."""
    lams = LAMBDAS_OF[(k, family)]
    return (lams[0], lams[-1])


def all_cases() -> list:
    """Every (k, family, lambda) the conditioning tests solve."""
    return [(k, fam, lam) for (k, fam), lams in LAMBDAS_OF.items() for lam in lams]


@functools.lru_cache(maxsize=None)
def block() -> rs.Ladder:
    return rs.ladder_block(DEGS, n_opp=N_OPP, seed=4)


@functools.lru_cache(maxsize=None)
def table(family: str, k: int) -> np.ndarray:
    """The opposite factors of a family, exactly representable in fp32, read-only."""
    F = rs.factors(N_OPP, k)
    if family == "offset":
        F = (np.sqrt(1 - OFFSET_T ** 2) * F + OFFSET_T / np.sqrt(k)).astype(np.float32).astype(np.float64)
    else:
        assert family == "signed", family
    F.setflags(write=False)
    return F


def padded_k(k: int) -> int:
    """The stride of a factor row: 16 / 32 / 64 / 128 on the fixed-width paths, whole 16s on the generic path."""
    return 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128 if k <= 128 else -(-k // 16) * 16


def _unit_diagonal_pivots(A: np.ndarray):
    d = 1.0 / np.sqrt(np.diag(A))
    S = A * d[:, None] * d[None, :]
    return float((np.diag(np.linalg.cholesky(S)) ** 2).min()), S


def scaled_pivots(Y: np.ndarray, lam: float, k: int, dual: bool = False):
    """(smallest pivot, condition number) in fp64 of the unit-diagonal system the tile solve factors for a row with
    the gathered factor rows Y (n x k) -- the quantity its refinement gate compares with 0.45.

    Primal: D (Y^T Y + lambda n I) D padded to KP x KP with identity rows, in the kernel's feature order (feature
    f = C i + b at position 16 b + i, C = KP / 16; the natural order on the Cholesky paths' widths). Dual: the entry
    system D (Y Y^T + lambda n I) D in the physical entry order of als_plan.h (block_position), padded to whole
    32-entry blocks with identity rows. Pivots depend on the elimination order, hence the permutations; the condition
    number is that of the real rows alone."""
    Y = np.asarray(Y, np.float64)
    n = Y.shape[0]
    reg = float(np.float32(lam)) * n
    if dual:
        size = -(-n // rs.BLOCK_ENTRIES) * rs.BLOCK_ENTRIES
        e = np.arange(n)
        w = e % rs.BLOCK_ENTRIES
        pos = e - w + (w % 4) * 8 + w // 4
        A = np.eye(size)
        A[np.ix_(pos, pos)] = Y @ Y.T + reg * np.eye(n)
        real = np.sort(pos)
    else:
        kp = padded_k(k)
        A = np.eye(kp)
        A[:k, :k] = Y.T @ Y + reg * np.eye(k)
        if kp in (32, 64, 128):
            C = kp // 16
            p = np.arange(kp)
            order = C * (p % 16) + p // 16          # feature at position p
            A = A[np.ix_(order, order)]
            real = np.nonzero(order < k)[0]
        else:
            real = np.arange(k)
    piv, S = _unit_diagonal_pivots(A)
    return piv, float(np.linalg.cond(S[np.ix_(real, real)]))


def bucket_of(piv) -> np.ndarray:
    """Index into BUCKET_NAMES of each pivot; -1 below the last bucket (no case may hold such a row)."""
    piv = np.asarray(piv, np.float64)
    out = np.full(piv.shape, -1)
    for b in range(len(BUCKET_NAMES)):
        hi, lo = BUCKET_EDGES[b], BUCKET_EDGES[b + 1]
        out[(piv >= lo) & ((piv < hi) | (b == 0))] = b
    return out


Case = namedtuple("Case", "k family lam F ref64 ref32 piv dpiv cond bucket")


@functools.lru_cache(maxsize=None)
def case(k: int, family: str, lam: float) -> Case:
    """Everything a (k, family, lambda) needs, computed once and read-only: the table, the fp64 oracle, the
    reference's fp32 result, and per row the smallest primal pivot, the smallest dual pivot (rows of <= min(k, 96)
    entries, NaN elsewhere), the condition number and the pivot bucket (-1 on the empty row)."""
    lad = block()
    F = table(family, k)
    ref64, ref32 = rs.references(lad.side, F, lam)
    n = len(lad.degs)
    piv, dpiv, cond = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    for i, d in enumerate(lad.degs):
        if d == 0:
            continue
        Y = F[lad.side.col[lad.side.row_ptr[i]:lad.side.row_ptr[i + 1]]]
        piv[i], cond[i] = scaled_pivots(Y, lam, k)
        if d <= min(k, 96):
            dpiv[i] = scaled_pivots(Y, lam, k, dual=True)[0]
    bucket = np.where(lad.degs > 0, bucket_of(np.nan_to_num(piv, nan=1.0)), -1)
    for a in (ref64, ref32, piv, dpiv, cond, bucket):
        a.setflags(write=False)
    return Case(k, family, lam, F, ref64, ref32, piv, dpiv, cond, bucket)


def kinds_of(k: int, path: str = "mfma_split", dual: bool = True, chunk: int = CHUNK) -> list:
    return rs.task_kinds(block().degs, k, chunk, path, dual)


def gate_pivots(c: Case, kinds) -> np.ndarray:
    """The pivot the gate sees on each row: the dual one where the plan solves the row in entry space."""
    entry = np.array([kd == "entry-space" for kd in kinds])
    assert not np.isnan(c.dpiv[entry]).any()
    return np.where(entry, c.dpiv, c.piv)


def bucket_worst(rel, bucket) -> tuple:
    """Largest per-row error of each bucket (0 where it holds no row)."""
    return tuple(float(rel[bucket == b].max()) if (bucket == b).any() else 0.0 for b in range(len(BUCKET_NAMES)))


def round_up(x: float) -> float:
    """x rounded up in its third significant digit, as the recorded figures are."""
    if x == 0:
        return 0.0
    e = int(np.floor(np.log10(x))) - 2
    return float(f"{np.ceil(x / 10.0 ** e * (1 - 1e-12)) * 10.0 ** e:.2e}")


# The worst per-row error of the reference's own fp32 arithmetic (oracle, f32 mode) per bucket of each case, rounded up
# in the third digit; 0: no row. Measured on the CPU; test_conditioning_host.py re-measures every figure.
REF32_WORST = {
    (32, "signed", 0.05): (1.51e-06, 2.19e-06, 5.56e-06, 0, 0),
    (32, "signed", 0.025): (1.32e-06, 4.53e-06, 1.96e-05, 0, 0),
    (32, "signed", 0.008): (6.88e-07, 8.22e-07, 5.88e-05, 7.72e-05, 0),
    (32, "signed", 0.0025): (8.03e-07, 1.09e-06, 3.70e-06, 1.39e-04, 7.62e-04),
    (32, "offset", 0.05): (5.14e-06, 4.80e-06, 0, 0, 0),
    (32, "offset", 0.025): (8.48e-06, 6.59e-06, 3.11e-05, 0, 0),
    (32, "offset", 0.008): (0, 1.55e-05, 5.98e-05, 4.27e-05, 0),
    (32, "offset", 0.002): (0, 0, 2.37e-05, 1.74e-04, 1.56e-04),
    (40, "signed", 0.04): (2.21e-06, 4.55e-06, 1.16e-05, 0, 0),
    (40, "signed", 0.012): (7.22e-07, 2.35e-06, 4.24e-05, 8.99e-05, 0),
    (40, "signed", 0.006): (7.79e-07, 1.05e-06, 5.18e-05, 1.38e-04, 0),
    (40, "signed", 0.002): (7.16e-07, 1.05e-06, 3.91e-06, 2.14e-04, 4.66e-04),
    (40, "offset", 0.05): (4.89e-06, 4.45e-06, 0, 0, 0),
    (40, "offset", 0.02): (1.01e-05, 7.84e-06, 2.14e-05, 0, 0),
    (40, "offset", 0.007): (0, 1.82e-05, 9.53e-05, 1.07e-04, 0),
    (40, "offset", 0.002): (0, 0, 2.92e-05, 4.06e-04, 3.49e-04),
    (64, "signed", 0.05): (3.24e-06, 5.88e-06, 0, 0, 0),
    (64, "signed", 0.01): (1.06e-06, 3.27e-06, 8.37e-05, 8.44e-05, 0),
    (64, "signed", 0.005): (7.94e-07, 1.87e-06, 5.19e-05, 1.87e-04, 0),
    (64, "signed", 0.002): (9.70e-07, 1.42e-06, 5.07e-06, 2.17e-04, 3.01e-04),
    (64, "offset", 0.04): (7.28e-06, 6.68e-06, 0, 0, 0),
    (64, "offset", 0.012): (1.48e-05, 1.36e-05, 2.88e-05, 0, 0),
    (64, "offset", 0.005): (0, 2.21e-05, 2.43e-04, 1.54e-04, 0),
    (64, "offset", 0.0025): (0, 0, 6.67e-05, 4.90e-04, 0),
    (128, "signed", 0.04): (7.12e-06, 1.03e-05, 0, 0, 0),
    (128, "signed", 0.012): (3.44e-06, 1.17e-05, 8.87e-05, 0, 0),
    (128, "signed", 0.005): (1.59e-06, 4.89e-06, 1.63e-04, 3.74e-04, 0),
    (128, "signed", 0.003): (1.35e-06, 2.68e-06, 9.60e-05, 7.63e-04, 0),
    (128, "offset", 0.05): (7.11e-06, 0, 0, 0, 0),
    (128, "offset", 0.01): (2.05e-05, 2.59e-05, 3.63e-05, 0, 0),
    (128, "offset", 0.007): (2.27e-05, 3.51e-05, 1.44e-04, 0, 0),
    (128, "offset", 0.0025): (0, 3.14e-05, 1.85e-04, 6.68e-04, 0),
    (10, "signed", 0.05): (5.93e-07, 2.21e-06, 3.08e-06, 0, 0),
    (10, "signed", 0.004): (5.27e-07, 1.44e-06, 3.65e-06, 3.49e-05, 8.61e-05),
    (10, "offset", 0.05): (4.68e-06, 2.53e-06, 3.41e-06, 0, 0),
    (10, "offset", 0.002): (0, 0, 1.53e-05, 1.58e-05, 7.86e-05),
    (20, "signed", 0.05): (1.08e-06, 2.11e-06, 5.07e-06, 0, 0),
    (20, "signed", 0.006): (6.87e-07, 7.02e-07, 9.22e-06, 5.99e-05, 0),
    (20, "offset", 0.03): (6.53e-06, 3.81e-06, 1.66e-05, 0, 0),
    (20, "offset", 0.002): (0, 0, 1.65e-05, 6.19e-05, 1.75e-04),
    (130, "signed", 0.05): (7.38e-06, 0, 0, 0, 0),
    (130, "signed", 0.002): (1.09e-06, 2.40e-06, 6.32e-05, 1.53e-03, 0),
    (130, "offset", 0.05): (7.39e-06, 0, 0, 0, 0),
    (130, "offset", 0.0025): (0, 3.29e-05, 2.60e-04, 1.16e-03, 0),
}


def bounds(c: Case, precision: str) -> np.ndarray:
    """The per-row bound of a case: BOUND[precision], or for fp32 ENVELOPE x the reference's recorded worst row of the
    row's bucket where that is more."""
    out = np.full(len(c.bucket), rs.BOUND[precision])
    if precision == "f32":
        worst = np.asarray(REF32_WORST[(c.k, c.family, c.lam)] + (0.0,))      # bucket -1 (empty row): BOUND
        out = np.maximum(out, ENVELOPE * worst[c.bucket])
    return out


def rejected_rows(got, c: Case, precision: str) -> np.ndarray:
    """Per row: True where check_case would reject it on its bound (rows without a rating: on any nonzero)."""
    degs = block().degs
    bad = ~(rs.row_errors(got, c.ref64) <= bounds(c, precision))
    zero = degs == 0
    bad[zero] = np.any(np.asarray(got)[zero] != 0, axis=1)
    return bad


def check_case(got, c: Case, precision: str, kinds=None) -> np.ndarray:
    """Every row of `got` against the fp64 oracle of the case: within its bound (bounds), the row without a rating
    exactly zero, and for fp32 the median over the rated rows <= max(2 x the reference's fp32 median, 2e-5). Returns
    the per-row errors; raises AssertionError naming each failing row (the 12 worst), its degree, task kind, bucket,
    pivot and error."""
    degs = block().degs
    assert len(degs) == len(got) == len(c.ref64)
    rel = rs.row_errors(got, c.ref64)
    bnd = bounds(c, precision)
    bad = rejected_rows(got, c, precision)
    if bad.any():
        rows = np.nonzero(bad)[0]
        worst = rows[np.argsort(-np.nan_to_num(rel[rows], posinf=1e300))][:12]
        lines = [f"row {i} deg {degs[i]} {kinds[i] if kinds is not None else ''} bucket "
                 f"{BUCKET_NAMES[c.bucket[i]] if c.bucket[i] >= 0 else 'empty'} pivot {c.piv[i]:.3f}: "
                 f"err {rel[i]:.3e} > {bnd[i]:.3e}" for i in worst]
        raise AssertionError(f"{len(rows)} of {len(degs)} rows beyond their bound (k={c.k} {c.family} lam={c.lam:g} "
                             f"{precision}): " + "; ".join(lines))
    if precision == "f32":
        rated = degs > 0
        med, med_ref = np.median(rel[rated]), np.median(rs.row_errors(c.ref32, c.ref64)[rated])
        assert med <= max(2 * med_ref, 2e-5), f"median {med:.3e} vs the reference's fp32 median {med_ref:.3e}"
    return rel
