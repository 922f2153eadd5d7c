"""The cases of test_gpu_cache_policy.py and of its golden's recorder, tools/record_cache_policy_golden.py.

One movie block on the degree ladder DEGS (80 rows of 1 .. 513 entries and one without a rating, over 700 user rows,
about 13k ratings; rowshapes.ladder_block) and its transpose as the user block. A case solves one movie half from a
seeded user table and then one user half from the movie rows just solved, under ALS_CHUNK=64 (128 at k = 128), so the
movie half has entry-space rows (up to 32 entries at k = 64, 96 at k = 128), FULL rows (up to the chunk) and rows of
2..9 PARTIAL slots with a REDUCE task; the user rows (9..28 entries) are entry-space rows at k = 64 and 128 and FULL
rows at k = 32.
"""
from __future__ import annotations

import functools
import hashlib
from collections import namedtuple

import numpy as np

import rowshapes as rs

DEGS = (1, 2, 3, 4, 5, 8, 15, 16, 17, 24, 31, 32, 33, 34, 40, 47, 48, 49, 56, 63, 64, 65, 66, 72, 80, 95, 96, 97, 100, 112,
        127, 128, 129, 130, 144, 159, 160, 161, 176, 191, 192, 193, 208, 224, 240, 255, 256, 257, 258, 272, 288, 300, 319,
        320, 321, 352, 383, 384, 385, 416, 447, 448, 449, 480, 511, 512, 513, 0, 12, 6, 20, 28, 36, 44, 52, 60, 61, 62, 35,
        50)
N_USERS = 700
CHUNK = {"ALS_CHUNK": "64"}
LAM = 0.05
LAM_REFINE = 0.005      # FULL rows of 33..64 entries at k = 64 then fall under the refinement gate (0.45): RowResidual runs
U_SAMPLE = 8            # the golden keeps every U_SAMPLE-th user row beside the whole table's digest

# name; features; knobs; lambda; user table ("unit": rowshapes.factors, "row_norms": row norms over 2^-24 .. 1, the
# table of test_gpu_integrity.test_presplit_range_guard); halves as two chunks each; the golden entry it must equal
Case = namedtuple("Case", "name k env lam table two_chunks golden")
CASES = (
    Case("k32", 32, CHUNK, LAM, "unit", False, "k32"),
    Case("k64", 64, CHUNK, LAM, "unit", False, "k64"),
    # a 128-entry chunk at k = 128: rows of up to 96 entries are solved in entry space, so FULL rows need 97..128
    Case("k128", 128, {"ALS_CHUNK": "128"}, LAM, "unit", False, "k128"),
    Case("k64_on_the_fly", 64, {**CHUNK, "ALS_PRESPLIT": "0"}, LAM, "unit", False, "k64_on_the_fly"),
    Case("k64_range_guard", 64, CHUNK, LAM, "row_norms", False, "k64_range_guard"),
    # als_solve_half_chunk over two row ranges is bitwise als_solve_half (test_gpu_rowshapes.py): the k64 entry
    Case("k64_two_chunks", 64, CHUNK, LAM, "unit", True, "k64"),
    Case("k64_refine", 64, CHUNK, LAM_REFINE, "unit", False, "k64_refine"),
)
RECORDED = tuple(c for c in CASES if c.golden == c.name)


@functools.lru_cache(maxsize=None)
def blocks():
    """(the movie block as a rowshapes.Ladder, the user block -- its transpose -- as (CSR dict, oracle.Side, degrees))."""
    lad = rs.ladder_block(DEGS, n_opp=N_USERS, seed=11)
    rp, col, rat = lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"]
    movie_of = np.repeat(np.arange(len(DEGS), dtype=np.int32), np.diff(rp))
    order = np.lexsort((movie_of, col))            # by user, movies ascending inside a user
    udegs = np.bincount(col, minlength=N_USERS).astype(np.int64)
    urp = np.zeros(N_USERS + 1, np.int64)
    np.cumsum(udegs, out=urp[1:])
    ucol, urat = movie_of[order].copy(), rat[order].copy()
    blk = {"row_ptr": urp, "col": ucol, "ratings": urat, "n_rows": N_USERS}
    side = rs.oracle.Side(np.arange(1, N_USERS + 1, dtype=np.int64), urp.copy(), ucol.copy(), urat.copy())
    return lad, (blk, side, udegs)


@functools.lru_cache(maxsize=None)
def user_table(kind: str, k: int) -> np.ndarray:
    """The seeded user factors a case starts from (fp32 values)."""
    if kind == "unit":
        F = rs.factors(N_USERS, k).astype(np.float32)
    else:
        rng = np.random.default_rng(k + 1)
        F = rng.random((N_USERS, k)) * 2.0 ** -rng.uniform(0, 24, size=(N_USERS, 1))
        F[0] *= 1.0 / F[0].max()
        F[1] *= 2.0 ** -24 / F[1].max()
        F = F.astype(np.float32)
    F.setflags(write=False)
    return F


def run_case(cfk, case: Case, env=None):
    """One movie half and one user half of `case` on a fresh engine (env: knobs instead of the case's own); returns
    (M, U, facts) with the factor tables read back and facts = the plan of both blocks and the integrity record."""
    lad, (ublk, _, _) = blocks()
    n_movies = len(DEGS)
    with rs.knobs(dict(case.env if env is None else env)):
        eng = cfk.ALSEngine(case.k, "f32")
    try:
        eng.use_torch_stream()
        eng.alloc_factors(0, n_movies)
        eng.alloc_factors(1, N_USERS)
        eng.set_block(0, lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"], 0, N_USERS)
        eng.set_block(1, ublk["row_ptr"], ublk["col"], ublk["ratings"], 0, n_movies)
        eng.write_factors(1, user_table(case.table, case.k))
        for side, n in ((0, n_movies), (1, N_USERS)):
            if case.two_chunks:
                bounds = [0, n // 2, n]
                eng.set_chunks(side, bounds)
                for c in range(len(bounds) - 1):
                    eng.solve_half_chunk(side, case.lam, c)
            else:
                eng.solve_half(side, case.lam)
        M, U = eng.read_factors(0, 0, n_movies), eng.read_factors(1, 0, N_USERS)
        facts = {"path": [eng.block_path(s) for s in (0, 1)], "stats": [eng.block_stats(s) for s in (0, 1)],
                 "integrity": eng.integrity_status()}
        return M, U, facts
    finally:
        eng.close()


def digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def golden_entry(M: np.ndarray, U: np.ndarray) -> dict:
    """What the golden holds of a case: the movie table, the user table's digest and every U_SAMPLE-th user row."""
    return {"M": M, "U_sha256": np.array(digest(U)), "U_rows": U[::U_SAMPLE].copy()}
