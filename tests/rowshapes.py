"""Degree-ladder blocks, their mutants and the per-row comparator shared by test_rowshapes_host.py (CPU) and
test_gpu_rowshapes.py (GPU).

The ladder is one purpose-built in-block: a row of every degree 1..330 (the 4-entry step, the 32-entry block, the
entry-space cut-offs at 32 / 64 / 96 entries and n <= k, and d = chunk, chunk +- 1, m chunk +- 1 under a forced
64- or 128-entry chunk), twelve rows around 1024, 1056, 2048, 3072 and 4000 entries (split under the unforced
1024-entry chunk too), and two rows without a rating. The opposite factors are signed with unit-norm rows
(standard normal / sqrt(k), rounded through fp32): on these the reference's own fp32 error stays near 1e-5 on every
row, while losing, adding or changing a single entry of a row moves its fp64 solution by ~1e-3 or more. A per-row
bound of 1e-4 therefore separates a correct kernel from one that drops the last entry of a chunk, miscounts a padded
block or sums one partial slot too few -- which the global envelope over uniform [0, 1) factors does not
(test_rowshapes_host.py keeps that contrast on record).
"""
from __future__ import annotations

import contextlib
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle  # noqa: E402  (checker only)

BLOCK_ENTRIES = 32      # als_plan.h: every row is padded to whole blocks of 32 entries
N_OPP = 4096
LONG_DEGS = (1023, 1024, 1025, 1055, 1056, 1057, 2047, 2048, 2049, 3071, 3073, 4000)
# rows 0..329: degree row + 1; one empty row; the twelve long rows; one empty row
DEFAULT_DEGS = tuple(range(1, 331)) + (0,) + LONG_DEGS + (0,)

# The any-k ladder (test_gpu_anyk.py): degrees either side of the generic path's batches of 8, 10, 15, 16, 55 and 64
# staged rows and of the 32-entry block, an empty row inside and one at the end, 512 opposite rows; for k >= 1010 one
# more row of 1100 > k entries over a 1280-row table.
ANYK_DEGS = (1, 2, 3, 9, 10, 11, 15, 16, 31, 32, 0, 33, 55, 56, 64, 65, 97, 130, 257, 330, 0)
ANYK_WIDE_DEG = 1100
# (precision, k, kp, Gram in LDS, batch): the launch geometry generic_plan gives each case
ANYK_CASES = (("f32", 129, 144, True, 64), ("f32", 257, 272, True, 10), ("f32", 273, 288, False, 56),
              ("f32", 500, 512, False, 32), ("f32", 1010, 1024, False, 16), ("f32", 1024, 1024, False, 16),
              ("f64", 65, 80, True, 64), ("f64", 130, 144, True, 55), ("f64", 161, 176, True, 15),
              ("f64", 177, 192, False, 42), ("f64", 1024, 1024, False, 8))


# Grid-stride cases: (precision, k, rows) of degrees 1..40 cycling -- more rows than the 1024 slabs of the slab variant
# (a slab is zeroed and used again), more than the 4096 workgroups an LDS-variant launch is capped at.
ANYK_STRIDE_CASES = (("f32", 273, 1100), ("f64", 177, 1100), ("f32", 129, 4200))
ANYK_LAM = 0.05


@functools.lru_cache(maxsize=None)
def anyk_ladder(k: int, rows: int = 0) -> Ladder:
    """The any-k ladder of a case with k features; rows > 0: the grid-stride block of that many rows."""
    if rows:
        return ladder_block(tuple(1 + i % 40 for i in range(rows)), n_opp=512, seed=3)
    if k >= 1010:
        return ladder_block(ANYK_DEGS + (ANYK_WIDE_DEG,), n_opp=1280, seed=2)
    return ladder_block(ANYK_DEGS, n_opp=512, seed=2)


@functools.lru_cache(maxsize=None)
def anyk_inputs(k: int, rows: int = 0):
    """(ladder, factors, fp64 oracle, the reference's fp32 result) of an any-k case: computed once per k (the fp32 and
    fp64 engines of one k share them), read-only."""
    lad = anyk_ladder(k, rows)
    F = factors(lad.n_opp, k)
    ref64, ref32 = references(lad.side, F, ANYK_LAM)
    for a in (F, ref64, ref32):
        a.setflags(write=False)
    return lad, F, ref64, ref32


BOUND = {"f32": 1e-4, "f64": 1e-8}    # per-row norm-relative error against the fp64 oracle
MARGIN = 5.0                          # every row's nearest mutant is at least MARGIN * BOUND away
# Where the reference's own fp32 arithmetic (oracle, f32 mode) does not stay within BOUND / MARGIN on every row, the
# fp32 bound of that case is MARGIN x the reference's worst row, measured on the CPU and recorded here (rounded up):
# the one-rating row of the any-k ladder at k = 1010 and k = 1024 (2.167e-05 and 2.056e-05 against 2e-05). The bound
# comes from the reference alone, never from a GPU result; test_rowshapes_host.py re-measures the figure, and proves
# the mutant margin, MARGIN x the bound, for it.
ANYK_REF32_WORST = {1010: 2.17e-5, 1024: 2.06e-5}


def anyk_bound(precision: str, k: int) -> float:
    """Per-row bound of an any-k case: BOUND, or MARGIN x the reference's recorded worst fp32 row where that is more."""
    if precision == "f32" and k in ANYK_REF32_WORST:
        return max(BOUND["f32"], MARGIN * ANYK_REF32_WORST[k])
    return BOUND[precision]


# The width ladder (test_gpu_foldin_edges.py), built for als_fold_in's batching: the last batch's tail is zero-filled up
# to a whole 4-entry MFMA step (1..5), the 64-entry batch boundary from both sides (63..66, 127..130), a fourth and a
# fifth batch (200, 257), the 16- and 32-entry neighbours, one empty query at the end; 512 opposite rows. WIDTH_KS: the
# widths next to every factor stride (16 / 32 / 64 / 128) that the fold-in cases solve on it, at WIDTH_LAM.
WIDTH_DEGS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 200, 257, 0)
WIDTH_KS = {"f32": (1, 2, 3, 5, 15, 16, 17, 31, 33, 48, 63, 65, 96, 127), "f64": (1, 15, 16, 17, 33, 63, 65, 127)}
# fp64 only: an fp64 engine of 65..112 features has the generic path's stride, the next multiple of 16 (65 above: 80);
# these fill each of the strides 80, 96 and 112 and stop one feature into 96 and 112
WIDTH_KS_F64_STRIDES = (80, 81, 96, 97, 112)
WIDTH_LAM = 0.05
# Repeated indices and the whole int16 rating range on that ladder: the widths, and the ratings drawn for the second
REPEAT_KS = {"f32": (10, 16, 64, 128), "f64": (64,)}
EXTREME_RATINGS = (-32768, -1, 0, 257, 32767)
FOLDIN_BATCH = 64       # als_plan.h FOLDIN_MAX_BATCH: opposite rows staged per pass


@functools.lru_cache(maxsize=None)
def width_ladder() -> Ladder:
    return ladder_block(WIDTH_DEGS, n_opp=512, seed=6)


@functools.lru_cache(maxsize=None)
def repeat_ladder(extreme: bool = False) -> Ladder:
    """The width ladder with repeated indices: in every row of >= 2 entries the last index repeats the first, in rows
    of >= 66 entries entry 64 also repeats entry 63 (a repeat across the 64-entry batch boundary). Every entry keeps
    its own rating (1..5), or with `extreme` one drawn from EXTREME_RATINGS. No COO form."""
    lad = width_ladder()
    rp, col = lad.blk["row_ptr"], lad.blk["col"].copy()
    for i, d in enumerate(lad.degs):
        if d >= 2:
            col[rp[i + 1] - 1] = col[rp[i]]
        if d >= FOLDIN_BATCH + 2:
            col[rp[i] + FOLDIN_BATCH] = col[rp[i] + FOLDIN_BATCH - 1]
    rat = lad.blk["ratings"].copy()
    if extreme:
        rat = np.random.default_rng(9).choice(np.asarray(EXTREME_RATINGS), len(col)).astype(np.int16)
    blk = {"row_ptr": rp.copy(), "col": col, "ratings": rat, "n_rows": len(lad.degs)}
    side = oracle.Side(lad.side.ids.copy(), rp.copy(), col.copy(), rat.copy())
    return Ladder(blk, side, None, lad.degs, lad.n_opp)


def counted_once(side: oracle.Side) -> oracle.Side:
    """Copy of `side` in which an index a row lists more than once counts once: every later occurrence is removed,
    with its rating -- what a kernel computes that merges repeated indices instead of counting each."""
    keep = np.ones(len(side.col), bool)
    n = len(side.row_ptr) - 1
    for i in range(n):
        lo, hi = side.row_ptr[i], side.row_ptr[i + 1]
        _, first = np.unique(side.col[lo:hi], return_index=True)
        keep[lo:hi] = False
        keep[lo + first] = True
    rp = np.zeros_like(side.row_ptr)
    np.cumsum([keep[side.row_ptr[i]:side.row_ptr[i + 1]].sum() for i in range(n)], out=rp[1:])
    return oracle.Side(side.ids, rp, side.col[keep].copy(), side.ratings[keep].copy())


@functools.lru_cache(maxsize=None)
def width_inputs(k: int, entries: str = "distinct"):
    """(ladder, factors, fp64 oracle, the reference's fp32 result) of a width-ladder case with k features at WIDTH_LAM;
    entries: "distinct" (width_ladder), "repeat" or "extreme" (repeat_ladder). Computed once, read-only."""
    lad = {"distinct": width_ladder, "repeat": repeat_ladder, "extreme": lambda: repeat_ladder(True)}[entries]()
    F = factors(lad.n_opp, k)
    ref64, ref32 = references(lad.side, F, WIDTH_LAM)
    for a in (F, ref64, ref32):
        a.setflags(write=False)
    return lad, F, ref64, ref32


BUCKETS = ((1, 1), (2, 32), (33, 64), (65, 128), (129, 330), (1023, 1 << 30))

Ladder = namedtuple("Ladder", "blk side coo degs n_opp")
# every knob of the product library that selects a plan or a code path: cleared while an engine is created, so a case
# runs exactly the knobs it names
KNOBS = ("ALS_CHUNK", "ALS_INTERLEAVE", "ALS_XCD_RANGES", "ALS_PRESPLIT", "ALS_GRAM", "ALS_DUAL", "ALS_DUAL_SIDE",
         "ALS_FORCE_VALU", "ALS_REFINE_MIN_PIVOT")


@contextlib.contextmanager
def knobs(env):
    """The engine reads its knobs once, when it is created: set them for that moment only."""
    assert set(env) <= set(KNOBS), env
    saved = {v: os.environ.get(v) for v in KNOBS}
    for v in KNOBS:
        os.environ.pop(v, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for v, old in saved.items():
            if old is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = old


GenericPlan = namedtuple("GenericPlan", "g_in_lds batch lds_bytes slab_elems")
GENERIC_STATIC_LDS = {"f32": 4112, "f64": 16912}    # als_solve_generic's static vectors (als_plan.h)


def generic_plan(precision: str, kp: int) -> GenericPlan:
    """generic_plan of als_plan.cpp restated: the Gram's packed triangle stays in LDS while it and 8 staged rows fit
    in 160 KiB beside the static vectors (batch: what fits, at most 64), else it goes to a global slab and the staged
    rows get 64 KiB. test_plan_host.py holds this equal to the C++ for every kp = 16..1024."""
    elem = 4 if precision == "f32" else 8
    ntri = kp * (kp + 1) // 2
    tri_b, row_b = (ntri + 1) // 2 * 2 * elem, kp * elem
    avail = 160 * 1024 - GENERIC_STATIC_LDS[precision]
    if tri_b + 8 * row_b <= avail:
        batch = min(64, (avail - tri_b) // row_b)
        return GenericPlan(True, batch, tri_b + batch * row_b, 0)
    batch = max(1, min(64, 64 * 1024 // row_b))
    return GenericPlan(False, batch, batch * row_b, ntri + 1)


def ladder_block(degs=DEFAULT_DEGS, n_opp=N_OPP, seed=0, sort_cols=True) -> Ladder:
    """One in-block with row i of degs[i] distinct columns drawn from n_opp and ratings 1..5.

    blk: the CSR dict ALSEngine.set_block takes (row_ptr, col, ratings, n_rows); side: the same rows as an oracle.Side;
    coo: (rows, cols, ratings) for set_block_coo, the entries of all rows shuffled together, each row's entries in
    their CSR order (the device build's sort is stable). sort_cols: each row's columns ascending by slot, else in the
    order they were drawn."""
    rng = np.random.default_rng(seed)
    degs = np.asarray(degs, np.int64)
    assert degs.max() <= n_opp
    row_ptr = np.zeros(len(degs) + 1, np.int64)
    np.cumsum(degs, out=row_ptr[1:])
    col = np.zeros(row_ptr[-1], np.int32)
    for i, d in enumerate(degs):
        c = rng.choice(n_opp, size=int(d), replace=False)
        col[row_ptr[i]:row_ptr[i + 1]] = np.sort(c) if sort_cols else c
    ratings = rng.integers(1, 6, len(col)).astype(np.int16)
    blk = {"row_ptr": row_ptr, "col": col, "ratings": ratings, "n_rows": len(degs)}
    side = oracle.Side(np.arange(1, len(degs) + 1, dtype=np.int64), row_ptr.copy(), col.copy(), ratings.copy())
    arrival = np.repeat(np.arange(len(degs), dtype=np.int32), degs)[rng.permutation(len(col))]
    pos = np.argsort(arrival, kind="stable")      # arrival positions, grouped by row, ascending inside a row
    coo_c = np.zeros_like(col)
    coo_r = np.zeros_like(ratings)
    coo_c[pos] = col
    coo_r[pos] = ratings
    coo = {"n_rows": len(degs), "rows": arrival, "cols": coo_c, "ratings": coo_r}
    return Ladder(blk, side, coo, degs, n_opp)


def factors(n_opp: int, k: int, seed: int = 1) -> np.ndarray:
    """Signed, zero-mean opposite factors with unit-norm rows (in expectation), exactly representable in fp32."""
    rng = np.random.default_rng([seed, k])
    return (rng.standard_normal((n_opp, k)) / np.sqrt(k)).astype(np.float32).astype(np.float64)


def _without(side: oracle.Side, which) -> oracle.Side:
    """Copy of `side` without entry which(d) of every row of d >= 2 entries."""
    degs = np.diff(side.row_ptr)
    keep = np.ones(len(side.col), bool)
    for i, d in enumerate(degs):
        if d >= 2:
            keep[side.row_ptr[i] + which(int(d))] = False
    rp = np.zeros_like(side.row_ptr)
    np.cumsum(np.where(degs >= 2, degs - 1, degs), out=rp[1:])
    return oracle.Side(side.ids, rp, side.col[keep].copy(), side.ratings[keep].copy())


def mutants(side: oracle.Side) -> dict:
    """Oracle-side copies of the block that differ from it by one entry in every row of >= 2 entries: what a kernel
    computes that loses the first, the last or a middle entry of a row, or reads one rating wrong (by the least
    possible amount, 1)."""
    out = {"drop_first": _without(side, lambda d: 0), "drop_last": _without(side, lambda d: d - 1),
           "drop_middle": _without(side, lambda d: d // 2)}
    rat = side.ratings.copy()
    degs = np.diff(side.row_ptr)
    last = side.row_ptr[1:][degs >= 2] - 1
    rat[last] = np.where(rat[last] < 5, rat[last] + 1, 4)
    out["last_rating"] = oracle.Side(side.ids, side.row_ptr.copy(), side.col.copy(), rat)
    return out


def references(side: oracle.Side, F: np.ndarray, lam: float):
    """(fp64 oracle solution, the reference's own fp32 solution) of every row."""
    return (oracle.update_side(side, F, lam, "f64"),
            oracle.update_side(side, F.astype(np.float32), lam, "f32"))


def row_errors(got, ref64) -> np.ndarray:
    """Norm-relative error of every row against ref64 (0 where both are exactly zero, inf where only ref64 is)."""
    got = np.asarray(got, np.float64)
    ref64 = np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    num = np.linalg.norm(got - ref64, axis=1)
    den = np.linalg.norm(ref64, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(den > 0, num / den, np.where(num == 0, 0.0, np.inf))
    return np.where(np.isfinite(got).all(axis=1), rel, np.inf)


def rejected_rows(got, ref64, degs, precision, bound=None) -> np.ndarray:
    """Per row: True where check_rows would reject it."""
    degs = np.asarray(degs)
    rel = row_errors(got, ref64)
    bad = ~(rel <= (BOUND[precision] if bound is None else bound))
    zero = degs == 0
    bad[zero] = np.any(np.asarray(got)[zero] != 0, axis=1)
    return bad


def task_kinds(degs, k, chunk, path="mfma_split", dual=True) -> list:
    """How the plan (als_plan.cpp) solves each row: in entry space, as one FULL task, or split into n PARTIAL slots
    summed by a REDUCE task. path as ALSEngine.block_path()['gram_path']."""
    kp = 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128
    max_blocks = {64: 1, 128: 3}.get(kp, 0) if (path == "mfma_split" and dual) else 0
    chunk = 1 << 62 if path == "generic" else -(-int(chunk) // BLOCK_ENTRIES) * BLOCK_ENTRIES
    kinds = []
    for d in np.asarray(degs):
        d = int(d)
        if d == 0:
            kinds.append("empty")
        elif d > chunk:
            kinds.append(f"split into {-(-d // chunk)} slots")
        elif d <= k and -(-d // BLOCK_ENTRIES) <= max_blocks:
            kinds.append("entry-space")
        else:
            kinds.append("FULL")
    return kinds


def check_rows(got, ref64, ref32, degs, precision, kinds=None, bound=None) -> np.ndarray:
    """Every row of `got` against the fp64 oracle: norm-relative error <= 1e-4 (fp32) / 1e-8 (fp64) on each row with a
    rating, rows without one exactly zero; fp32 also p99 <= max(2 x the reference's own fp32 p99, 2e-5). ref32 (the
    reference's fp32 solution) is read for fp32 only. kinds: per-row task kind for the failure report (task_kinds).
    Returns the per-row errors; raises AssertionError naming each failing row (the 12 worst), its degree, task kind
    and error. bound: the per-row bound where it is not BOUND[precision] (anyk_bound)."""
    degs = np.asarray(degs)
    assert len(degs) == len(got) == len(ref64)
    bound = BOUND[precision] if bound is None else bound
    rel = row_errors(got, ref64)
    bad = rejected_rows(got, ref64, degs, precision, bound)
    if bad.any():
        rows = np.nonzero(bad)[0]
        worst = rows[np.argsort(-np.nan_to_num(rel[rows], posinf=1e300))][:12]
        lines = [f"row {i} deg {degs[i]} {kinds[i] if kinds is not None else ''}: err {rel[i]:.3e}" for i in worst]
        raise AssertionError(f"{len(rows)} of {len(degs)} rows beyond {bound:g} ({precision}): "
                             + "; ".join(lines))
    rated = degs > 0
    if precision == "f32":
        p99 = np.percentile(rel[rated], 99)
        p99_ref = np.percentile(row_errors(ref32, ref64)[rated], 99)
        assert p99 <= max(2 * p99_ref, 2e-5), f"p99 {p99:.3e} vs the reference's fp32 p99 {p99_ref:.3e}"
    return rel


def bucket_max(rel, degs) -> dict:
    """Largest per-row error per degree bucket (BUCKETS), for the record in test_gpu_rowshapes.py's docstring."""
    degs = np.asarray(degs)
    return {f"{lo}..{hi}" if hi < 1 << 30 else f">={lo}": float(rel[(degs >= lo) & (degs <= hi)].max())
            for lo, hi in BUCKETS}
