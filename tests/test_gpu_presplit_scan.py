"""GPU: the one-pass preparation of the pre-split table (als_presplit_scan + als_presplit_confirm).

The scan splits the opposite table at the exponent that side's table was last split at and accumulates the table's
range words on the way; the confirm launch splits it again only when the true exponent differs. Whatever an engine
did before, the table a half gathers is therefore the one a fresh engine would make, and every comparison here is
bitwise: np.array_equal on the factor rows against a fresh engine's result on the same table.

Blocks are small ladders of tests/rowshapes.py (rows of 1..257 entries, one without a rating; ALS_CHUNK = 64, so the
long rows are split into PARTIAL slots and a REDUCE task) over opposite tables of 2, 63 and 257 rows plus the
sentinel: fewer items than one wave, a last workgroup that is part full, and more than one 1024-item workgroup at
k = 128 (257 rows x 16 items). k = 64 and 128, both sides.
"""
import functools
import os

import numpy as np
import pytest
import torch

import rowshapes as rs

pytestmark = pytest.mark.gpu

LAM = 0.05
TABLES = (2, 63, 257)
DEGS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 96, 97, 129, 200, 257)
CASES = [(k, side) for k in (64, 128) for side in (0, 1)]


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for v in ("ALS_INTERLEAVE", "ALS_XCD_RANGES", "ALS_PRESPLIT", "ALS_GRAM", "ALS_DUAL", "ALS_DUAL_SIDE",
              "ALS_FORCE_VALU", "ALS_REFINE_MIN_PIVOT"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("ALS_CHUNK", "64")


@functools.lru_cache(maxsize=None)
def _ladder(n_opp, max_rows=None):
    degs = tuple(d for d in DEGS if d <= n_opp)[:max_rows] + ((0,) if max_rows is None else ())
    return rs.ladder_block(degs=degs, n_opp=n_opp, seed=n_opp)


@functools.lru_cache(maxsize=None)
def _table(n_opp, k):
    F = rs.factors(n_opp, k, seed=n_opp).astype(np.float32)
    F.setflags(write=False)
    return F


def _engine(cfk, k, side, lad, presplit=None):
    """An engine with `lad` as the block of `side`. The engine reads its knobs when it is created."""
    if presplit is not None:
        os.environ["ALS_PRESPLIT"] = presplit
    try:
        eng = cfk.ALSEngine(k, "f32")
    finally:
        os.environ.pop("ALS_PRESPLIT", None)
    eng.alloc_factors(1 - side, lad.n_opp)
    eng.alloc_factors(side, lad.blk["n_rows"])
    eng.set_block(side, lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"], 0, lad.n_opp)
    assert eng.block_path(side)["presplit"] == (presplit != "0")
    return eng


def _solve(eng, side, F, n_rows):
    """Write F as the opposite table of `side`, clear the side's own rows, solve the half, return its rows."""
    eng.write_factors(1 - side, F)
    eng.write_factors(side, np.zeros((n_rows, eng.k), np.float32))
    eng.solve_half(side, LAM)
    got = eng.read_factors(side, 0, n_rows)
    assert eng.integrity_status() == [0, 0, 0, 0]
    return got


def _fresh(cfk, k, side, lad, F, presplit=None):
    """What an engine without a history makes of table F: the first preparation of a side has no prediction."""
    eng = _engine(cfk, k, side, lad, presplit)
    try:
        return _solve(eng, side, F, lad.blk["n_rows"])
    finally:
        eng.close()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _with_max(F, value):
    """F with element [0, 0] set to `value`, which is larger than every other |x| of it."""
    G = F.copy()
    assert np.abs(F).max() < abs(value)
    G[0, 0] = value
    return G


@pytest.mark.parametrize("k,side", CASES)
def test_three_histories_one_answer(cfk, k, side):
    """No prediction (fresh engine), a wrong one (the table was X * 2^3 before) and a right one (X twice) end in the
    same bits: the first two through the repair path, the third through the fast path."""
    for n_opp in TABLES:
        lad, X = _ladder(n_opp), _table(n_opp, k)
        n = lad.blk["n_rows"]
        a = _fresh(cfk, k, side, lad, X)
        assert np.all(np.isfinite(a)) and np.any(a != 0)
        eng = _engine(cfk, k, side, lad)
        try:
            _solve(eng, side, X * np.float32(8), n)
            b = _solve(eng, side, X, n)
            c = _solve(eng, side, X, n)
        finally:
            eng.close()
        assert _same(a, b), (n_opp, "wrong prediction")
        assert _same(a, c), (n_opp, "right prediction")


@pytest.mark.parametrize("k,side", CASES)
def test_largest_magnitude_of_either_sign(cfk, k, side):
    """The scale comes from the largest |x|, whatever its sign and the signs next to it: one element of magnitude 4
    in a row whose other elements have the opposite sign (all other |x| < 1), as -4 among positive ones and as +4
    among negative ones. A maximum taken from the signed values, or from the raw bits before the sign is cleared,
    misses one of the two; the table is then scaled by 2^14 or more and the element's fp16 head overflows
    (4 x 2^14 = 65536 rounds to Inf), leaving Inf or NaN in the rows that gather it.
    Every row finite, and within 2e-3 (norm-relative) of the on-the-fly split's result on a fresh engine, which uses
    no range words: each result keeps the per-row fp32 bound of tests/rowshapes.py, 1e-4 on unit-norm rows, against
    the oracle, and the one row of squared norm 17 instead of 1 raises a gathering row's condition number, and with
    it the fp32 solve's error, at most 17-fold. On the repair path and on the fast path."""
    for n_opp in TABLES:
        lad, X = _ladder(n_opp), _table(n_opp, k)
        n = lad.blk["n_rows"]
        assert np.abs(X).max() < 1
        for sign in (1.0, -1.0):
            T = X.copy()
            T[n_opp - 1] = sign * np.abs(X[n_opp - 1])
            T[n_opp - 1, k // 2] = -4.0 * sign
            ref = _fresh(cfk, k, side, lad, T, presplit="0").astype(np.float64)
            assert np.all(np.isfinite(ref))
            eng = _engine(cfk, k, side, lad)
            try:
                for _ in range(2):
                    got = _solve(eng, side, T, n)
                    assert np.all(np.isfinite(got)), (n_opp, sign)
                    err = np.linalg.norm(got - ref, axis=1)
                    assert np.all(err <= 2e-3 * np.linalg.norm(ref, axis=1)), (n_opp, sign, err.max())
            finally:
                eng.close()


@pytest.mark.parametrize("k,side", CASES)
def test_exponent_boundary(cfk, k, side):
    """Table maxima of exactly 2^e, the float below and the float above (the last one has another split_exp), each
    solved on an engine whose prediction is that of the middle one."""
    one = np.float32(1.0)
    for n_opp in TABLES:
        lad, X = _ladder(n_opp), _table(n_opp, k)
        n = lad.blk["n_rows"]
        tabs = {"at": _with_max(X, one), "below": _with_max(X, np.nextafter(one, np.float32(0))),
                "above": _with_max(X, np.nextafter(one, np.float32(2)))}
        want = {name: _fresh(cfk, k, side, lad, T) for name, T in tabs.items()}
        eng = _engine(cfk, k, side, lad)
        try:
            _solve(eng, side, tabs["at"], n)
            assert _same(_solve(eng, side, tabs["at"], n), want["at"]), n_opp
            for name in ("below", "at", "above", "at"):
                assert _same(_solve(eng, side, tabs[name], n), want[name]), (n_opp, name)
        finally:
            eng.close()


@pytest.mark.parametrize("k,side", CASES)
def test_scale_follows_the_table_down(cfk, k, side):
    """Three solves on one engine, the table 2^6 smaller each time: a maximum left over in a set of range words that
    was not zeroed would keep the old scale and change bits."""
    for n_opp in TABLES:
        lad, X = _ladder(n_opp), _table(n_opp, k)
        n = lad.blk["n_rows"]
        tabs = [X * np.float32(2.0 ** (-6 * j)) for j in range(3)]
        want = [_fresh(cfk, k, side, lad, T) for T in tabs]
        eng = _engine(cfk, k, side, lad)
        try:
            for j, T in enumerate(tabs):
                assert _same(_solve(eng, side, T, n), want[j]), (n_opp, j)
        finally:
            eng.close()


@pytest.mark.parametrize("k", [64, 128])
def test_scale_follows_both_tables_down(cfk, k):
    """The same with the two sides of one engine solved in turn, so the two sets of range words serve different
    tables alternately: side 0 gathers a table of N rows, side 1 the side-0 table (as many rows as side 0's block)."""
    for n_opp in TABLES:
        lad0 = _ladder(n_opp)
        n0 = lad0.blk["n_rows"]
        lad1 = _ladder(n0, n_opp)              # side 1's rows live in the N-row table
        n1 = lad1.blk["n_rows"]
        tabs0 = [_table(n_opp, k) * np.float32(2.0 ** (-6 * j)) for j in range(3)]
        tabs1 = [_table(n0, k) * np.float32(2.0 ** (5 - 6 * j)) for j in range(3)]
        want0 = [_fresh(cfk, k, 0, lad0, T) for T in tabs0]
        want1 = [_fresh(cfk, k, 1, lad1, T) for T in tabs1]
        eng = cfk.ALSEngine(k, "f32")
        try:
            eng.alloc_factors(0, n0)
            eng.alloc_factors(1, n_opp)
            eng.set_block(0, lad0.blk["row_ptr"], lad0.blk["col"], lad0.blk["ratings"], 0, n_opp)
            eng.set_block(1, lad1.blk["row_ptr"], lad1.blk["col"], lad1.blk["ratings"], 0, n0)
            for j in range(3):
                eng.write_factors(1, tabs0[j])
                eng.write_factors(0, np.zeros((n0, k), np.float32))
                eng.solve_half(0, LAM)
                assert _same(eng.read_factors(0, 0, n0), want0[j]), (n_opp, j, "side 0")
                eng.write_factors(0, tabs1[j])
                eng.write_factors(1, np.zeros((n_opp, k), np.float32))
                eng.solve_half(1, LAM)
                assert _same(eng.read_factors(1, 0, n1), want1[j]), (n_opp, j, "side 1")
            assert eng.integrity_status() == [0, 0, 0, 0]
        finally:
            eng.close()


@pytest.mark.parametrize("k,side", CASES)
def test_range_guard_after_warm_up(cfk, k, side):
    """After a right-prediction solve, a table whose row maxima span 2^-24..1 stands the pre-split down: the result
    is that of the on-the-fly split (ALS_PRESPLIT=0, fresh engine), as tests/test_gpu_integrity.py checks on first
    use. An in-range table after it gives a fresh engine's result again. (On these well-scaled tables the two splits
    can round to the same rows -- they do at k = 128 over 63 rows --, so which launch served the last solve is not
    read off the bits here; the range words it keys on are the ones the out-of-range solve before it had to get
    right.)"""
    for n_opp in TABLES:
        lad, X = _ladder(n_opp), _table(n_opp, k)
        n = lad.blk["n_rows"]
        rng = np.random.default_rng([k, n_opp])
        W = rng.random((n_opp, k)) * 2.0 ** -rng.uniform(0, 24, size=(n_opp, 1))
        W[0] *= 1.0 / W[0].max()
        W[1] *= 2.0 ** -24 / W[1].max()
        W = W.astype(np.float32)
        want_w = _fresh(cfk, k, side, lad, W, presplit="0")
        want_x = _fresh(cfk, k, side, lad, X)
        eng = _engine(cfk, k, side, lad)
        try:
            _solve(eng, side, X, n)
            assert _same(_solve(eng, side, X, n), want_x), n_opp
            assert _same(_solve(eng, side, W, n), want_w), (n_opp, "out of range")
            assert _same(_solve(eng, side, X, n), want_x), (n_opp, "in range again")
        finally:
            eng.close()


@pytest.mark.parametrize("k,side", CASES)
def test_inf_and_nan_on_the_second_solve(cfk, k, side):
    """One Inf or NaN element in the table of the second solve: the output is a fresh engine's on that table."""
    for n_opp in TABLES:
        lad, X = _ladder(n_opp), _table(n_opp, k)
        n = lad.blk["n_rows"]
        want_x = _fresh(cfk, k, side, lad, X)
        for bad in (np.inf, -np.inf, np.nan):
            T = X.copy()
            T[n_opp - 1, k - 1] = bad
            want = _fresh(cfk, k, side, lad, T)
            eng = _engine(cfk, k, side, lad)
            try:
                _solve(eng, side, X, n)
                assert _same(_solve(eng, side, T, n), want), (n_opp, bad)
                assert _same(_solve(eng, side, X, n), want_x), (n_opp, bad, "after")
            finally:
                eng.close()


@pytest.mark.parametrize("k,side", CASES)
def test_chunked_half_reuses_the_conversion(cfk, k, side):
    """als_set_chunks with three chunks: chunk 0 prepares the table, chunks 1 and 2 reuse its planes and range words;
    the rows equal the one-piece half's, with no prediction and with a right one."""
    for n_opp in TABLES:
        lad, X = _ladder(n_opp), _table(n_opp, k)
        n = lad.blk["n_rows"]
        want = _fresh(cfk, k, side, lad, X)
        eng = _engine(cfk, k, side, lad)
        try:
            eng.set_chunks(side, [0, n // 3, 2 * n // 3, n])
            for _ in range(2):
                eng.write_factors(1 - side, X)
                eng.write_factors(side, np.zeros((n, k), np.float32))
                for c in range(3):
                    eng.solve_half_chunk(side, LAM, c)
                assert _same(eng.read_factors(side, 0, n), want), n_opp
            assert eng.integrity_status() == [0, 0, 0, 0]
        finally:
            eng.close()
