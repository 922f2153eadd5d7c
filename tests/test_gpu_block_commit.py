"""A failed als_set_block / als_set_chunks leaves the side as it was, a replaced block is a fresh block, and the timing
events of many halves come from the engine's pool and go back to it.

One k = 128 fp32 engine with ALS_CHUNK=64 and a 40-row block from the degree ladder (tests/rowshapes.py): empty rows,
rows of at most 32 and at most 64 entries (solved in entry space) and one row of 200 entries (4 PARTIAL slots and a
REDUCE task), on the pre-split Gram. Every test first asserts that the REDUCE list, the entry-space lists and the
pre-split operands exist, so none of them can pass on an empty list. All provoked failures are validated on the host;
every comparison is bitwise.
"""
import numpy as np
import pytest
import torch

import rowshapes as rs
from test_gpu_rowshapes import _knobs

pytestmark = pytest.mark.gpu

K, LAM, N_OPP, N_FAC = 128, 0.05, 512, 48
DEGS_A = (0, 1, 2, 3, 5, 8, 13, 21, 31, 32, 33, 34, 40, 47, 48, 50, 55, 60, 63, 64,
          200, 4, 16, 30, 62, 7, 9, 11, 12, 17, 0, 35, 36, 45, 57, 58, 59, 61, 6, 10)
BOUNDS = [0, 10, 25, 40]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def blocks():
    a = rs.ladder_block(DEGS_A, N_OPP, seed=3)
    b = rs.ladder_block(DEGS_A[::-1], N_OPP, seed=4)
    F = rs.factors(N_OPP, K)
    F.setflags(write=False)
    assert len(DEGS_A) == 40 and a.blk["col"].tolist() != b.blk["col"].tolist()
    return a, b, F


def _engine(cfk, lad, F, side=0):
    with _knobs({"ALS_CHUNK": "64"}):
        eng = cfk.ALSEngine(K, "f32")
    eng.alloc_factors(1 - side, lad.n_opp)
    eng.alloc_factors(side, N_FAC)
    eng.set_block(side, lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"], 0, lad.n_opp)
    eng.write_factors(1 - side, F)
    return eng


def _fails(status):
    from cfk_amd._lib import ALSError     # (loaded by the cfk fixture)
    return pytest.raises(ALSError, match=status)


def _plan(eng, side=0):
    """The block's plan facts; asserts that no list this module relies on is empty."""
    stats, path, info = eng.block_stats(side), eng.block_path(side), eng.split_info(side)
    assert stats["n_reduce"] > 0 and path["dual_rows"] > 0 and path["presplit"] is True, (stats, path)
    return stats, path, info


def _solve(eng, side=0, chunks=None):
    """The side's factor rows after one half from zeroed rows (so a half that wrote nothing cannot pass)."""
    eng.factors[side].zero_()
    if chunks is None:
        eng.solve_half(side, LAM)
    else:
        for c in range(chunks):
            eng.solve_half_chunk(side, LAM, c)
    out = eng.read_factors(side, 0, N_FAC)
    assert eng.integrity_status() == [0, 0, 0, 0]
    assert np.any(out != 0)
    return out


def test_failed_set_block_keeps_the_block(cfk, blocks):
    a, _, F = blocks
    eng = _engine(cfk, a, F)
    try:
        plan = _plan(eng)
        first = _solve(eng)
        c = a.coo
        bad_cols = c["cols"].copy()
        bad_cols[len(bad_cols) // 2] = a.n_opp
        with _fails("ALS_ERR_INVALID_ARGUMENT"):
            eng.set_block_coo(0, c["n_rows"], c["rows"], bad_cols, c["ratings"], 0, a.n_opp)
        bad_ptr = a.blk["row_ptr"].copy()
        bad_ptr[20] = bad_ptr[19] - 1
        with _fails("ALS_ERR_INVALID_ARGUMENT"):
            eng.set_block(0, bad_ptr, a.blk["col"], a.blk["ratings"], 0, a.n_opp)
        assert _plan(eng) == plan
        assert np.array_equal(_solve(eng), first)
    finally:
        eng.close()


def test_replaced_block_is_a_fresh_block(cfk, blocks):
    a, b, F = blocks
    eng, fresh = _engine(cfk, a, F), _engine(cfk, b, F)
    try:
        _plan(eng)
        eng.set_chunks(0, BOUNDS)
        eng.set_row_layout(0, 20, 24)
        scattered = _solve(eng, chunks=3)
        assert np.any(scattered[40:44] != 0) and not np.any(scattered[20:24] != 0)   # the layout was in force
        eng.set_block(0, b.blk["row_ptr"], b.blk["col"], b.blk["ratings"], 0, b.n_opp)
        with _fails("ALS_ERR_STATE"):
            eng.solve_half_chunk(0, LAM, 0)
        assert _plan(eng) == _plan(fresh)
        assert np.array_equal(_solve(eng), _solve(fresh))
    finally:
        eng.close()
        fresh.close()


def test_failed_set_chunks_keeps_the_chunks(cfk, blocks):
    a, _, F = blocks
    eng = _engine(cfk, a, F)
    try:
        _plan(eng)
        whole = _solve(eng)
        eng.set_chunks(0, BOUNDS)
        with _fails("ALS_ERR_INVALID_ARGUMENT"):
            eng.set_chunks(0, [0, 25, 10, 40])
        assert np.array_equal(_solve(eng, chunks=3), whole)
    finally:
        eng.close()


def test_timing_across_many_halves(cfk, blocks):
    a, _, F = blocks
    with _knobs({"ALS_CHUNK": "64"}):
        eng = cfk.ALSEngine(K, "f32")
    try:
        for side in (0, 1):   # the same block on both sides of two N_OPP-row factor matrices
            eng.alloc_factors(side, a.n_opp)
        for side in (0, 1):
            eng.set_block(side, a.blk["row_ptr"], a.blk["col"], a.blk["ratings"], 0, a.n_opp)
            eng.write_factors(side, F)
            _plan(eng, side)
        eng.set_timing(True)
        for _ in range(2):   # the second round reuses the events the first returned to the pool
            for i in range(20):
                eng.solve_half(i % 2, LAM)
            for side in (0, 1):
                gram, reduce, n = eng.timing_collect(side)
                assert n == 10, (side, n)
                assert np.isfinite(gram) and np.isfinite(reduce) and gram >= 0 and reduce >= 0, (gram, reduce)
        assert eng.timing_collect(0)[2] == 0 and eng.timing_collect(1)[2] == 0
        assert eng.integrity_status() == [0, 0, 0, 0]
    finally:
        eng.close()
