"""Where every kernel family stores a solved row: als_set_block's row_offset and als_set_row_layout's chunk-major slots.

Each family computes its own output address with factor_row(row_offset, rows_per_chunk, chunk_stride, row): the MFMA
tile solve, the VALU / LDS solve, the REDUCE epilogues, the entry-space solve, the generic solve, and the squared-error
kernels that read the rows back. One ladder of 41 rows (two of them empty; FULL, entry-space and split rows under a
64-entry chunk) is solved per family

  * contiguously, on a fresh engine with row_offset = 0 -- that result passes rowshapes.check_rows against the oracle;
  * as shard 1 of G = 3 with Sc = 7 rows per chunk: row_offset = Sc, als_set_row_layout(side, Sc, G * Sc), a table of
    ceil(41 / 7) * 21 rows whose last chunk is part full;
  * with row_offset = 5 and no layout;
  * under the same layout chunk by chunk (als_set_chunks on multiples of Sc, als_solve_half_chunk).

Every placed solve must put bitwise the contiguous rows (padded features included) at the mapped slots, leave every
other row's canary and the hidden sentinel rows of both tables bit for bit alone, report exactly the contiguous
als_sq_error (the task order is the same) and a clean integrity record. A layout that reaches past the table is refused
by als_solve_half before anything is launched. Under a tenth of a second per case on an MI355X, 1.5 s for the module.
"""
import functools

import numpy as np
import pytest
import torch

import rowshapes as rs

pytestmark = pytest.mark.gpu

LAM = 0.05
N_OPP = 512
# 1..8, the 32-entry block, the 64-entry chunk, 2 / 3 / 4 / 5 / 9 slots, n <= k and n > k at every k below; two empty rows
DEGS = (1, 2, 3, 4, 5, 6, 7, 8, 0, 9, 12, 16, 20, 24, 31, 32, 33, 40, 48, 63, 64, 65, 70, 80, 96, 97, 100, 127, 128,
        129, 130, 150, 180, 192, 193, 200, 220, 256, 257, 300, 0)
G, SHARD, SC = 3, 1, 7
C64 = {"ALS_CHUNK": "64"}

# (precision, k, knobs, gram_path, kernels the family stores through)
FAMILIES = [
    ("f32", 10, {}, "valu"),
    ("f64", 10, C64, "valu"),
    ("f64", 64, C64, "valu"),
    ("f32", 64, C64, "mfma_split"),
    ("f32", 128, C64, "mfma_split"),
    ("f32", 64, {**C64, "ALS_PRESPLIT": "0"}, "mfma_split"),
    ("f32", 64, {**C64, "ALS_GRAM": "f32"}, "mfma_f32"),
    ("f32", 64, {**C64, "ALS_DUAL": "0"}, "mfma_split"),
    ("f32", 64, {**C64, "ALS_INTERLEAVE": "1"}, "mfma_split"),
    ("f32", 130, {}, "generic"),
    ("f32", 273, {}, "generic"),
    ("f64", 65, {}, "generic"),
]
# the user half too for one family of each kernel: VALU fp32 / fp64, the pre-split and the f32 Gram with their REDUCE
# and entry-space launches, the generic solve in LDS, on the slab and in fp64
BOTH_SIDES = {0, 2, 3, 6, 9, 10, 11}
CASES = [(i, side) for i in range(len(FAMILIES)) for side in ((0, 1) if i in BOTH_SIDES else (0,))]


def _case_id(case):
    precision, k, env, _ = FAMILIES[case[0]]
    knobs = " ".join(f"{n[4:]}={v}" for n, v in env.items())
    return f"{precision}-k{k}{'-' + knobs if knobs else ''}-{'user' if case[1] else 'movie'}"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _ladder():
    lad = rs.ladder_block(DEGS, n_opp=N_OPP, seed=5)
    assert len(lad.degs) == 41 and int((lad.degs == 0).sum()) == 2
    assert {1, 2, 3, 4, 5, 6, 7, 8, 31, 32, 33, 63, 64, 65, 96, 97, 129, 200, 257} <= set(lad.degs.tolist())
    return lad


@functools.lru_cache(maxsize=None)
def _inputs(k):
    lad = _ladder()
    F = rs.factors(lad.n_opp, k)
    ref64, ref32 = rs.references(lad.side, F, LAM)
    for a in (F, ref64, ref32):
        a.setflags(write=False)
    return F, ref64, ref32


def _slots(n, row_offset, sc, stride):
    i = np.arange(n)
    return row_offset + i if sc == 0 else row_offset + (i // sc) * stride + i % sc


def _canary(n_table, kp, dtype):
    """A table whose every element names its row: row r holds -(1000 + r) in every column, padded ones included."""
    return torch.arange(1000, 1000 + n_table, dtype=dtype).neg().reshape(-1, 1).repeat(1, kp)


class _Placed:
    """An engine with the ladder as the block of `side` at row_offset (and, sc > 0, the chunk-major layout), its own
    table of n_table rows filled with the canary."""

    def __init__(self, cfk, family, side, n_table, row_offset=0, sc=0, stride=0):
        precision, k, env, path = family
        lad = _ladder()
        with rs.knobs(env):
            self.eng = eng = cfk.ALSEngine(k, precision)
        self.side, self.n_table = side, n_table
        eng.alloc_factors(1 - side, lad.n_opp)
        eng.alloc_factors(side, n_table)
        eng.set_block(side, lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"], row_offset, lad.n_opp)
        if sc:
            eng.set_row_layout(side, sc, stride)
        assert eng.block_path(side)["gram_path"] == path, eng.block_path(side)
        eng.write_factors(1 - side, _inputs(k)[0])
        self.canary = _canary(n_table, eng.kp, eng.dtype)
        eng.factors[side][:n_table].copy_(self.canary)
        eng.synchronize()

    def raw(self, side=None):
        self.eng.synchronize()
        return self.eng.factors[self.side if side is None else side].cpu()

    def close(self):
        self.eng.close()


def _contiguous(cfk, family, side):
    """The contiguous solve of a family: (raw rows [41, kp] as the kernels stored them, als_sq_error, block_stats)."""
    precision, k, env, path = family
    lad = _ladder()
    F, ref64, ref32 = _inputs(k)
    p = _Placed(cfk, family, side, len(lad.degs))
    try:
        stats, bp = p.eng.block_stats(side), p.eng.block_path(side)
        p.eng.solve_half(side, LAM)
        raw = p.raw()
        got = p.eng.read_factors(side, 0, len(lad.degs))
        assert np.array_equal(raw[:-1, :k].numpy(), got)
        chunk = int(env.get("ALS_CHUNK", 1024))
        kinds = rs.task_kinds(lad.degs, k, chunk, path, env.get("ALS_DUAL", "1") != "0")
        rs.check_rows(got, ref64, ref32, lad.degs, precision, kinds)
        assert not raw[-1].any() and not p.raw(1 - side)[-1].any()
        assert p.eng.integrity_status() == [0, 0, 0, 0]
        se = p.eng.sq_error(side)
        assert se[1] == int(lad.degs.sum())
        # the family stores through the launches it is here for
        if "ALS_CHUNK" in env:
            assert stats["n_reduce"] == int((lad.degs > 64).sum()) == 19, stats
            dual = path == "mfma_split" and env.get("ALS_DUAL", "1") != "0"
            assert (bp["dual_rows"] > 0) == dual, bp
            assert p.eng.split_info(side)["interleaved_rows"] == (19 if env.get("ALS_INTERLEAVE") == "1" else 0)
        else:
            assert stats["n_reduce"] == 0 and bp["dual_rows"] == 0, (stats, bp)
        if path == "generic":      # k = 130 and fp64 k = 65 keep the Gram in LDS, k = 273 is the slab variant
            assert rs.generic_plan(precision, p.eng.kp).g_in_lds == (k != 273)
        return raw[:-1], se
    finally:
        p.close()


def _assert_placed(p, slots, want_raw, want_se):
    """The placed engine after its solve: the contiguous rows at `slots`, every other row its canary, both sentinel
    rows zero, the same squared error, a clean record."""
    raw = p.raw()
    assert raw.shape[0] == p.n_table + 1
    at = raw[torch.as_tensor(slots)]
    assert torch.equal(at, want_raw), np.nonzero((at != want_raw).any(dim=1).numpy())[0][:8]
    others = np.setdiff1d(np.arange(p.n_table), slots)
    assert len(others) == p.n_table - len(slots)
    o = torch.as_tensor(others)
    assert torch.equal(raw[o], p.canary[o]), others[(raw[o] != p.canary[o]).any(dim=1).numpy()][:8]
    assert not raw[-1].any() and not p.raw(1 - p.side)[-1].any()
    assert p.eng.sq_error(p.side) == want_se
    assert p.eng.integrity_status() == [0, 0, 0, 0]


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_rows_land_at_their_slots(cfk, case):
    family, side = FAMILIES[case[0]], case[1]
    n = len(DEGS)
    want_raw, want_se = _contiguous(cfk, family, side)
    n_chunks = -(-n // SC)
    assert n % SC != 0 and n_chunks == 6
    n_table = n_chunks * G * SC
    slots = _slots(n, SHARD * SC, SC, G * SC)
    assert slots[0] == 7 and slots[6] == 13 and slots[7] == 28 and slots[-1] == 7 + 5 * 21 + 5 < n_table

    # the chunk-major layout, one launch per list
    p = _Placed(cfk, family, side, n_table, SHARD * SC, SC, G * SC)
    try:
        p.eng.solve_half(side, LAM)
        _assert_placed(p, slots, want_raw, want_se)
        p.eng.solve_half(side, LAM)          # a second half over the stored rows: the same rows again
        _assert_placed(p, slots, want_raw, want_se)
    finally:
        p.close()

    # a plain row offset
    p = _Placed(cfk, family, side, n + 9, 5)
    try:
        p.eng.solve_half(side, LAM)
        _assert_placed(p, _slots(n, 5, 0, 0), want_raw, want_se)
    finally:
        p.close()

    # the layout, chunk by chunk: after chunk c only the chunks up to c are stored
    p = _Placed(cfk, family, side, n_table, SHARD * SC, SC, G * SC)
    try:
        bounds = [min(c * SC, n) for c in range(n_chunks + 1)]
        p.eng.set_chunks(side, bounds)
        for c in range(n_chunks):
            p.eng.solve_half_chunk(side, LAM, c)
            if c == 2:
                raw = p.raw()
                done = torch.as_tensor(slots[:bounds[3]])
                rest = torch.as_tensor(np.setdiff1d(np.arange(n_table), slots[:bounds[3]]))
                assert torch.equal(raw[done], want_raw[:bounds[3]]) and torch.equal(raw[rest], p.canary[rest])
        _assert_placed(p, slots, want_raw, want_se)
    finally:
        p.close()


@pytest.mark.parametrize("family", [FAMILIES[3], FAMILIES[9]], ids=["f32-k64", "f32-k130"])
def test_layout_past_the_table_is_refused(cfk, family):
    """The last row's slot (117) in a table of 117 rows: als_solve_half and als_solve_half_chunk return ALS_ERR_STATE
    before any launch, and the table keeps its canary."""
    n = len(DEGS)
    slots = _slots(n, SHARD * SC, SC, G * SC)
    p = _Placed(cfk, family, 0, int(slots[-1]), SHARD * SC, SC, G * SC)
    try:
        with pytest.raises(cfk.ALSError) as e:
            p.eng.solve_half(0, LAM)
        assert e.value.status == 5 and "ALS_ERR_STATE" in str(e.value) and "exceed factor rows 117" in str(e.value)
        p.eng.set_chunks(0, [0, SC, n])
        with pytest.raises(cfk.ALSError) as e:
            p.eng.solve_half_chunk(0, LAM, 0)
        assert e.value.status == 5
        raw = p.raw()
        assert torch.equal(raw[:-1], p.canary) and not raw[-1].any()
        assert p.eng.integrity_status() == [0, 0, 0, 0]
        # one more row and the same layout fits
        q = _Placed(cfk, family, 0, int(slots[-1]) + 1, SHARD * SC, SC, G * SC)
        try:
            q.eng.solve_half(0, LAM)
            assert not torch.equal(q.raw()[int(slots[-1])], q.canary[int(slots[-1])])
        finally:
            q.close()
    finally:
        p.close()
