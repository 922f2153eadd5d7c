"""Every solve path on the degree ladder (tests/rowshapes.py), every row against the fp64 oracle.

One in-block with a row of each degree 1..330, twelve rows of 1023..4000 entries and two empty rows goes through
als_set_block / als_solve_half once per path: the split path under a forced 64- or 128-entry chunk (FULL rows up to the
chunk, 2..63 PARTIAL slots beyond, k below and at its padded stride), the pre-split and on-the-fly Grams, the exact f32
Gram, the entry-space solve on and off, the interleaved plan with and without XCD ranges on sorted and unsorted
columns, the unforced plan, fp64, the generic path, lambda = 1, the device block build and the chunked half. Each case
asserts: rowshapes.check_rows on ALL rows (1e-4 per row in fp32, 1e-8 in fp64, empty rows exactly zero), a clean
integrity record, a bitwise repeat, the plan facts that prove the intended path ran (worked out here from the degrees),
and als_sq_error against the oracle's. test_rowshapes_host.py shows on the CPU that this check rejects a block that
differs by one entry in any row with a 5x margin. A few seconds per case; test_gpu_fullscale.py and
test_gpu_interleave.py remain the checks at scale.

Largest per-row error measured on an MI355X (lambda = 0.05, ALS_CHUNK=64, default knobs otherwise), per degree bucket,
next to the reference's own fp32 arithmetic (oracle, f32 mode) on the same rows:

    degree      k = 64: GPU   reference fp32      k = 128: GPU   reference fp32
    1             7.5e-08        4.1e-06             2.5e-08        5.6e-06
    2..32         2.5e-07        2.9e-06             2.5e-07        3.1e-06
    33..64        2.9e-07        5.0e-07             2.9e-07        7.0e-07
    65..128       2.5e-07        5.1e-07             3.0e-07        5.6e-07
    129..330      2.8e-07        6.3e-07             3.4e-07        6.3e-07
    >= 1023       2.8e-07        1.3e-06             2.7e-07        1.3e-06

Over all fp32 cases of this module the largest per-row error was 2.0e-06 (k = 130, generic path, a one-rating row;
1.4e-06 on the VALU Gram at k = 10, 1.3e-06 with ALS_GRAM=f32 or ALS_DUAL=0), over the fp64 cases 1.3e-14: the 1e-4 and
1e-8 bounds have 50x and more to spare, and the nearest one-entry mutant is >= 1.5e-3 away.
"""
import functools

import numpy as np
import pytest
import torch

import rowshapes as rs

pytestmark = pytest.mark.gpu

LAM = 0.05
KNOBS = rs.KNOBS      # the knobs a case may name; rs.knobs clears the rest while its engine is created
_knobs = rs.knobs


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _ladder(sort_cols=True):
    return rs.ladder_block(sort_cols=sort_cols)


@functools.lru_cache(maxsize=None)
def _inputs(k, lam=LAM, sort_cols=True):
    """(factors, fp64 oracle, the reference's fp32 result) of a case: computed once, shared, read-only."""
    lad = _ladder(sort_cols)
    F = rs.factors(lad.n_opp, k)
    ref64, ref32 = rs.references(lad.side, F, lam)
    for a in (F, ref64, ref32):
        a.setflags(write=False)
    return F, ref64, ref32


def _ceil_blocks(n):
    return -(-int(n) // rs.BLOCK_ENTRIES) * rs.BLOCK_ENTRIES


def _expected_plan(degs, k, precision, env):
    """What als_plan.cpp makes of the ladder under `env`, worked out from the degrees (4096 opposite rows: the
    pre-split table is 1 or 2 MB, so the pre-split Gram is the default wherever it exists and the interleave is off
    unless forced)."""
    generic = k > (64 if precision == "f64" else 128)
    path = "generic" if generic else "valu" if (precision == "f64" or k < 32) else \
        "mfma_f32" if env.get("ALS_GRAM") == "f32" else "mfma_split"
    kp = 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128
    nnz_padded = sum(_ceil_blocks(d) for d in degs)
    chunk = _ceil_blocks(env["ALS_CHUNK"]) if "ALS_CHUNK" in env else \
        _ceil_blocks(min(max(nnz_padded // 4096, 1024), 32768))
    can_presplit = path == "mfma_split" and kp in (64, 128)
    kinds = rs.task_kinds(degs, k, chunk, path, env.get("ALS_DUAL", "1") != "0")
    split = np.array([kd.startswith("split") for kd in kinds])
    ilv = can_presplit and env.get("ALS_INTERLEAVE") == "1"
    slots = int(sum(-(-int(d) // chunk) for d in degs[split]))
    return {"gram_path": path, "chunk": chunk, "kinds": kinds,
            "presplit": can_presplit and env.get("ALS_PRESPLIT", "1") != "0",
            "dual_rows": kinds.count("entry-space"),
            "n_reduce": int(split.sum()),
            "n_tasks": int((~split).sum()) + slots,
            "interleaved_rows": int(split.sum()) if ilv else 0,
            "chunk_tasks": slots if ilv else 0,
            "ranges": ilv and env.get("ALS_XCD_RANGES") == "1"}


def _engine(cfk, lad, k, precision, env, side=0, coo=False):
    with _knobs(env):
        eng = cfk.ALSEngine(k, precision)
    eng.use_torch_stream()
    eng.alloc_factors(1 - side, lad.n_opp)
    eng.alloc_factors(side, lad.blk["n_rows"])
    if coo:
        c = lad.coo
        eng.set_block_coo(side, c["n_rows"], c["rows"], c["cols"], c["ratings"], 0, lad.n_opp)
    else:
        eng.set_block(side, lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"], 0, lad.n_opp)
    return eng


def _assert_plan(eng, side, exp):
    path, stats, info = eng.block_path(side), eng.block_stats(side), eng.split_info(side)
    assert path["gram_path"] == exp["gram_path"], path
    assert path["chunk"] == exp["chunk"], path
    assert path["presplit"] == exp["presplit"] == info["presplit"], (path, info)
    assert path["dual_rows"] == exp["dual_rows"], (path, exp["dual_rows"])
    assert stats["n_reduce"] == exp["n_reduce"], stats
    assert info["interleaved_rows"] == exp["interleaved_rows"], info
    if exp["interleaved_rows"]:
        assert info["chunk"] == exp["chunk"], info     # the contiguous chunk caps the interleave length
    if exp["ranges"]:   # a chunk per range a row reaches: never fewer tasks than the plain interleave
        assert info["chunk_tasks"] >= exp["chunk_tasks"] and stats["n_tasks"] >= exp["n_tasks"], (info, stats)
    else:
        assert info["chunk_tasks"] == exp["chunk_tasks"] and stats["n_tasks"] == exp["n_tasks"], (info, stats)


def _run_case(cfk, k, precision="f32", env=None, lam=LAM, sort_cols=True, side=0, coo=False, label=""):
    """One half of the ladder under `env` with every assertion of this module; returns (output, block_stats)."""
    env = dict(env or {})
    lad = _ladder(sort_cols)
    F, ref64, ref32 = _inputs(k, lam, sort_cols)
    exp = _expected_plan(lad.degs, k, precision, env)
    eng = _engine(cfk, lad, k, precision, env, side, coo)
    try:
        _assert_plan(eng, side, exp)
        eng.write_factors(1 - side, F)
        eng.solve_half(side, lam)
        got = eng.read_factors(side, 0, lad.blk["n_rows"])
        rel = rs.check_rows(got, ref64, ref32, lad.degs, precision, exp["kinds"])
        print(f"\n[{label or env}] k={k} {precision} lam={lam}: per-row max {rel.max():.2e} "
              f"{rs.bucket_max(rel, lad.degs)}; reference fp32 {rs.bucket_max(rs.row_errors(ref32, ref64), lad.degs)}")
        assert eng.integrity_status() == [0, 0, 0, 0]
        se, cnt = eng.sq_error(side)
        se_o, cnt_o = rs.oracle.sq_error(lad.side, got.astype(np.float64), F)
        assert cnt == cnt_o == int(lad.degs.sum())
        assert se == pytest.approx(se_o, rel=1e-5 if precision == "f32" else 1e-12)
        eng.solve_half(side, lam)
        again = eng.read_factors(side, 0, lad.blk["n_rows"])
        assert np.array_equal(again, got), np.nonzero(np.any(again != got, axis=1))[0][:8]
        assert eng.integrity_status() == [0, 0, 0, 0]
        return got, eng.block_stats(side)
    finally:
        eng.close()


SPLIT64 = [(k, {"ALS_CHUNK": "64"}) for k in (32, 40, 64, 70, 96, 128)] + \
          [(k, {"ALS_CHUNK": "64", **extra}) for k in (64, 128)
           for extra in ({"ALS_PRESPLIT": "0"}, {"ALS_GRAM": "f32"}, {"ALS_DUAL": "0"})] + \
          [(128, {"ALS_CHUNK": "128"})]


def _id(v):
    return " ".join(f"{n[4:]}={x}" for n, x in v.items()) if isinstance(v, dict) else None


@pytest.mark.parametrize("k,env", SPLIT64, ids=_id)
def test_f32_split_path(cfk, k, env):
    """Path 1: FULL rows up to the chunk, 2..63 PARTIAL slots + a REDUCE beyond; KP = 32 / 64 / 128 each with k < KP
    and k = KP; the on-the-fly split Gram, the exact f32 Gram and the k x k solve of short rows at k = 64 and 128."""
    _run_case(cfk, k, "f32", env)


@pytest.mark.parametrize("sort_cols", [True, False], ids=["sorted", "arrival"])
@pytest.mark.parametrize("k", [64, 128, 40])
def test_interleaved_plan(cfk, k, sort_cols):
    """Path 2: every row above 64 entries interleaved (ALS_INTERLEAVE=1, the 64-entry chunk caps its length), with and
    without XCD ranges, on columns ascending by slot and in arrival order (the range grouping reads the first column
    of each block; correctness must not depend on the order). Each plan against the oracle, and the three plans
    (ranges, plain interleave, contiguous) against each other within the same bound."""
    base = {"ALS_CHUNK": "64"}
    outs = {}
    for name, env in (("ranges", {**base, "ALS_INTERLEAVE": "1", "ALS_XCD_RANGES": "1"}),
                      ("interleaved", {**base, "ALS_INTERLEAVE": "1", "ALS_XCD_RANGES": "0"}),
                      ("contiguous", {**base, "ALS_INTERLEAVE": "0"})):
        outs[name], _ = _run_case(cfk, k, "f32", env, sort_cols=sort_cols, label=name)
    lad = _ladder(sort_cols)
    assert int((lad.degs > 64).sum()) == 278
    ref64 = _inputs(k, LAM, sort_cols)[1]
    den = np.where(lad.degs > 0, np.linalg.norm(ref64, axis=1), 1.0)
    for a, b in (("ranges", "interleaved"), ("ranges", "contiguous"), ("interleaved", "contiguous")):
        d = np.linalg.norm(outs[a].astype(np.float64) - outs[b], axis=1) / den
        assert d.max() <= rs.BOUND["f32"], (a, b, int(d.argmax()), lad.degs[d.argmax()], d.max())
    # rows no plan splits are the same FULL / entry-space tasks in all three
    short = lad.degs <= 64
    assert np.array_equal(outs["ranges"][short], outs["contiguous"][short])
    assert np.array_equal(outs["interleaved"][short], outs["contiguous"][short])


@pytest.mark.parametrize("k", [10, 20, 32, 64, 128])
def test_unforced_plan(cfk, k):
    """Path 3: no knob. 77,143 entries keep the chunk at its 1024-entry floor, so the ten rows of >= 1025 entries are
    the only split rows; k = 10 / 20 on the VALU Gram, 32 on the split-bf16 Gram without entry space, 64 / 128 on the
    pre-split Gram."""
    lad = _ladder()
    exp = _expected_plan(lad.degs, k, "f32", {})
    assert exp["chunk"] == 1024 and exp["n_reduce"] == 10 == int((lad.degs >= 1025).sum())
    assert [d for d, kd in zip(lad.degs, exp["kinds"]) if kd.startswith("split")] == [d for d in rs.LONG_DEGS if d > 1024]
    _run_case(cfk, k, "f32", {})


@pytest.mark.parametrize("k,precision,env", [(10, "f64", {"ALS_CHUNK": "64"}), (64, "f64", {"ALS_CHUNK": "64"}),
                                             (130, "f64", {}), (130, "f32", {})])
def test_f64_and_generic_paths(cfk, k, precision, env):
    """Path 4: fp64 split rows at 1e-8 per row; k = 130 on the generic path (one workgroup per whole row of any
    length: no REDUCE task) in both precisions."""
    exp = _expected_plan(_ladder().degs, k, precision, env)
    assert exp["n_reduce"] == (0 if k == 130 else 278) and exp["gram_path"] == ("generic" if k == 130 else "valu")
    _run_case(cfk, k, precision, env)


@pytest.mark.parametrize("k", [64, 128])
def test_lambda_one(cfk, k):
    """Path 5: lambda = 1 on the split path: a REDUCE task regularises with lambda x the WHOLE row's degree, not its
    last chunk's."""
    _run_case(cfk, k, "f32", {"ALS_CHUNK": "64"}, lam=1.0)


@pytest.mark.parametrize("sort_cols", [True, False], ids=["sorted", "arrival"])
def test_device_block_build(cfk, sort_cols):
    """Path 6: the interleaved XCD-range plan at k = 64 from arrival-order COO (als_set_block_coo): the same plan and
    bitwise the same output as the host-built block."""
    env = {"ALS_CHUNK": "64", "ALS_INTERLEAVE": "1", "ALS_XCD_RANGES": "1"}
    host, host_stats = _run_case(cfk, 64, "f32", env, sort_cols=sort_cols, label="host build")
    dev, dev_stats = _run_case(cfk, 64, "f32", env, sort_cols=sort_cols, coo=True, label="device build")
    assert host_stats == dev_stats
    assert np.array_equal(host, dev), np.nonzero(np.any(host != dev, axis=1))[0][:8]


def test_chunked_half_with_split_rows(cfk):
    """Path 7: als_set_chunks / als_solve_half_chunk over row ranges with an empty chunk, a cut between two rows of
    4 slots (200 | 201 entries) and one between two long rows (2047 | 2048): every chunk launches its own PARTIAL and
    REDUCE tasks, and together they are bitwise als_solve_half."""
    env = {"ALS_CHUNK": "64"}
    lad = _ladder()
    F, ref64, ref32 = _inputs(64, LAM, True)
    whole, _ = _run_case(cfk, 64, "f32", env, side=1)
    n = lad.blk["n_rows"]
    bounds = [0, 50, 50, 200, 338, n]
    assert lad.degs[199] == 200 and lad.degs[200] == 201 and lad.degs[337] == 2047 and lad.degs[338] == 2048
    eng = _engine(cfk, lad, 64, "f32", env, side=1)
    try:
        eng.write_factors(0, F)
        eng.set_chunks(1, bounds)
        for c in range(len(bounds) - 1):
            eng.solve_half_chunk(1, LAM, c)
        got = eng.read_factors(1, 0, n)
        assert eng.integrity_status() == [0, 0, 0, 0]
    finally:
        eng.close()
    rs.check_rows(got, ref64, ref32, lad.degs, "f32", rs.task_kinds(lad.degs, 64, 64))
    assert np.array_equal(got, whole), np.nonzero(np.any(got != whole, axis=1))[0][:8]
