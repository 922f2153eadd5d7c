"""Every solve path across conditioning and the refinement gate of the tile solve (tests/conditioning.py).

One 79-row block (degrees 1..330 and an empty row, 64-entry chunk: entry-space, FULL and PARTIAL + REDUCE tasks) is
uploaded once per engine and solved for two factor families over a ladder of lambdas: `signed` (small pivots from rank
deficiency) and `offset` (every row shares a direction: small pivots on every row, the entry-space system below the
gate), condition numbers up to ~3e3, rows on both sides of the 0.45 gate and next to it. Every solve asserts
conditioning.check_case -- per row within max(1e-4, 3 x the worst row of the reference's own fp32 arithmetic in the same
pivot bucket of the same case), the empty row exactly zero, the median within 2 x the reference's -- a clean integrity
record and als_sq_error against the oracle's. test_conditioning_host.py proves on the CPU that this bar rejects a block
that differs by one entry in any row with a margin of 3 bounds, and that the inputs populate both sides of the gate.

- fp32 MFMA tile solve, all three residual implementations of its refinement step and the entry-space instantiation:
  the pre-split Gram (RowResidual; split rows' REDUCE tasks keep a register copy), ALS_PRESPLIT=0 (RegStore at KP = 64,
  the LDS working tiles at KP = 128), ALS_GRAM=f32, ALS_DUAL=0, and k = 32 / 40. Each also with ALS_REFINE_MIN_PIVOT=2
  (every row refines): within the same bounds, bitwise the default run on every row below the gate.
- the paths without a gate, largest and smallest lambda: VALU Cholesky (k = 10, 20), fp64 (k = 10, 64), generic (130).
- the gate is where the code says it is: with the refinement step compiled out of reach below the gate
  (ALS_DEBUG_SKIP_REFINE, debug build, tests/conditioning_skip_refine.py) no row above the gate changes and every row
  below it does.

Largest per-row error measured on an MI355X per pivot bucket, over the families and lambdas of each path, next to the
reference's own fp32 arithmetic (oracle, f32 mode) on the same rows; `unrefined` is the debug build without the
refinement step (recorded, not asserted: it comes from the code under test):

    pivot bucket                        [0.45, 1] [0.3, 0.45) [0.1, 0.3) [0.03, 0.1) [0.01, 0.03)
    k = 64  pre-split (default)          4.7e-06   4.8e-06    6.0e-06    1.3e-06     2.1e-07
    k = 64  ALS_PRESPLIT=0               4.7e-06   4.2e-06    5.7e-06    1.3e-06     2.1e-07
    k = 64  ALS_GRAM=f32                 5.2e-06   4.4e-06    1.3e-05    2.2e-05     3.5e-05
    k = 64  ALS_DUAL=0                   4.7e-06   5.2e-06    1.6e-05    3.2e-05     3.6e-05
    k = 64  default, unrefined           5.3e-06   1.2e-05    4.2e-05    2.5e-06     2.1e-07
    k = 64  reference fp32               1.5e-05   2.2e-05    2.4e-04    4.9e-04     3.0e-04
    k = 128 pre-split (default)          6.1e-06   5.5e-06    5.9e-06    5.4e-07        -
    k = 128 ALS_PRESPLIT=0               6.0e-06   5.8e-06    5.4e-06    5.4e-07        -
    k = 128 ALS_GRAM=f32                 5.4e-06   6.2e-06    2.1e-05    2.1e-05        -
    k = 128 ALS_DUAL=0                   6.1e-06   8.4e-06    2.4e-05    2.9e-05        -
    k = 128 default, unrefined           8.9e-06   1.4e-05    2.1e-05    4.0e-07        -
    k = 128 reference fp32               2.3e-05   3.5e-05    1.8e-04    7.6e-04        -
    k = 32  on-the-fly split Gram        4.1e-06   3.4e-06    7.6e-06    2.0e-05     2.9e-05
    k = 32  reference fp32               8.5e-06   1.5e-05    6.0e-05    1.7e-04     7.6e-04
    k = 40  pre-split (default)          2.8e-06   3.7e-06    6.0e-06    3.5e-06     2.0e-07
    k = 40  reference fp32               1.0e-05   1.8e-05    9.5e-05    4.1e-04     4.7e-04
    k = 10  VALU Cholesky                2.6e-06   1.4e-06    7.5e-06    8.2e-06     2.0e-05
    k = 10  reference fp32               4.7e-06   2.5e-06    1.5e-05    3.5e-05     8.6e-05
    k = 20  VALU Cholesky                3.0e-06   2.2e-06    8.8e-06    1.2e-05     1.6e-05
    k = 20  reference fp32               6.5e-06   3.8e-06    1.7e-05    6.2e-05     1.7e-04
    k = 130 generic                      4.8e-06   2.4e-05    1.3e-05    2.5e-05        -
    k = 130 reference fp32               7.4e-06   3.3e-05    2.6e-04    1.5e-03        -
    k = 10  VALU Cholesky fp64           3.6e-15   4.3e-15    1.5e-14    7.8e-14     3.3e-13
    k = 64  VALU Cholesky fp64           1.0e-14   1.2e-14    1.2e-13    6.5e-13     5.9e-13
    k = 130 generic fp64                 1.3e-14   4.9e-14    5.7e-13    1.3e-12        -

(The rows of a default-knob line include the run that refines every row; the lowest buckets hold short rows, which the
default plan solves in entry space -- hence its small errors there against ALS_DUAL=0 and ALS_GRAM=f32.) Every path,
the fp32 Cholesky paths without a refinement step included, stays 1.3x to over 1000x below the reference's own fp32 LU
in every bucket; no bound had to move and no kernel changed. What the refinement step buys at k = 64 is 6.0e-06 against
4.2e-05 in the [0.1, 0.3) bucket (2.5x in [0.3, 0.45)), at k = 128 5.9e-06 against 2.1e-05. The unrefined solve still
lies 6x below the reference, so the per-bucket bar does NOT reject a solve without the refinement step (0 of 1264
unrefined rows beyond their bound): that the step runs where it should, and only there, is held by the bitwise
assertions of this module, not by the error bar.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conditioning as cd
import rowshapes as rs
from test_gpu_rowshapes import _assert_plan, _expected_plan

pytestmark = pytest.mark.gpu

BASE = {"ALS_CHUNK": str(cd.CHUNK)}
ALWAYS = {"ALS_REFINE_MIN_PIVOT": "2"}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _engine(cfk, k, precision, env):
    """An engine under `env` with the block uploaded once (side 0; the opposite table is side 1)."""
    lad = cd.block()
    with rs.knobs(env):
        eng = cfk.ALSEngine(k, precision)
    eng.use_torch_stream()
    eng.alloc_factors(1, lad.n_opp)
    eng.alloc_factors(0, lad.blk["n_rows"])
    eng.set_block(0, lad.blk["row_ptr"], lad.blk["col"], lad.blk["ratings"], 0, lad.n_opp)
    return eng


def _solve(eng, c, precision, kinds):
    """write_factors + solve_half of one case with every assertion of this module; returns (output, per-row errors)."""
    lad = cd.block()
    eng.write_factors(1, c.F)
    eng.solve_half(0, c.lam)
    got = eng.read_factors(0, 0, lad.blk["n_rows"])
    rel = cd.check_case(got, c, precision, kinds)
    assert eng.integrity_status() == [0, 0, 0, 0]
    se, cnt = eng.sq_error(0)
    se_o, cnt_o = rs.oracle.sq_error(lad.side, got.astype(np.float64), c.F)
    assert cnt == cnt_o == int(lad.degs.sum())
    assert se == pytest.approx(se_o, rel=1e-5 if precision == "f32" else 1e-12)
    return got, rel


def _record(label, k, precision, worst_gpu, worst_ref):
    print(f"\nRECORD {json.dumps({'path': label, 'k': k, 'precision': precision, 'gpu': worst_gpu, 'ref': worst_ref})}")


def _fmt(v):
    return "[" + ", ".join(f"{x:.1e}" if x else "-" for x in v) + "]"


MFMA = [(k, extra) for extra in ({}, {"ALS_PRESPLIT": "0"}, {"ALS_GRAM": "f32"}, {"ALS_DUAL": "0"})
        for k in (64, 128)] + [(32, {}), (40, {})]


def _id(v):
    return (" ".join(f"{n[4:]}={x}" for n, x in v.items()) or "default") if isinstance(v, dict) else None


@pytest.mark.parametrize("k,extra", MFMA, ids=_id)
def test_mfma_tile_solve(cfk, k, extra):
    """The fp32 tile solve under `extra`, once at the product gate and once refining every row."""
    env = {**BASE, **extra}
    degs = cd.block().degs
    exp = _expected_plan(degs, k, "f32", env)
    kinds = exp["kinds"]
    # the path the case is about: the Gram, the pre-split (RowResidual) or a kept copy, entry space on or off
    assert exp["gram_path"] == ("mfma_f32" if "ALS_GRAM" in extra else "mfma_split")
    assert exp["presplit"] == (cd.padded_k(k) >= 64 and extra.get("ALS_PRESPLIT") != "0" and "ALS_GRAM" not in extra)
    assert (exp["dual_rows"] > 0) == (k != 32 and extra in ({}, {"ALS_PRESPLIT": "0"}))
    assert exp["n_reduce"] == int((degs > cd.CHUNK).sum()) == 31 and exp["chunk"] == cd.CHUNK
    assert ("FULL" in kinds) == (not (k == 128 and exp["dual_rows"]))
    gate_eng, all_eng = _engine(cfk, k, "f32", env), _engine(cfk, k, "f32", {**env, **ALWAYS})
    worst_gpu, worst_ref = np.zeros(5), np.zeros(5)
    try:
        for eng in (gate_eng, all_eng):
            _assert_plan(eng, 0, exp)
        for family in cd.FAMILIES:
            for lam in cd.lambdas(k, family):
                c = cd.case(k, family, lam)
                got, rel = _solve(gate_eng, c, "f32", kinds)
                got_all, rel_all = _solve(all_eng, c, "f32", kinds)
                # both runs refine a row below the gate: bitwise equal (the band round the gate is exempt: the
                # kernel's pivots are fp32); above it they may differ, each within the row's bound (_solve)
                gp = cd.gate_pivots(c, kinds)
                below = gp < cd.GATE - cd.GATE_BAND
                same = np.all(got == got_all, axis=1)
                assert same[below].all(), (family, lam, np.nonzero(below & ~same)[0][:8], gp[below & ~same][:8])
                ref = cd.bucket_worst(rs.row_errors(c.ref32, c.ref64), c.bucket)
                gpu, gpu_all = cd.bucket_worst(rel, c.bucket), cd.bucket_worst(rel_all, c.bucket)
                print(f"\n[k={k} {_id(extra)}] {family} lam={lam}: {int(below.sum())} rows below the gate, "
                      f"{int((gp > cd.GATE + cd.GATE_BAND).sum())} above ({int((~same).sum())} differ when all "
                      f"refine); per bucket GPU {_fmt(gpu)} all-refine {_fmt(gpu_all)} reference fp32 {_fmt(ref)}")
                worst_gpu = np.maximum(worst_gpu, np.maximum(gpu, gpu_all))
                worst_ref = np.maximum(worst_ref, ref)
    finally:
        gate_eng.close()
        all_eng.close()
    _record(_id(extra), k, "f32", worst_gpu.tolist(), worst_ref.tolist())


@pytest.mark.parametrize("precision,k", cd.UNGATED, ids=str)
def test_paths_without_a_gate(cfk, precision, k):
    """VALU Cholesky (fp32 k = 10 / 20, fp64 k = 10 / 64; split rows summed by REDUCE tasks) and the generic
    workgroup Cholesky (k = 130, whole rows), largest and smallest lambda of each family: fp32 has no refinement
    here at all, so the per-bucket bound is all that stands between these paths and cond * eps."""
    env = dict(BASE) if k <= 64 else {}
    degs = cd.block().degs
    exp = _expected_plan(degs, k, precision, env)
    assert exp["gram_path"] == ("generic" if k == 130 else "valu") and exp["dual_rows"] == 0
    assert exp["n_reduce"] == (0 if k == 130 else 31)
    eng = _engine(cfk, k, precision, env)
    worst_gpu, worst_ref = np.zeros(5), np.zeros(5)
    try:
        _assert_plan(eng, 0, exp)
        for family in cd.FAMILIES:
            for lam in cd.ungated_lambdas(k, family):
                c = cd.case(k, family, lam)
                _, rel = _solve(eng, c, precision, exp["kinds"])
                ref = cd.bucket_worst(rs.row_errors(c.ref32, c.ref64), c.bucket)
                gpu = cd.bucket_worst(rel, c.bucket)
                print(f"\n[k={k} {precision}] {family} lam={lam}: per bucket GPU {_fmt(gpu)} reference fp32 "
                      f"{_fmt(ref)}")
                worst_gpu, worst_ref = np.maximum(worst_gpu, gpu), np.maximum(worst_ref, ref)
    finally:
        eng.close()
    _record("valu" if k < 130 else "generic", k, precision, worst_gpu.tolist(), worst_ref.tolist())


def _backward_error(c, i, x):
    """Normwise backward error, in fp64, of x as the solution of row i's system (Y^T Y + lambda n I) x = Y^T r."""
    side = cd.block().side
    lo, hi = side.row_ptr[i], side.row_ptr[i + 1]
    Y, r = c.F[side.col[lo:hi]], side.ratings[lo:hi].astype(np.float64)
    A = Y.T @ Y + float(np.float32(c.lam)) * (hi - lo) * np.eye(c.k)
    b = Y.T @ r
    return float(np.linalg.norm(b - A @ x) / (np.linalg.norm(A, 2) * np.linalg.norm(x) + np.linalg.norm(b)))


def test_the_gate_is_where_the_code_says(cfk):
    """k = 64 and 128, default knobs, solved by the debug build with and without its refinement step
    (tests/conditioning_skip_refine.py, one child process). The flag is read below the gate only, so (a) no row whose
    fp64 pivot -- the dual one for entry-space rows -- is above 0.46 changes, and (b) every row below 0.44 changes in
    at least one component; rows within 0.01 of the gate are exempt (the kernel's pivots are fp32). On an MI355X
    3 of the 391 rows below the gate do not change, all entry-space rows of 2 entries on `offset` (k = 64: lambda 0.04
    and 0.012, dual pivots 0.41 and 0.35; k = 128: lambda 0.01, 0.35). Their unrefined solution was not the correctly
    rounded one (per-row error 2.1e-07 .. 3.9e-07 against 3.5e-08 for a correctly rounded entry-space solution), but
    neither is that of their 2-entry neighbours the step does change (2.7e-07): what is left is the rounding of the
    fp32 Gram entries, which a residual against that same Gram cannot see, and the 2 x 2 solve itself leaves a
    correction below half a unit in the last place. The test therefore accepts an unchanged row only when, in fp64,
    its normwise backward error is at most 2^-23 -- already converged in fp32, nothing for the step to give (the
    three rows: 1.2 .. 1.7 x 2^-24; refined rows reach 3.6 x 2^-24) -- and only for a few rows (<= 2 %); an unrefined
    row the gate wrongly let through would carry the block inverses' error and fail it. (c) The unrefined
    errors per bucket are printed for the record in this module's docstring, not asserted."""
    from conftest import ROOT
    env = dict(os.environ, CFK_ALS_LIB=os.path.join(ROOT, "collaborative-filtering-kafka_amd", "build_debug",
                                                    "libcfk_als.so"))
    env.pop("ALS_DEBUG_SKIP_REFINE", None)
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "conditioning_skip_refine.py")],
                         env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    cases = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
    assert [(c["k"], c["family"], c["lam"]) for c in cases] == \
        [(k, f, lam) for k in (64, 128) for f in cd.FAMILIES for lam in cd.lambdas(k, f)]
    degs = cd.block().degs
    n_above = n_below = 0
    stuck = []      # rows below the gate that the refinement step left bitwise unchanged
    for k in (64, 128):
        kinds = cd.kinds_of(k)
        worst = {"refined": np.zeros(5), "unrefined": np.zeros(5), "ref": np.zeros(5)}
        for j in (j for j in cases if j["k"] == k):
            assert j["path"]["gram_path"] == "mfma_split" and j["path"]["presplit"] and j["path"]["dual_rows"] > 0
            c = cd.case(k, j["family"], j["lam"])
            gp = cd.gate_pivots(c, kinds)
            differ = np.asarray(j["differ"])
            above, below = gp > cd.GATE + cd.GATE_BAND, gp < cd.GATE - cd.GATE_BAND
            n_above, n_below = n_above + int(above.sum()), n_below + int(below.sum())
            assert not differ[above].any(), (k, j["family"], j["lam"], np.nonzero(above & differ)[0][:8],
                                             gp[above & differ][:8])
            # (b), the fp64 check of a row the step left unchanged: was there anything to refine? A solution whose
            # normwise backward error is within one fp32 unit in the last place solves a system no further from
            # the true one than storing its entries in fp32 puts it; a refinement step in fp32 cannot improve on it.
            assert sorted(int(i) for i in j["unchanged_below"]) == np.nonzero(below & ~differ)[0].tolist()
            for i, x in j["unchanged_below"].items():
                i = int(i)
                eta = _backward_error(c, i, np.asarray(x, np.float64))
                stuck.append((k, j["family"], j["lam"], i, int(degs[i]), kinds[i], round(float(gp[i]), 4),
                              f"err {j['unrefined'][i]:.2e}", f"backward error {eta / 2.0 ** -24:.2f} x 2^-24"))
                assert eta <= 2.0 ** -23, stuck[-1]
            assert not differ[degs == 0].any()
            rel = {name: np.asarray(j[name]) for name in ("refined", "unrefined")}
            rel["ref"] = rs.row_errors(c.ref32, c.ref64)
            out = ~(rel["unrefined"] <= cd.bounds(c, "f32"))
            print(f"\n[k={k}] {j['family']} lam={j['lam']}: {int(below.sum())} rows below the gate; per bucket "
                  f"refined {_fmt(cd.bucket_worst(rel['refined'], c.bucket))} unrefined "
                  f"{_fmt(cd.bucket_worst(rel['unrefined'], c.bucket))}; the bar rejects {int(out.sum())} of them")
            for name in worst:
                worst[name] = np.maximum(worst[name], cd.bucket_worst(rel[name], c.bucket))
        _record("debug build refined", k, "f32", worst["refined"].tolist(), worst["ref"].tolist())
        _record("debug build unrefined", k, "f32", worst["unrefined"].tolist(), worst["ref"].tolist())
    assert n_above >= 100 and n_below >= 100, (n_above, n_below)
    print(f"\nrows below the gate unchanged by the refinement step, each already converged in fp32: {stuck}")
    assert len(stuck) <= 0.02 * n_below, stuck
