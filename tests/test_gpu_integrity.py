"""GPU: the split-row hand-off check (PARTIAL -> REDUCE partial slots) and the reference's full rating range.

- Every partial slot is stored keyed by its launch generation with a check word (SlotCodec, als_slots.h);
  a REDUCE task that reads a slot its PARTIAL task's writes have not reached -- including a slot left over
  from an earlier launch with identical numbers -- fails the check and the engine's next synchronising call
  returns ALS_ERR_INTEGRITY.
- Ratings are Java shorts (Short.parseShort, NetflixDataFormatProducer.java:50; (float) of the short,
  MFeatureCalculator.java:80): every Gram path must be exact for |r| up to 32768, not only for 1..5.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LAM = 0.05


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _engine(cfk, k, precision, side, blk, n_opp, opp_f):
    eng = cfk.ALSEngine(k, precision)
    eng.alloc_factors(1 - side, n_opp)
    eng.alloc_factors(side, max(1, blk["n_rows"]))
    eng.set_block(side, blk["row_ptr"], blk["col"], blk["ratings"], 0, n_opp)
    eng.write_factors(1 - side, opp_f)
    return eng


def _split_row_data(cfk, oracle_mod, ratings=None, seed=3):
    ds = cfk.Dataset.synthetic_netflix(n_users=2000, n_movies=150, nnz=60_000, seed=seed, nthreads=8)
    m, u, r = ds.ratings()
    if ratings is not None:
        r = np.random.default_rng(seed).choice(np.asarray(ratings, np.int16), size=len(r))
        ds = cfk.Dataset.from_ratings(m, u, r)
    return ds, oracle_mod.build_blocks(m, u, r)


def test_integrity_clean_on_split_rows(cfk, oracle_mod, monkeypatch):
    """Split rows (chunk 64: every movie row of degree > 64 becomes PARTIAL tasks + a REDUCE task), repeated
    halves: no slot ever fails its check, and the record is readable."""
    monkeypatch.setenv("ALS_CHUNK", "64")
    ds, b = _split_row_data(cfk, oracle_mod)
    for k, prec in ((64, "f32"), (128, "f32"), (10, "f64")):
        F = np.random.default_rng(1).random((len(b.user.ids), k))
        F = F.astype(np.float32 if prec == "f32" else np.float64)
        eng = _engine(cfk, k, prec, 0, ds.shard_block(0), len(b.user.ids), F)
        assert eng.block_stats(0)["n_reduce"] > 0
        for _ in range(5):
            eng.solve_half(0, LAM)
        eng.synchronize()
        assert eng.integrity_status() == [0, 0, 0, 0]
        eng.close()


def test_integrity_check_catches_foreign_slots():
    """Fault injection: the REDUCE launch decodes with another launch's generation (ALS_DEBUG_REDUCE_GEN_SKEW),
    which is exactly what a slot still holding an earlier launch's sums looks like. Every such read must be
    caught, reported with its slot and row, and cleared by a reset. The knob exists only in the debug build
    (CFK_DEBUG_KNOBS), so the cases run in a child process on build_debug/libcfk_als.so
    (tests/integrity_fault_injection.py); the product library cannot be told to skew."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, ALS_CHUNK="64", ALS_DEBUG_REDUCE_GEN_SKEW="1",
               CFK_ALS_LIB=os.path.join(ROOT, "collaborative-filtering-kafka_amd", "build_debug", "libcfk_als.so"))
    res = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "integrity_fault_injection.py")],
                         env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    cases = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
    assert len(cases) == 4, res.stdout
    for c in cases:
        st, rec = c["stats"], c["rec"]
        assert c["raised"] and "ALS_ERR_INTEGRITY" in c["raised"], c
        # every REDUCE task fails (the record counts failing REDUCE tasks)
        n_slots = st["n_tasks"] - (c["n_movies"] - st["n_reduce"])
        assert rec[0] == st["n_reduce"] > 0, c
        assert rec[2] < n_slots and rec[3] < c["n_movies"], c
        assert c["after"] == [0, 0, 0, 0], c


def test_product_library_has_no_debug_knobs():
    """The work-dropping and integrity-weakening knobs compile into the debug build only."""
    import os
    from conftest import ROOT
    blob = open(os.path.join(ROOT, "collaborative-filtering-kafka_amd", "build", "libcfk_als.so"), "rb").read()
    assert b"ALS_DEBUG_" not in blob
    dbg = open(os.path.join(ROOT, "collaborative-filtering-kafka_amd", "build_debug", "libcfk_als.so"), "rb").read()
    assert b"ALS_DEBUG_REDUCE_GEN_SKEW" in dbg and b"ALS_DEBUG_SKIP_SOLVE" in dbg


def _check_vs_oracle(got32, ref, ref32):
    """test_gpu_parity.test_one_half_every_k_vs_oracle's bar: within the reference's own fp32 envelope."""
    norm = np.linalg.norm(ref, axis=1)
    zero = norm == 0                      # every rating of the row is 0: the solution is exactly 0
    assert np.all(got32[zero] == 0)
    got32, ref, ref32, norm = got32[~zero], ref[~zero], ref32[~zero], norm[~zero]
    rel = np.linalg.norm(got32 - ref, axis=1) / norm
    rel_ref = np.linalg.norm(ref32 - ref, axis=1) / norm
    assert np.percentile(rel, 99) <= max(2 * np.percentile(rel_ref, 99), 2e-5), (np.percentile(rel, 99),)
    assert rel.max() <= max(3 * rel_ref.max(), 1e-4), (rel.max(), rel_ref.max())


@pytest.mark.parametrize("k", [64, 128])
@pytest.mark.parametrize("presplit_env", [None, "1", "0"])
def test_extreme_short_ratings_every_path(cfk, oracle_mod, monkeypatch, k, presplit_env):
    """Ratings from {-32768, -1, 0, 257, 32767} (257 and 32767 are neither bf16 nor fp16 numbers): both halves at
    k = 64 and 128 against the fp64 oracle. The pre-split Gram (default at KP = 64 and 128) feeds them to its RHS
    MFMAs as rh + rm fp16 pairs (exact for every Java short); ALS_PRESPLIT=0 takes the on-the-fly bf16 split with
    its fp32 VALU RHS."""
    if presplit_env is not None:
        monkeypatch.setenv("ALS_PRESPLIT", presplit_env)
    ds, b = _split_row_data(cfk, oracle_mod, ratings=[-32768, -1, 0, 257, 32767], seed=5)
    rng = np.random.default_rng(k)
    for side, rows, opp in ((0, b.movie, b.user), (1, b.user, b.movie)):
        F = rng.random((len(opp.ids), k))
        ref = oracle_mod.update_side(rows, F, LAM, "f64")
        ref32 = oracle_mod.update_side(rows, F.astype(np.float32), LAM, "f32")
        eng = _engine(cfk, k, "f32", side, ds.shard_block(side), len(opp.ids), F.astype(np.float32))
        assert eng.block_path(side)["presplit"] == (presplit_env != "0")
        eng.solve_half(side, LAM)
        got = eng.read_factors(side)
        eng.close()
        _check_vs_oracle(got, ref, ref32)


@pytest.mark.parametrize("scale", [1e-20, 1e-6, 1.0, 3e4, 1e12])
def test_presplit_scale_extreme_factor_magnitudes(cfk, oracle_mod, scale):
    """The fp16 pre-split scales each opposite table by 2^s from its largest |x| (als_absmax, split_exp): tables of
    any magnitude whose Gram fits fp32 -- far below the fp16 range, far beyond its 65504 maximum -- stay within the
    fp32 envelope, both halves, k = 64 and 128. Above scale 1, lambda grows with scale^2 so the systems keep their
    conditioning (with lambda fixed, a 3e4-scaled table makes every short row's system singular in fp32 -- the
    reference's own fp32 solve returns NaN there); below, lambda n I dominates anyway."""
    ds, b = _split_row_data(cfk, oracle_mod, seed=7)
    lam = float(np.float32(LAM * max(1.0, scale) ** 2))
    for k in (64, 128):
        rng = np.random.default_rng(k)
        for side, rows, opp in ((0, b.movie, b.user), (1, b.user, b.movie)):
            F = rng.standard_normal((len(opp.ids), k)) * scale
            ref = oracle_mod.update_side(rows, F, lam, "f64")
            ref32 = oracle_mod.update_side(rows, F.astype(np.float32), lam, "f32")
            assert np.all(np.isfinite(ref32))
            eng = _engine(cfk, k, "f32", side, ds.shard_block(side), len(opp.ids), F.astype(np.float32))
            assert eng.block_path(side)["presplit"]
            eng.solve_half(side, lam)
            got = eng.read_factors(side)
            eng.close()
            assert np.all(np.isfinite(got))
            _check_vs_oracle(got, ref, ref32)


@pytest.mark.parametrize("k", [64, 128])
def test_presplit_range_guard(cfk, oracle_mod, monkeypatch, k):
    """The fp16 pre-split uses one scale per table (split_exp): values far below the table's largest |x| lose
    precision toward the fp16 subnormal floor. als_absmax also records the smallest nonzero row maximum; when the
    table's rows span more than 2^16 (PRESPLIT_RANGE) the pre-split launch stands down and its guarded on-the-fly
    launch (three-term bf16 split of the fp32 rows, an 8-bit exponent per value) solves the half.
    - Row norms spanning 2^-24..1, both halves: within the reference's fp32 envelope, and bitwise the result of the
      on-the-fly path (ALS_PRESPLIT=0), i.e. the guard fired.
    - Columns of very unequal size (a mean-rating-sized column 0, the others ~1e-5 of it) keep every row's maximum in
      range: the pre-split serves the half (not bitwise the on-the-fly result) and stays within the envelope."""
    ds, b = _split_row_data(cfk, oracle_mod, seed=9)
    rng = np.random.default_rng(k + 1)
    for case in ("row_norms", "columns"):
        for side, rows, opp in ((0, b.movie, b.user), (1, b.user, b.movie)):
            n = len(opp.ids)
            if case == "row_norms":
                F = rng.random((n, k)) * 2.0 ** -rng.uniform(0, 24, size=(n, 1))
                F[0] *= 1.0 / F[0].max()                # the extremes present: one row at 1 ...
                F[1] *= 2.0 ** -24 / F[1].max()         # ... and one at 2^-24
            else:
                F = rng.random((n, k)) * 1e-5
                F[:, 0] = 3.0 + rng.random(n)
            F = F.astype(np.float32)
            ref = oracle_mod.update_side(rows, F.astype(np.float64), LAM, "f64")
            ref32 = oracle_mod.update_side(rows, F, LAM, "f32")
            out = {}
            for ps in ("1", "0"):
                monkeypatch.setenv("ALS_PRESPLIT", ps)
                eng = _engine(cfk, k, "f32", side, ds.shard_block(side), n, F)
                assert eng.block_path(side)["presplit"] == (ps == "1")
                eng.solve_half(side, LAM)
                out[ps] = eng.read_factors(side)
                eng.close()
            monkeypatch.delenv("ALS_PRESPLIT")
            assert np.all(np.isfinite(out["1"]))
            _check_vs_oracle(out["1"], ref, ref32)
            assert np.array_equal(out["1"], out["0"]) == (case == "row_norms"), (case, side)
