"""GPU parity: libcfk_als.so on cuda:0 against the CPU oracle and the committed golden fixtures.

Tolerances (BASELINE.json north star): fp64 parity mode -> factor max-relative error <= 1e-6 (denominator
floor max(|x|, 1e-12*||row||)) and MSE relative <= 1e-6; fp32 fast mode -> MSE delta <= 1e-3.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, max_rel

pytestmark = pytest.mark.gpu

LAM = 0.05


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"{name}_k10_n10_p4_seed42_f64.npz"))


@pytest.mark.parametrize("name,nm,nu", [("tiny", 426, 302), ("medium", 3590, 2120)])
def test_f64_parity_vs_golden(cfk, name, nm, nu):
    """BASELINE configs[0]/[1]: k=10, lambda=0.05, 10 iterations, 4 partitions, fp64 parity mode."""
    ds = cfk.Dataset.load_netflix(os.path.join(GOLDEN, f"data_sample_{name}.txt"))
    app = cfk.ALSApp(4, 10, LAM, 10, nm, nu, precision="f64", seed=42).setup(ds)
    app.run()
    U, M = app.factors()
    g = _golden(name)
    assert max_rel(U, g["U"]) <= 1e-6
    assert max_rel(M, g["M"]) <= 1e-6
    assert abs(app.mse() - float(g["mse"])) / float(g["mse"]) <= 1e-6


@pytest.mark.parametrize("name,nm,nu", [("tiny", 426, 302), ("medium", 3590, 2120)])
def test_f32_fast_mode_mse_delta(cfk, name, nm, nu):
    ds = cfk.Dataset.load_netflix(os.path.join(GOLDEN, f"data_sample_{name}.txt"))
    app = cfk.ALSApp(4, 10, LAM, 10, nm, nu, precision="f32", seed=42).setup(ds)
    app.run()
    g = _golden(name)
    assert abs(app.mse() - float(g["mse"])) <= 1e-3
    U, M = app.factors()
    assert np.linalg.norm(U - g["U"]) / np.linalg.norm(g["U"]) < 1e-3


def _one_half(cfk, side, blk, opp_f, k, precision, opp_rows):
    eng = cfk.ALSEngine(k, precision)
    eng.use_torch_stream()
    eng.alloc_factors(1 - side, opp_rows)
    eng.alloc_factors(side, max(1, blk["n_rows"]))
    eng.set_block(side, blk["row_ptr"], blk["col"], blk["ratings"], 0, opp_rows)
    eng.write_factors(1 - side, opp_f)
    eng.solve_half(side, LAM)
    out = eng.read_factors(side, 0, blk["n_rows"])
    eng.close()
    return out


def test_known_answer_systems(cfk):
    import json
    for c in json.load(open(os.path.join(GOLDEN, "known_answers.json"))):
        n, k = c["n"], c["k"]
        blk = {"row_ptr": np.array([0, n]), "col": np.arange(n, dtype=np.int32), "ratings": np.array(c["r"], np.int16),
               "n_rows": 1}
        Y = np.asarray(c["Y"], np.float64)
        x64 = _one_half(cfk, 0, blk, Y, k, "f64", n)[0]
        np.testing.assert_allclose(x64, c["x"], rtol=1e-12, atol=1e-13)
        x32 = _one_half(cfk, 0, blk, Y.astype(np.float32), k, "f32", n)[0]
        np.testing.assert_allclose(x32, c["x"], rtol=3e-4, atol=3e-5)


def _synthetic(cfk, oracle_mod, n_users=3000, n_movies=400, nnz=90_000, seed=11):
    ds = cfk.Dataset.synthetic_netflix(n_users=n_users, n_movies=n_movies, nnz=nnz, seed=seed, nthreads=8)
    m, u, r = ds.ratings()
    return ds, oracle_mod.build_blocks(m, u, r)


def _exact_solution(rows, F, lam):
    """(Y^T Y + lambda n I)^{-1} Y^T r per row to ~extended precision: fp64 solves refined twice against residuals
    formed in long double from the rows themselves (b - Y^T (Y x) - lambda n x; no long-double Gram)."""
    ld = np.longdouble
    lam = ld(np.float64(np.float32(lam)))
    k = F.shape[1]
    out = np.zeros((len(rows.row_ptr) - 1, k), np.float64)
    for i in range(len(rows.row_ptr) - 1):
        lo, hi = rows.row_ptr[i], rows.row_ptr[i + 1]
        if hi == lo:
            continue
        Y = F[rows.col[lo:hi]].astype(np.float64)
        r = rows.ratings[lo:hi].astype(np.float64)
        A = Y.T @ Y + float(lam) * (hi - lo) * np.eye(k)
        YL, rL = Y.astype(ld), r.astype(ld)
        bL = YL.T @ rL
        x = np.linalg.solve(A, Y.T @ r).astype(ld)
        for _ in range(2):
            res = bL - YL.T @ (YL @ x) - lam * ld(hi - lo) * x
            x = x + np.linalg.solve(A, res.astype(np.float64)).astype(ld)
        out[i] = x.astype(np.float64)
    return out


@pytest.mark.parametrize("k", [1, 5, 10, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 127, 128, 129, 160, 256])
def test_one_half_every_k_vs_oracle(cfk, oracle_mod, k):
    """Both sides. f64 (VALU path k <= 64, generic workgroup path above) to 1e-7 max-rel. f32 (VALU k<32 / MFMA tile
    solve 32 <= k <= 128 / generic workgroup Cholesky k > 128, ALSAppRunner.java:18 takes any k) against the exact
    solution, held to the error envelope of the reference's OWN fp32 arithmetic on the same rows (the oracle's
    f32 mode restates EJML's fp32 LU): per-row norm-relative error p99 <= 2x and max <= 3x the reference's,
    with floors 2e-5 / 1e-4. The worst rows on both paths are users with one rating (A = y y^T + 0.05 I,
    condition number ~ k/0.15), where the reference itself is off by up to ~1e-3 at k = 64."""
    ds, b = _synthetic(cfk, oracle_mod)
    rng = np.random.default_rng(k)
    for side, rows, opp in ((0, b.movie, b.user), (1, b.user, b.movie)):
        blk = ds.shard_block(side)
        F = rng.random((len(opp.ids), k))
        ref = oracle_mod.update_side(rows, F, LAM, "f64")
        got64 = _one_half(cfk, side, blk, F, k, "f64", len(opp.ids))   # k > 64: the generic workgroup path
        rel64 = np.linalg.norm(got64 - ref, axis=1) / np.linalg.norm(ref, axis=1)
        if k <= 128:
            # 10x inside the 1e-6 north-star bar on the VALU path (k <= 64), the bar itself on the generic path
            assert max_rel(got64, ref) <= (1e-7 if k <= 64 else 1e-6), (side, k)
        else:
            # Beyond 128 the oracle's own fp64 (EJML LU) solution misses the 1e-6 bar on near-zero elements of these
            # wide solutions (max-rel 1.2e-6 at k = 129, 2.6e-6 at k = 256 against the extended-precision solution:
            # ~cond * eps of the row norm), so no fp64 result can be held to 1e-6 against it there. The generic
            # path (workgroup Cholesky + one fp64 refinement step) is held to the north-star bar against the exact
            # solution itself, and stays within 1e-5 of the oracle.
            ex = _exact_solution(rows, F, LAM)
            assert max_rel(got64, ex) <= 1e-6, (side, k, max_rel(got64, ex), max_rel(ref, ex))
            assert max_rel(got64, ref) <= 1e-5 and rel64.max() <= 1e-10, (side, k, rel64.max())
        got32 = _one_half(cfk, side, blk, F.astype(np.float32), k, "f32", len(opp.ids))
        ref32 = oracle_mod.update_side(rows, F.astype(np.float32), LAM, "f32")
        norm = np.linalg.norm(ref, axis=1)
        rel = np.linalg.norm(got32 - ref, axis=1) / norm
        rel_ref = np.linalg.norm(ref32 - ref, axis=1) / norm
        assert np.percentile(rel, 99) <= max(2 * np.percentile(rel_ref, 99), 2e-5), (side, k)
        assert rel.max() <= max(3 * rel_ref.max(), 1e-4), (side, k, rel.max(), rel_ref.max())


@pytest.mark.parametrize("chunk", ["4", "64", "256"])
def test_partial_reduce_split_rows(cfk, oracle_mod, monkeypatch, chunk):
    """Long rows split into PARTIAL chunks + a REDUCE task give the same solution."""
    monkeypatch.setenv("ALS_CHUNK", chunk)
    ds, b = _synthetic(cfk, oracle_mod, n_users=2000, n_movies=150, nnz=60_000, seed=3)
    for k, prec, tol in ((10, "f64", 1e-8), (64, "f64", 1e-8), (64, "f32", 1e-4), (32, "f32", 1e-4), (10, "f32", 1e-4),
                         (128, "f32", 1e-4)):
        F = np.random.default_rng(1).random((len(b.user.ids), k))
        ref = oracle_mod.update_side(b.movie, F, LAM, "f64")
        got = _one_half(cfk, 0, ds.shard_block(0), F.astype(np.float32 if prec == "f32" else np.float64), k, prec,
                        len(b.user.ids))
        rel = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
        assert rel.max() <= tol, (chunk, k, prec, rel.max())


def test_valu_and_mfma_paths_agree(cfk, oracle_mod, monkeypatch):
    ds, b = _synthetic(cfk, oracle_mod)
    F = np.random.default_rng(2).random((len(b.user.ids), 64)).astype(np.float32)
    mfma = _one_half(cfk, 0, ds.shard_block(0), F, 64, "f32", len(b.user.ids))
    monkeypatch.setenv("ALS_FORCE_VALU", "1")
    valu = _one_half(cfk, 0, ds.shard_block(0), F, 64, "f32", len(b.user.ids))
    assert np.linalg.norm(mfma - valu) / np.linalg.norm(valu) < 1e-4     # fp32 accumulation order differs


@pytest.mark.parametrize("k", [64, 128])
def test_full_run_f32_mse_vs_oracle(cfk, oracle_mod, k):
    """BASELINE configs[2]/[3] at test size: k = 64 and k = 128 (MFMA Gram path), 3 iterations, fp32 fast mode
    MSE delta <= 1e-3 against the fp64 oracle."""
    ds, b = _synthetic(cfk, oracle_mod)
    app = cfk.ALSApp(1, k, LAM, 3, precision="f32", seed=9).setup(ds)
    app.run()
    U, M = app.factors()
    Uo, Mo = oracle_mod.run_als(b, k, LAM, 3, seed=9, precision="f64")
    assert abs(app.mse() - oracle_mod.mse(b, Uo, Mo)) <= 1e-3
    se, cnt = app.sq_error()
    se_o, cnt_o = oracle_mod.sq_error(b.movie, M.astype(np.float64), U.astype(np.float64))
    assert cnt == cnt_o and se == pytest.approx(se_o, rel=1e-5)


def test_sq_error_reduction_f64(cfk, oracle_mod, tiny_path):
    ds = cfk.Dataset.load_netflix(tiny_path)
    app = cfk.ALSApp(4, 10, LAM, 2, precision="f64", seed=42).setup(ds)
    app.run()
    U, M = app.factors()
    m, u, r = oracle_mod.parse_netflix(tiny_path)
    b = oracle_mod.build_blocks(m, u, r)
    se_o, cnt_o = oracle_mod.sq_error(b.movie, M, U)
    for side in ("movie", "user"):
        se, cnt = app.engine.sq_error(side)
        assert cnt == cnt_o == 3415 and se == pytest.approx(se_o, rel=1e-12)


def test_deterministic_bitwise(cfk, tiny_path):
    outs = []
    for _ in range(2):
        ds = cfk.Dataset.load_netflix(tiny_path)
        app = cfk.ALSApp(4, 64, LAM, 3, precision="f32", seed=1).setup(ds)
        app.run()
        outs.append(app.factors())
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_edge_cases(cfk):
    # empty block: no-op
    eng = cfk.ALSEngine(16, "f32")
    eng.use_torch_stream()
    eng.alloc_factors(0, 1)
    eng.alloc_factors(1, 3)
    eng.set_block(0, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int16), 0, 3)
    eng.solve_half(0, LAM)
    eng.synchronize()
    # a zero-degree row (cannot occur in the reference) yields zeros; extreme short ratings stay finite
    eng.set_block(0, np.array([0, 0, 2], np.int64), np.array([1, 2], np.int32), np.array([-32768, 32767], np.int16), 0, 3)
    eng.alloc_factors(0, 2)
    eng.write_factors(1, np.ones((3, 16), np.float32))
    eng.solve_half(0, LAM)
    out = eng.read_factors(0)
    assert np.all(out[0] == 0) and np.all(np.isfinite(out[1]))
    # out-of-range column indices are rejected on the host (never reach the GPU)
    from cfk_amd._lib import ALSError
    with pytest.raises(ALSError, match="ALS_ERR_INVALID_ARGUMENT"):
        eng.set_block(0, np.array([0, 1], np.int64), np.array([3], np.int32), np.array([1], np.int16), 0, 3)
    with pytest.raises(ALSError, match="ALS_ERR_STATE"):
        eng2 = cfk.ALSEngine(16, "f32")
        eng2.solve_half(0, LAM)
    eng.close()


def test_cli_app_end_to_end(tmp_path, oracle_mod, tiny_path):
    """als_app (ALSAppRunner CLI) writes the prediction CSV; its MSE matches the f64 oracle run."""
    import subprocess
    from conftest import ROOT
    app = os.path.join(ROOT, "collaborative-filtering-kafka_amd", "build", "als_app")
    res = subprocess.run([app, "4", "10", "0.05", "10", tiny_path, "426", "302", "--precision", "f64", "--seed", "42",
                          "--out", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    csvs = list(tmp_path.glob("prediction_matrix_*"))
    assert len(csvs) == 1
    g = _golden("tiny")
    assert oracle_mod.mse_from_csv(tiny_path, str(csvs[0])) == pytest.approx(float(g["mse"]), rel=1e-6)
    res = subprocess.run([app, "4", "10", "0.05", "10", tiny_path, "1000", "302"], capture_output=True, text=True)
    assert res.returncode != 0 and "would wait forever" in res.stderr


def test_chunked_user_half_bitwise_equal(cfk, oracle_mod):
    """als_set_chunks / als_solve_half_chunk (the multi-GPU overlap path) reproduce als_solve_half exactly."""
    ds, b = _synthetic(cfk, oracle_mod)
    blk = ds.shard_block(1)
    F = np.random.default_rng(5).random((len(b.movie.ids), 64)).astype(np.float32)
    whole = _one_half(cfk, 1, blk, F, 64, "f32", len(b.movie.ids))
    eng = cfk.ALSEngine(64, "f32")
    eng.use_torch_stream()
    eng.alloc_factors(0, len(b.movie.ids))
    eng.alloc_factors(1, blk["n_rows"])
    eng.set_block(1, blk["row_ptr"], blk["col"], blk["ratings"], 0, len(b.movie.ids))
    eng.write_factors(0, F)
    n = blk["n_rows"]
    bounds = [0, n // 5, n // 5, n // 2, n]          # includes an empty chunk
    eng.set_chunks(1, bounds)
    for c in range(len(bounds) - 1):
        eng.solve_half_chunk(1, LAM, c)
    got = eng.read_factors(1, 0, n)
    eng.close()
    assert np.array_equal(got, whole)


def _gloo_gpu_worker(rank, world, port, path, out_dir):
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import __graft_entry__
    cfk = __graft_entry__.load_package()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ds = cfk.Dataset.load_netflix(path)
    app = cfk.ALSApp(4, 10, LAM, 10, 426, 302, precision="f64", seed=42, device=0, rank=rank, world_size=world,
                     overlap_chunks=3)
    app.setup(ds)
    app.run()
    U, M = app.factors()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), U=U, M=M, mse=app.mse())
    dist.destroy_process_group()


def test_sharded_two_ranks_on_one_gpu(tmp_path, tiny_path):
    """The real HIP engine under the sharded driver: 2 ranks (both on cuda:0; gloo carries the all-gathers of
    CUDA tensors, RCCL needs one GPU per rank) with the chunked user half -> the golden fp64 result."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_gloo_gpu_worker, args=(2, port, tiny_path, str(tmp_path)), nprocs=2, join=True)
    g = _golden("tiny")
    for rank in range(2):
        res = np.load(os.path.join(tmp_path, f"rank{rank}.npz"))
        assert max_rel(res["U"], g["U"]) <= 1e-6 and max_rel(res["M"], g["M"]) <= 1e-6
        assert abs(float(res["mse"]) - float(g["mse"])) / float(g["mse"]) <= 1e-6


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_gpu_collector_prediction_matrix(cfk, tiny_path, tmp_path, precision):
    """FeatureCollector's U M^T on the GPU (als_predict) is bitwise the Java-float dot of the factors, and the
    CSV written from it is byte-identical to the host writer's (FeatureCollector.java:90-110)."""
    from test_host import java_float_dots
    ds = cfk.Dataset.load_netflix(tiny_path)
    app = cfk.ALSApp(4, 10, LAM, 2, 426, 302, precision=precision, seed=42).setup(ds)
    app.run()
    U, M = app.factors()
    P = app.prediction_matrix()
    assert P.shape == (302, 426)
    assert np.array_equal(P, java_float_dots(U.astype(np.float32), M.astype(np.float32)))
    a, c = tmp_path / "a.csv", tmp_path / "c.csv"
    cfk.write_prediction_csv(str(a), U.astype(np.float32), M.astype(np.float32))
    cfk.write_prediction_matrix_csv(str(c), P)
    assert a.read_bytes() == c.read_bytes()


@pytest.mark.parametrize("precision,k", [("f32", 64), ("f64", 10), ("f32", 10)])
def test_device_block_build_matches_host(cfk, oracle_mod, precision, k):
    """als_set_block_coo (GPU radix-sort block build) == als_set_block (host CSR): same work plan, bitwise
    identical half-iteration output, on a sharded synthetic block (G = 3, shard 1) and the whole block."""
    ds, b = _synthetic(cfk, oracle_mod)
    for G, shard in ((1, 0), (3, 1)):
        for side in (0, 1):
            csr = ds.shard_block(side, G, shard)
            coo = ds.shard_coo(side, G, shard)
            opp = ds.shard_info(1 - side, G, shard)["n_slots"]
            F = np.random.default_rng(3).random((opp, k)).astype(np.float32 if precision == "f32" else np.float64)
            outs, stats = [], []
            for mode in ("host", "device"):
                eng = cfk.ALSEngine(k, precision)
                eng.use_torch_stream()
                eng.alloc_factors(1 - side, opp)
                eng.alloc_factors(side, csr["n_slots"])
                if mode == "host":
                    eng.set_block(side, csr["row_ptr"], csr["col"], csr["ratings"], csr["row_offset"], opp)
                else:
                    eng.set_block_coo(side, coo["n_rows"], coo["rows"], coo["cols"], coo["ratings"], coo["row_offset"],
                                      opp)
                eng.write_factors(1 - side, F)
                eng.solve_half(side, LAM)
                outs.append(eng.read_factors(side))
                stats.append(eng.block_stats(side))
                eng.close()
            assert stats[0] == stats[1]
            assert np.array_equal(outs[0], outs[1]), (G, shard, side)


def test_device_block_build_edge_cases(cfk):
    from cfk_amd._lib import ALSError
    eng = cfk.ALSEngine(16, "f32")
    eng.use_torch_stream()
    eng.alloc_factors(0, 3)
    eng.alloc_factors(1, 4)
    eng.set_block_coo(0, 3, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int16), 0, 4)   # empty
    assert eng.block_stats(0)["nnz_padded"] == 0
    # rows 0 and 2 rated, row 1 empty (zero factor), arrival order kept
    eng.set_block_coo(0, 3, np.array([2, 0, 2], np.int32), np.array([1, 3, 0], np.int32), np.array([5, 1, 2], np.int16), 0, 4)
    assert eng.block_stats(0)["nnz_padded"] == 64
    eng.write_factors(1, np.ones((4, 16), np.float32))
    eng.solve_half(0, LAM)
    out = eng.read_factors(0)
    assert np.all(out[1] == 0) and np.all(np.isfinite(out))
    with pytest.raises(ALSError, match="ALS_ERR_INVALID_ARGUMENT"):
        eng.set_block_coo(0, 3, np.array([3], np.int32), np.array([0], np.int32), np.array([1], np.int16), 0, 4)
    with pytest.raises(ALSError, match="ALS_ERR_INVALID_ARGUMENT"):
        eng.set_block_coo(0, 3, np.array([0], np.int32), np.array([4], np.int32), np.array([1], np.int16), 0, 4)
    eng.close()


def _split_slots(deg, nnz_padded):
    """Partial slots of each split row, as the engine's work plan assigns them (als_plan.cpp plan_layout /
    plan_build: rows in order, ceil(deg / chunk) consecutive slots per row longer than chunk)."""
    c = min(max(nnz_padded // 4096, 1024), 32768)
    c = (c + 31) // 32 * 32
    slots, nxt = {}, 0
    for i, d in enumerate(deg):
        if d > c:
            n = -(-int(d) // c)
            slots[i] = (nxt, nxt + n)
            nxt += n
    return slots


def test_bitwise_determinism_netflix_shape(cfk):
    """Full Netflix-shape workload (1e8 ratings, k = 64, pre-split fp16 Gram on both halves, split rows): each half
    repeated from identical inputs -- with the other half run in between, which reuses the shared partial-slot and
    pre-split workspaces -- gives bitwise identical factors. (This is the test that caught an MFMA operand hazard at
    ~20 rows in 17,770; see MFMA_DRAIN in als_mfma.h.) A failure reports each deviating row's kind (split or
    FULL) and its error against the fp64 restatement; slot-level diagnosis (a fixed launch generation) is the
    debug build's tools/split_diag.py."""
    ds = cfk.Dataset.synthetic_netflix(480_189, 17_770, 100_000_000, 0xA15, nthreads=16)
    U0 = ds.init_user_factors(64, 42)
    eng = cfk.ALSEngine(64, "f32")
    for side in (0, 1):
        b = ds.shard_coo(side)
        eng.alloc_factors(side, b["n_slots"])
        eng.set_block_coo(side, b["n_rows"], b["rows"], b["cols"], b["ratings"], 0, ds.shard_info(1 - side)["n_slots"])
    reps = 6
    Ms, Us = [], []
    for rep in range(reps):
        eng.write_factors(1, U0)
        eng.solve_half(0, LAM)
        Ms.append(eng.read_factors(0))
        eng.solve_half(1, LAM)
        Us.append(eng.read_factors(1))
    nnz_padded = eng.block_stats(0)["nnz_padded"]
    eng.close()
    report = []
    mblk = ds.shard_block(0)
    slots = _split_slots(np.diff(mblk["row_ptr"]), nnz_padded)
    for name, reps_ in (("movie", Ms), ("user", Us)):
        side = 0 if name == "movie" else 1
        rows = sorted(set().union(*[set(np.nonzero(np.any(reps_[0] != reps_[r], axis=1))[0].tolist())
                                    for r in range(1, reps)]))
        if not rows:
            continue
        blk = mblk if side == 0 else ds.shard_block(side)
        for i in rows[:4]:
            lo, hi = int(blk["row_ptr"][i]), int(blk["row_ptr"][i + 1])
            odd = [r for r in range(reps) if sum(np.array_equal(reps_[r][i], reps_[q][i]) for q in range(reps)) == 1]
            err, where = [], ""
            if side == 0:   # fp64 restatement of the movie update from U0 (MFeatureCalculator.java:82-99)
                Y = U0[blk["col"][lo:hi], :64].astype(np.float64)
                rr = blk["ratings"][lo:hi].astype(np.float64)
                ref = np.linalg.solve(Y.T @ Y + np.float64(np.float32(LAM)) * (hi - lo) * np.eye(64), Y.T @ rr)
                err = [float(np.max(np.abs(reps_[r][i] - ref)) / np.max(np.abs(ref))) for r in range(reps)]
                where = f" split row, slots {slots[i]}" if i in slots else " FULL row"
            report.append(f"{name} row {i} deg {hi - lo}{where}; deviating rep(s) {odd}; fp64 err per rep {err}")
        report.append(f"{name}: {len(rows)} differing rows in total")
    assert not report, "nondeterministic rows: " + "; ".join(report)


def test_engine_ordered_with_torch_default_stream(cfk):
    """use_torch_stream() on torch's default stream (handle 0) must put the engine on that NULL stream, so a torch
    op (or an RCCL collective, which waits on torch's current stream) issued right after als_solve_half sees the
    solved rows. The engine used to pick a private non-blocking stream here, and the all-gather of the multi-GPU
    driver was then unordered with the solve."""
    assert torch.cuda.current_stream().cuda_stream == 0
    ds = cfk.Dataset.synthetic_netflix(200_000, 6_000, 20_000_000, 7, nthreads=16)
    eng = cfk.ALSEngine(64, "f32")
    eng.use_torch_stream()
    for side in (0, 1):
        b = ds.shard_coo(side)
        eng.alloc_factors(side, b["n_slots"])
        eng.set_block_coo(side, b["n_rows"], b["rows"], b["cols"], b["ratings"], 0, ds.shard_info(1 - side)["n_slots"])
    eng.write_factors(1, ds.init_user_factors(64, 42))
    torch.cuda.synchronize()
    eng.solve_half(0, LAM)                                   # async on the engine's stream
    seen = eng.factors[0][:-1, :64].clone().cpu().numpy()   # torch, default stream, issued immediately
    torch.cuda.synchronize()
    M = eng.read_factors(0)
    eng.close()
    assert np.abs(M).sum() > 0
    assert np.array_equal(seen, M), int(np.any(seen != M, axis=1).sum())


def test_native_rccl_exchange_world1(cfk, oracle_mod):
    """The C-ABI exchange (als_comm_unique_id / als_comm_init / als_allgather_shard, RCCL) on a one-rank
    communicator: the all-gather of the whole shard and of single chunks leaves the replicas bitwise unchanged,
    and the chunked user half over chunk-major slots (als_set_row_layout) with an all-gather after every chunk
    (on the engine's comm stream, overlapping the next chunk) reproduces als_solve_half exactly. The N > 1
    exchange runs on the driver's multi-GPU node (test_comm_init_group_two_gpus where one exists)."""
    ds, b = _synthetic(cfk, oracle_mod)
    ds.set_slot_chunks(1, 3)                              # user slots in 3 chunks (world 1: identity layout)
    eng = cfk.ALSEngine(64, "f32")
    uid = cfk.ALSEngine.comm_unique_id()
    assert len(uid) == 128
    eng.comm_init(1, 0, uid)
    assert eng.comm_info() == (1, 0)
    info = [ds.shard_info(s) for s in (0, 1)]
    sc, nc = ds.slot_layout(1)
    assert nc == 3 and info[1]["n_slots"] == 3 * sc >= info[1]["n_rows"]
    for side in (0, 1):
        c = ds.shard_coo(side)
        eng.alloc_factors(side, info[side]["n_slots"])
        eng.set_block_coo(side, c["n_rows"], c["rows"], c["cols"], c["ratings"], 0, info[1 - side]["n_slots"])
    eng.set_row_layout(1, sc, sc)
    eng.write_factors(1, ds.init_user_factors(64, 3))
    eng.solve_half(0, LAM)
    M = eng.read_factors(0)
    eng.allgather_shard(0, info[0]["slots_per_shard"])
    eng.allgather_shard(0, 6, 2)                          # rows [12, 18)
    assert np.array_equal(eng.read_factors(0), M)
    eng.solve_half(1, LAM)
    U = eng.read_factors(1)
    n = info[1]["n_rows"]
    bounds = [0, min(sc, n), min(2 * sc, n), n]
    eng.set_chunks(1, bounds)
    for c in range(3):
        eng.solve_half_chunk(1, LAM, c)
        eng.allgather_shard(1, sc, c)
    assert np.array_equal(eng.read_factors(1), U)
    eng.solve_half(0, LAM)             # reads U: ordered after the pending all-gathers of the user side
    M2 = eng.read_factors(0)
    eng.close()
    ref = oracle_mod.update_side(b.movie, U[:n].astype(np.float64), LAM, "f64")
    assert np.linalg.norm(M2 - ref) / np.linalg.norm(ref) < 1e-4


def test_row_layout_scatters_rows_into_chunk_major_slots(cfk, oracle_mod):
    """als_set_row_layout: local row i is solved into row_offset + (i // Sc) * stride + i % Sc -- the slots of
    shard `row_offset / Sc` in a chunk-major layout of `stride / Sc` shards -- and every other row is untouched."""
    ds, b = _synthetic(cfk, oracle_mod)
    blk = ds.shard_block(1)
    n = blk["n_rows"]
    F = np.random.default_rng(8).random((len(b.movie.ids), 64)).astype(np.float32)
    whole = _one_half(cfk, 1, blk, F, 64, "f32", len(b.movie.ids))
    G, shard, sc = 3, 1, -(-n // 4)                       # 4 chunks of a 3-shard layout, this is shard 1
    eng = cfk.ALSEngine(64, "f32")
    eng.alloc_factors(0, len(b.movie.ids))
    eng.alloc_factors(1, 4 * G * sc)
    eng.set_block(1, blk["row_ptr"], blk["col"], blk["ratings"], shard * sc, len(b.movie.ids))
    eng.set_row_layout(1, sc, G * sc)
    eng.write_factors(0, F)
    eng.write_factors(1, np.full((4 * G * sc, 64), 7.0, np.float32))
    eng.solve_half(1, LAM)
    got = eng.read_factors(1)
    se, cnt = eng.sq_error(1)
    eng.close()
    i = np.arange(n)
    rows = shard * sc + (i // sc) * G * sc + i % sc
    assert np.array_equal(got[rows], whole)
    others = np.setdiff1d(np.arange(4 * G * sc), rows)
    assert np.all(got[others] == 7.0)
    se_o, cnt_o = oracle_mod.sq_error(b.user, whole.astype(np.float64), F.astype(np.float64))
    assert cnt == cnt_o and se == pytest.approx(se_o, rel=1e-4)


def test_comm_timeout_names_the_pending_exchange(cfk, oracle_mod):
    """als_comm_set_timeout: with a communicator, the engine's host waits are bounded; a stream still busy past the
    bound fails the synchronising call with ALS_ERR_COMM naming the last all-gather issued (side, chunk), the
    communicator aborted -- the diagnosis a hung exchange gets instead of a hang. Forced here with a 1-ms bound behind
    a queue of real halves on a one-rank communicator (whose kernels all complete)."""
    from cfk_amd._lib import ALSError
    ds = cfk.Dataset.synthetic_netflix(n_users=60_000, n_movies=2_000, nnz=3_000_000, seed=11, nthreads=8)
    eng = cfk.ALSEngine(64, "f32")
    eng.comm_init(1, 0, cfk.ALSEngine.comm_unique_id())
    info = [ds.shard_info(s) for s in (0, 1)]
    for side in (0, 1):
        c = ds.shard_coo(side)
        eng.alloc_factors(side, info[side]["n_slots"])
        eng.set_block_coo(side, c["n_rows"], c["rows"], c["cols"], c["ratings"], 0, info[1 - side]["n_slots"])
    eng.write_factors(1, ds.init_user_factors(64, 3))
    eng.synchronize()
    eng.comm_set_timeout(1)
    for _ in range(40):
        eng.solve_half(0, LAM)
        eng.allgather_shard(0, info[0]["slots_per_shard"])
        eng.solve_half(1, LAM)
        eng.allgather_shard(1, info[1]["slots_per_shard"])
    with pytest.raises(ALSError, match="ALS_ERR_COMM.*side user chunk 0"):
        eng.synchronize()
    eng.close()   # drains the stream: the queued kernels all complete


def test_comm_init_group_one_engine(cfk):
    e = cfk.ALSEngine(16, "f32")
    cfk.ALSEngine.comm_init_group([e])
    assert e.comm_info() == (1, 0)
    from cfk_amd._lib import ALSError, call
    with pytest.raises(ALSError, match="ALS_ERR_STATE"):
        cfk.ALSEngine.comm_init_group([e])            # already has a communicator
    with pytest.raises(ALSError, match="ALS_ERR_STATE"):
        call("als_comm_group_end")                     # no open group
    e.close()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs 2 GPUs (one engine per device)")
def test_comm_init_group_two_gpus(cfk, oracle_mod):
    """One host thread driving G = 2 engines through als_comm_init_group, every half's all-gathers grouped
    (als_comm_group_start / _end: the completion events are recorded at the outermost group end): the factors
    equal the one-GPU run's. Chunk-major user slots, 2 chunks, all-gathers after each chunk."""
    from cfk_amd._lib import call
    ds, b = _synthetic(cfk, oracle_mod)
    G, iters = 2, 3
    ds.set_slot_chunks(1, 2)
    engs = [cfk.ALSEngine(64, "f32", device=g) for g in range(G)]
    cfk.ALSEngine.comm_init_group(engs)
    info = [[ds.shard_info(s, G, g) for s in (0, 1)] for g in range(G)]
    sc = {s: ds.slot_layout(s, G)[0] for s in (0, 1)}
    for g, e in enumerate(engs):
        torch.cuda.set_device(g)
        for side in (0, 1):
            c = ds.shard_coo(side, G, g)
            e.alloc_factors(side, info[g][side]["n_slots"])
            e.set_block_coo(side, c["n_rows"], c["rows"], c["cols"], c["ratings"], c["row_offset"],
                            info[g][1 - side]["n_slots"])
        e.set_row_layout(1, sc[1], G * sc[1])
        n = info[g][1]["n_rows"]
        e.set_chunks(1, [0, min(sc[1], n), n])
        e.write_factors(1, ds.init_user_factors(64, 9, G))
    torch.cuda.set_device(0)
    for _ in range(iters):
        for e in engs:
            e.solve_half(0, LAM)
        call("als_comm_group_start")
        for e in engs:
            e.allgather_shard(0, sc[0], 0)
        call("als_comm_group_end")
        for c in range(2):
            for e in engs:
                e.solve_half_chunk(1, LAM, c)
            call("als_comm_group_start")
            for e in engs:
                e.allgather_shard(1, sc[1], c)
            call("als_comm_group_end")
    U = [e.read_factors(1) for e in engs]
    M = [e.read_factors(0) for e in engs]
    for e in engs:
        e.close()
    assert np.array_equal(U[0], U[1]) and np.array_equal(M[0], M[1])
    app = cfk.ALSApp(1, 64, LAM, iters, precision="f32", seed=9).setup(
        cfk.Dataset.synthetic_netflix(n_users=3000, n_movies=400, nnz=90_000, seed=11, nthreads=8))
    app.run()
    U1, M1 = app.factors()
    assert np.array_equal(U[0][ds.slots(1, G)], U1) and np.array_equal(M[0][ds.slots(0, G)], M1)


def test_gram_variants_vs_oracle(cfk, oracle_mod, monkeypatch):
    """Every knob that selects another product code path, against the fp64 oracle at k = 64 and 128:
    ALS_GRAM=f32 (exact v_mfma_f32_16x16x4_f32 Gram instead of the split-bf16 one), ALS_PRESPLIT=0 (the k = 64
    user half on the on-the-fly split instead of the pre-split LDS-DMA Gram; ALS_PRESPLIT=1 is the default there),
    ALS_REFINE_MIN_PIVOT=2 (the refinement step on every row; the product library clamps lower values to the
    validated 0.45 gate, so =0 is the default path; with ALS_PRESPLIT=0 as well: the matrix-free refinement of the
    on-the-fly path), and ALS_DUAL_SIDE=0 (entry-space launches on the engine stream
    instead of the side stream, bitwise equal to the default)."""
    ds, b = _synthetic(cfk, oracle_mod)
    blk = ds.shard_block(1)
    knobs = ("ALS_GRAM", "ALS_DUAL_SIDE", "ALS_PRESPLIT", "ALS_REFINE_MIN_PIVOT")
    for k in (64, 128):
        F = np.random.default_rng(k).random((len(b.movie.ids), k))
        ref = oracle_mod.update_side(b.user, F, LAM, "f64")
        ref32 = oracle_mod.update_side(b.user, F.astype(np.float32), LAM, "f32")
        outs = {}
        for env in ({}, {"ALS_GRAM": "f32"}, {"ALS_DUAL_SIDE": "0"}, {"ALS_PRESPLIT": "0"},
                    {"ALS_REFINE_MIN_PIVOT": "2"}, {"ALS_REFINE_MIN_PIVOT": "0"},
                    {"ALS_PRESPLIT": "0", "ALS_REFINE_MIN_PIVOT": "2"}):
            for name in knobs:
                monkeypatch.delenv(name, raising=False)
            for name, v in env.items():
                monkeypatch.setenv(name, v)
            outs[tuple(env.items())] = _one_half(cfk, 1, blk, F.astype(np.float32), k, "f32", len(b.movie.ids))
        norm = np.linalg.norm(ref, axis=1)
        rel_ref = np.linalg.norm(ref32 - ref, axis=1) / norm
        for got in outs.values():
            rel = np.linalg.norm(got - ref, axis=1) / norm
            assert np.percentile(rel, 99) <= max(2 * np.percentile(rel_ref, 99), 2e-5), k
            assert rel.max() <= max(3 * rel_ref.max(), 1e-4), k
        assert np.array_equal(outs[()], outs[(("ALS_DUAL_SIDE", "0"),)]), k
        assert np.array_equal(outs[()], outs[(("ALS_REFINE_MIN_PIVOT", "0"),)]), k   # clamped to the gate


def test_entry_space_only_for_rows_not_longer_than_k(cfk, oracle_mod):
    """k = 80 (KP = 128): rows of up to 3 padded blocks qualify for the entry-space solve by length, but one with
    n > k entries would make the n x n system rank-deficient up to lambda n I: those rows take the
    k x k path. Rows of 65..96 ratings are checked against the oracle, and the plan counts them out of the
    entry-space launches."""
    rng = np.random.default_rng(80)
    n_movies, k = 300, 80
    degs = np.concatenate([rng.integers(65, 97, 150), rng.integers(1, 80, 150)])
    mids, uids, rats = [], [], []
    for u, d in enumerate(degs):
        ms = rng.choice(n_movies, size=int(d), replace=False)
        mids += (ms + 1).tolist()
        uids += [u + 1] * int(d)
        rats += rng.integers(1, 6, int(d)).tolist()
    ds = cfk.Dataset.from_ratings(np.array(mids), np.array(uids), np.array(rats))
    m, u, r = ds.ratings()
    b = oracle_mod.build_blocks(m, u, r)
    blk = ds.shard_block(1)
    F = rng.random((len(b.movie.ids), k))
    eng = cfk.ALSEngine(k, "f32")
    eng.alloc_factors(0, len(b.movie.ids))
    eng.alloc_factors(1, blk["n_rows"])
    eng.set_block(1, blk["row_ptr"], blk["col"], blk["ratings"], 0, len(b.movie.ids))
    deg = np.diff(blk["row_ptr"])
    assert eng.block_path(1)["dual_rows"] == int(np.sum((deg <= k) & (deg <= 96)))
    eng.write_factors(0, F.astype(np.float32))
    eng.solve_half(1, LAM)
    got = eng.read_factors(1)
    eng.close()
    ref = oracle_mod.update_side(b.user, F, LAM, "f64")
    ref32 = oracle_mod.update_side(b.user, F.astype(np.float32), LAM, "f32")
    norm = np.linalg.norm(ref, axis=1)
    rel = np.linalg.norm(got - ref, axis=1) / norm
    rel_ref = np.linalg.norm(ref32 - ref, axis=1) / norm
    assert rel.max() <= max(3 * rel_ref.max(), 1e-4), (rel.max(), rel_ref.max())


@pytest.mark.parametrize("k", [64, 128])
def test_short_rows_entry_space_matches_kxk(cfk, oracle_mod, monkeypatch, k):
    """Short rows (1 padded block at k = 64, <= 2 at k = 128) are solved in entry space by als_solve_dual,
    (Y Y^T + lambda n I) alpha = r, m = Y^T alpha: the same solution as the k x k system. Against the fp64
    oracle at the every-k bar, and against the k x k path (ALS_DUAL=0) to fp32 accuracy."""
    ds, b = _synthetic(cfk, oracle_mod)                     # users of ~30 ratings: most rows are short
    F = np.random.default_rng(k + 7).random((len(b.movie.ids), k))
    blk = ds.shard_block(1)
    outs = []
    for env in ("1", "0"):
        monkeypatch.setenv("ALS_DUAL", env)
        eng = cfk.ALSEngine(k, "f32")
        eng.alloc_factors(0, len(b.movie.ids))
        eng.alloc_factors(1, blk["n_rows"])
        eng.set_block(1, blk["row_ptr"], blk["col"], blk["ratings"], 0, len(b.movie.ids))
        dual = eng.block_path(1)["dual_rows"]
        assert (dual > blk["n_rows"] // 3) if env == "1" else dual == 0
        eng.write_factors(0, F.astype(np.float32))
        eng.solve_half(1, LAM)
        outs.append(eng.read_factors(1))
        eng.close()
    ref = oracle_mod.update_side(b.user, F, LAM, "f64")
    ref32 = oracle_mod.update_side(b.user, F.astype(np.float32), LAM, "f32")
    norm = np.linalg.norm(ref, axis=1)
    for got in outs:
        rel = np.linalg.norm(got - ref, axis=1) / norm
        rel_ref = np.linalg.norm(ref32 - ref, axis=1) / norm
        assert np.percentile(rel, 99) <= max(2 * np.percentile(rel_ref, 99), 2e-5)
        assert rel.max() <= max(3 * rel_ref.max(), 1e-4), (rel.max(), rel_ref.max())
