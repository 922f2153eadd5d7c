"""als_similar on the GPU: top-N nearest rows of one factor table by cosine or dot product, compared EXACTLY with numpy.

Expected values come from tests/similar_ref.py only (java_float_dots, float32 sqrt / divide / multiply, a self mask,
np.lexsort((position, -score))) -- never from the code under test. idx is compared with array_equal, scores with
array_equal on the floats, padding is -1 / -inf. Reference semantics: include/als.h (als_similar).
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

import similar_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

SIDE_MOVIE, SIDE_USER = 0, 1
COSINE, DOT = 0, 1
MODES = [(m, x) for m in ("cosine", "dot") for x in (True, False)]


@pytest.fixture(scope="module")
def gpu(cfk):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return cfk


def make_engine(cfk, k, precision, table, side=SIDE_MOVIE):
    """An engine with `table` as the factors of `side`; the other side stays unallocated."""
    eng = cfk.ALSEngine(k, precision)
    eng.alloc_factors(side, table.shape[0])
    eng.write_factors(side, table)
    return eng


def check(eng, side, T, q, c, n, modes=MODES):
    """Every (metric, exclude_self) of `modes` against the restatement. The reference is computed once per distinct
    query slot (a list's content depends on the slot alone) and shared by the modes."""
    q, c = np.asarray(q, np.int64), np.asarray(c, np.int64)
    uq, inv = np.unique(q, return_inverse=True)
    S = {m: ref.similar_scores(T, uq, c, m) for m in {m for m, _ in modes}}
    for metric, excl in modes:
        idx, score = eng.similar(side, q, c, n, metric, excl)
        want_idx, want_score = ref.expected_lists(S[metric], uq, c, n, excl)
        assert idx.dtype == np.int32 and score.dtype == np.float32 and idx.shape == (len(q), n)
        assert np.array_equal(idx, want_idx[inv]), (metric, excl)
        assert np.array_equal(score, want_score[inv]), (metric, excl)


# ---------------------------------------------------------------------------------------------------------------------
# parity ladder
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (1, 2, 1), (3, 7, 10), (64, 64, 10), (65, 65, 64), (70, 333, 10), (130, 1000, 64), (5, 5000, 1),
          (16, 20000, 33), (16400, 130, 10)]     # the last: enough query tiles for one segment over three candidate tiles
_tables = {}


def tables(cfk, precision, k):
    """One engine and one table per (precision, k), shared by every shape and never modified. The sides alternate
    along the ladder."""
    key = (precision, k)
    if key not in _tables:
        side = ref.CONFIGS.index(key) % 2
        T = ref.ladder_table(precision, k)          # f64: not float-representable, narrowed by the engine
        _tables[key] = (make_engine(cfk, k, precision, T, side), side, T)
    return _tables[key]


def ladder_rows(rng, n_queries, n_cand):
    """Candidates: a shuffled subset of the table with a few slots listed twice. Queries: drawn (with repeats once there
    are more queries than that) half from the candidates and half from the rows that are not candidates."""
    repeats = min(5, n_cand // 2)
    cand = rng.choice(ref.N_TABLE, n_cand - repeats, replace=False)
    outside = np.setdiff1d(np.arange(ref.N_TABLE), cand)
    cand = rng.permutation(np.concatenate([cand, rng.choice(cand, repeats, replace=False)]) if repeats else cand)
    n_in = (n_queries + 1) // 2
    pool_in, pool_out = rng.choice(cand, min(n_in, 150)), rng.choice(outside, min(n_queries - n_in, 100)) \
        if n_queries > n_in else np.zeros(0, np.int64)
    q = np.concatenate([rng.choice(pool_in, n_in), rng.choice(pool_out, n_queries - n_in) if len(pool_out) else pool_out])
    return rng.permutation(q).astype(np.int64), cand.astype(np.int64)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("precision,k", ref.CONFIGS)
def test_parity_ladder(gpu, precision, k, shape):
    n_queries, n_cand, top_n = shape
    eng, side, T = tables(gpu, precision, k)
    q, c = ladder_rows(np.random.default_rng(n_queries * 7 + n_cand), n_queries, n_cand)
    assert len(q) == n_queries and len(c) == n_cand
    check(eng, side, T, q, c, top_n)


def test_ladder_runs_both_launch_shapes(gpu):
    eng, _, _ = tables(gpu, "f32", 5)
    plans = [eng.similar_plan(nq, nc, n) for nq, nc, n in SHAPES]
    assert any(p["segments"] == 1 and nc > p["user_tile"] for p, (_, nc, _) in zip(plans, SHAPES)), plans
    assert any(p["segments"] > 1 for p in plans), plans
    for p, (nq, nc, n) in zip(plans, SHAPES):
        assert p == eng.recommend_plan(nq, nc, n)                       # the same four numbers
        assert p["segment_len"] * p["segments"] >= nc and 0 < p["lds_bytes"] <= 160 * 1024


# ---------------------------------------------------------------------------------------------------------------------
# self-exclusion
# ---------------------------------------------------------------------------------------------------------------------
def test_all_against_all_never_returns_the_own_position(gpu):
    eng, side, T = tables(gpu, "f32", 5)
    rows = np.random.default_rng(31).choice(ref.N_TABLE, 200, replace=False).astype(np.int64)
    for metric in ("cosine", "dot"):
        idx, _ = eng.similar(side, rows, rows, 10, metric, True)
        assert not np.any(idx == np.arange(200)[:, None]) and np.all(idx >= 0)
    idx, _ = eng.similar(side, rows, rows, 10, "cosine", False)
    assert np.all(np.any(idx == np.arange(200)[:, None], axis=1))       # without the flag the row finds itself
    check(eng, side, T, rows, rows, 10)


def test_slot_listed_three_times_across_segments(gpu):
    eng, side, T = tables(gpu, "f32", 64)
    rng = np.random.default_rng(32)
    rows = rng.choice(ref.N_TABLE, 5001, replace=False).astype(np.int64)
    q, c = rows[:1], rows[1:].copy()
    plan = eng.similar_plan(1, 5000, 10)
    assert plan["segments"] >= 3
    at = [3, plan["segment_len"] + 7, 2 * plan["segment_len"] + 1]      # the first three segments
    c[at] = q[0]
    for metric in ("cosine", "dot"):
        idx, _ = eng.similar(side, q, c, 10, metric, True)
        assert not np.any(np.isin(idx, at))
        idx, _ = eng.similar(side, q, c, 10, metric, False)
        assert idx[0, :3].tolist() == at                                 # the best three by far, tied: by position
    check(eng, side, T, q, c, 10)


def test_query_outside_the_candidates_excludes_nothing(gpu):
    eng, side, T = tables(gpu, "f32", 33)
    rows = np.random.default_rng(33).choice(ref.N_TABLE, 700, replace=False).astype(np.int64)
    q, c = rows[:40], rows[40:]
    for metric in ("cosine", "dot"):
        a, b = eng.similar(side, q, c, 12, metric, True), eng.similar(side, q, c, 12, metric, False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    check(eng, side, T, q, c, 12)


@pytest.mark.parametrize("n_queries", [1, 16400], ids=["segmented", "one_segment"])
def test_self_does_not_raise_the_threshold(gpu, n_queries):
    """Dot product, top_n = 1, the query's self-dot far above every other score and its slot at positions 0, 1 and 2: had
    one of those cells reached the survivor queue, the threshold would sit above every other row and the list would
    come back as padding (or as the row itself)."""
    rng = np.random.default_rng(34)
    T = rng.standard_normal((301, 8)).astype(np.float32)
    T[0] *= 1000
    eng = make_engine(gpu, 8, "f32", T)
    c = np.concatenate([[0, 0, 0], np.arange(1, 301)]).astype(np.int64)
    q = np.zeros(n_queries, np.int64)
    assert (eng.similar_plan(n_queries, len(c), 1)["segments"] == 1) == (n_queries > 1)
    idx, score = eng.similar(SIDE_MOVIE, q, c, 1, "dot", True)
    S = ref.similar_scores(T, [0], c, "dot")
    assert S[0, 0] > 100 * np.max(S[0, 3:])
    best = 3 + int(np.argmax(S[0, 3:]))
    assert np.all(idx == best) and np.all(score == S[0, best])
    check(eng, SIDE_MOVIE, T, q, c, 1)


# ---------------------------------------------------------------------------------------------------------------------
# edge rows
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_rows(gpu):
    rng = np.random.default_rng(35)
    T = rng.standard_normal((500, 5)).astype(np.float32)
    T[[0, 77]] = 0
    eng = make_engine(gpu, 5, "f32", T, SIDE_USER)
    c = np.arange(500, dtype=np.int64)
    for n in (1, 10, 64):
        idx, score = eng.similar(SIDE_USER, [0], c, n, "cosine", True)
        assert np.array_equal(idx[0], np.arange(1, n + 1)) and np.all(score == 0)      # the first non-self positions
    # a zero row as candidate scores 0: with everything returned, it sits between the positive and the negative ones
    sub = np.concatenate([[77], rng.choice(np.arange(100, 500), 39, replace=False)]).astype(np.int64)
    idx, score = eng.similar(SIDE_USER, [5, 6], sub, 64, "cosine", True)
    assert np.all(score[idx == 0] == 0) and np.all(idx[:, 40:] == -1) and np.all(np.isneginf(score[:, 40:]))
    check(eng, SIDE_USER, T, [0, 5, 77, 6], c, 10)
    check(eng, SIDE_USER, T, [5, 6, 0], sub, 64)                        # top_n above the eligible count pads


def test_three_distinct_rows_repeated_tie_by_position(gpu):
    rng = np.random.default_rng(36)
    T = np.tile(rng.standard_normal((3, 10)).astype(np.float32), (100, 1))
    eng = make_engine(gpu, 10, "f32", T)
    c = np.arange(300, dtype=np.int64)
    for n in (7, 64):
        check(eng, SIDE_MOVIE, T, [0, 1, 2, 299], c, n)
    idx, score = eng.similar(SIDE_MOVIE, [4], c, 5, "cosine", True)
    assert idx[0].tolist() == [1, 7, 10, 13, 16] and len(set(score[0].tolist())) == 1   # its copies, own slot 4 left out


def test_top_n_above_the_eligible_count_pads(gpu):
    eng, side, T = tables(gpu, "f32", 5)
    idx, score = eng.similar(side, [9], [9, 9, 4], 3, "cosine", True)
    assert idx.tolist() == [[2, -1, -1]] and np.all(np.isneginf(score[0, 1:]))
    idx, score = eng.similar(side, [9], [9], 2, "dot", True)
    assert idx.tolist() == [[-1, -1]] and np.all(np.isneginf(score))
    check(eng, side, T, [9, 4], [9, 9, 4], 3)


# ---------------------------------------------------------------------------------------------------------------------
# insertion stress
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 10, 64])
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_insertion_stress(gpu, order, n):
    """Candidates in ascending reference cosine to the query all beat the threshold (most merges and queue flushes),
    descending ones never do after the first n. Once through the segmented plan, once through one workgroup per query
    tile that sweeps all 47 candidate tiles."""
    eng, side, T = tables(gpu, "f32", 5)
    rows = np.random.default_rng(37).choice(ref.N_TABLE, 3001, replace=False).astype(np.int64)
    q, c = rows[:1], rows[1:]
    by = np.argsort(ref.similar_scores(T, q, c, "cosine")[0], kind="stable")
    c = c[by] if order == "ascending" else c[by[::-1]]
    check(eng, side, T, q, c, n, [("cosine", True)])
    many = np.repeat(q, 64 * 300)
    assert eng.similar_plan(len(many), 3000, n)["segments"] == 1
    check(eng, side, T, many, c, n, [("cosine", True)])


# ---------------------------------------------------------------------------------------------------------------------
# the workspace the synchronous calls share
# ---------------------------------------------------------------------------------------------------------------------
def _csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    return ptr, np.concatenate([np.asarray(x, np.int32) for x in lists]).astype(np.int32)


def test_shared_workspace_growing_and_shrinking(gpu):
    """similar, recommend and rank_targets interleaved on one engine, sizes up and down: every result is bit for bit that
    of the same call on an engine that has made no other call."""
    k = 16
    rng = np.random.default_rng(38)
    U = rng.standard_normal((60, k)).astype(np.float32)
    M = rng.standard_normal((2100, k)).astype(np.float32)

    def fresh():
        eng = gpu.ALSEngine(k, "f32")
        for side, t in ((SIDE_USER, U), (SIDE_MOVIE, M)):
            eng.alloc_factors(side, t.shape[0])
            eng.write_factors(side, t)
        return eng

    def sim(nq, nc, n, metric):
        q, c = rng.integers(0, 2100, nq), rng.integers(0, 2100, nc)
        return lambda e: e.similar(SIDE_MOVIE, q, c, n, metric, True)

    def rec(nu, nc, n):
        u, m = rng.integers(0, 60, nu), rng.permutation(2100)[:nc]
        excl = _csr([np.sort(rng.choice(nc, 4, replace=False)) for _ in range(nu)])
        return lambda e: e.recommend(u, m, n, excl)

    def rank(nu, nc, nt):
        u, m = rng.integers(0, 60, nu), rng.permutation(2100)[:nc]
        tg = _csr(np.array_split(rng.integers(0, nc, nt).astype(np.int32), nu))
        return lambda e: e.rank_targets(u, m, tg)

    calls = [sim(3, 50, 5, "cosine"), rec(20, 400, 10), sim(40, 2000, 64, "dot"), rank(20, 900, 70), sim(200, 2100, 10, "cosine"),
             rec(5, 30, 3), sim(2, 9, 4, "cosine"), rank(3, 40, 9), sim(70, 333, 20, "cosine"),
             lambda e: e.similar(SIDE_USER, np.arange(60), np.arange(60), 7, "cosine", True)]
    shared = fresh()
    for i, call in enumerate(calls):
        got, want = call(shared), call(fresh())
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), i


def test_similar_between_two_chunks_of_a_half(gpu, tiny_path):
    """k = 64 (the half gathers the pre-split table chunk 0 prepared): a similar call between chunk 0 and chunk 1 of the
    movie half leaves chunk 1's output bitwise unchanged."""
    out = []
    for with_similar in (False, True):
        ds = gpu.Dataset.load_netflix(tiny_path)
        app = gpu.ALSApp(4, 64, 0.05, 1, precision="f32", seed=7).setup(ds)
        eng = app.engine
        n = app.info[SIDE_MOVIE]["n_rows"]
        eng.set_chunks(SIDE_MOVIE, [0, n // 2, n])
        assert eng.split_info(SIDE_MOVIE)["presplit"]          # the table chunk 0 prepares and chunk 1 reuses
        eng.solve_half_chunk(SIDE_MOVIE, 0.05, 0)
        if with_similar:
            idx, _ = eng.similar(SIDE_USER, np.arange(302), np.arange(302), 64)
            assert idx.shape == (302, 64) and np.all(idx >= 0)
            idx, _ = eng.similar(SIDE_MOVIE, np.arange(426), np.arange(426), 10, "dot", False)
            assert idx.shape == (426, 10)
        eng.solve_half_chunk(SIDE_MOVIE, 0.05, 1)
        out.append(eng.read_factors(SIDE_MOVIE))
    assert np.array_equal(out[0], out[1]) and np.any(out[0][n // 2:] != 0)


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(gpu):
    from cfk_amd import _lib
    from cfk_amd._lib import ALSError
    eng, side, _ = tables(gpu, "f32", 5)
    q, c = np.arange(3), np.arange(50)
    bad = "ALS_ERR_INVALID_ARGUMENT"
    for n in (0, 65, -1):
        with pytest.raises(ALSError, match=bad):
            eng.similar(side, q, c, n)
        with pytest.raises(ALSError, match=bad):
            eng.similar_plan(3, 50, n)
    with pytest.raises(ALSError, match=bad):
        eng.similar_plan(-1, 50, 5)
    with pytest.raises(ValueError):
        eng.similar(side, q, c, 5, metric="euclid")
    with pytest.raises(ALSError, match=rf"{bad}.*als_similar: query_rows\[1\] = {ref.N_TABLE} is outside \[0, {ref.N_TABLE}\)"):
        eng.similar(side, [0, ref.N_TABLE], c, 5)
    with pytest.raises(ALSError, match=rf"{bad}.*als_similar: cand_rows\[2\] = -1 is outside \[0, {ref.N_TABLE}\)"):
        eng.similar(side, q, [4, 5, -1], 5)
    with pytest.raises(ALSError, match="ALS_ERR_STATE"):
        eng.similar(1 - side, q, c, 5)                                   # the other side was never allocated
    with pytest.raises(ALSError, match="ALS_ERR_STATE"):
        gpu.ALSEngine(5, "f32").similar(side, q, c, 5)
    # the raw call: side, metric, counts, NULL pointers
    L = _lib.lib()
    qr, cr = q.astype(np.int64), c.astype(np.int64)
    idx, score = np.full((3, 5), 77, np.int32), np.full((3, 5), 7.5, np.float32)
    pq, pc = _lib.ptr(qr, ctypes.c_int64), _lib.ptr(cr, ctypes.c_int64)
    outs = (_lib.ptr(idx, ctypes.c_int32), _lib.ptr(score, ctypes.c_float))
    assert L.als_similar(eng._h, side, COSINE, pq, 3, pc, 50, 5, 1, *outs) == 0 and np.all(idx != 77)
    idx[:], score[:] = 77, 7.5
    for s in (2, -1):
        assert L.als_similar(eng._h, s, COSINE, pq, 3, pc, 50, 5, 1, *outs) == 1
    for m in (2, -1):
        assert L.als_similar(eng._h, side, m, pq, 3, pc, 50, 5, 1, *outs) == 1
        assert b"metric" in L.als_last_error()
    assert L.als_similar(eng._h, side, DOT, pq, -1, pc, 50, 5, 1, *outs) == 1
    assert L.als_similar(eng._h, side, DOT, pq, 3, pc, -1, 5, 1, *outs) == 1
    assert L.als_similar(None, side, DOT, pq, 3, pc, 50, 5, 1, *outs) == 1
    assert L.als_similar(eng._h, side, DOT, None, 3, pc, 50, 5, 1, *outs) == 1
    assert L.als_similar(eng._h, side, DOT, pq, 3, None, 50, 5, 1, *outs) == 1
    assert L.als_similar(eng._h, side, DOT, pq, 3, pc, 50, 5, 1, None, outs[1]) == 1
    assert L.als_similar(eng._h, side, DOT, pq, 3, pc, 50, 5, 1, outs[0], None) == 1
    assert L.als_similar(eng._h, side, DOT, pq, 3, pc, 2 ** 31, 5, 1, *outs) == 1
    info = (ctypes.c_int64 * 4)()
    assert L.als_similar_plan(None, 3, 50, 5, info) == 1 and L.als_similar_plan(eng._h, 3, 50, 5, None) == 1
    # nothing to do: ALS_OK, outputs untouched
    assert L.als_similar(eng._h, side, COSINE, pq, 0, pc, 50, 5, 1, *outs) == 0
    assert L.als_similar(eng._h, side, COSINE, pq, 3, pc, 0, 5, 1, *outs) == 0
    assert L.als_similar(eng._h, side, COSINE, None, 0, None, 0, 5, 1, None, None) == 0
    assert np.all(idx == 77) and np.all(score == 7.5)


# ---------------------------------------------------------------------------------------------------------------------
# end to end on the tiny sample
# ---------------------------------------------------------------------------------------------------------------------
def _tiny_app(cfk, tiny_path, precision, k=10, iters=2):
    ds = cfk.Dataset.load_netflix(tiny_path)
    app = cfk.ALSApp(4, k, 0.05, iters, 426, 302, precision=precision, seed=42).setup(ds)
    app.run()
    return ds, app


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_app_similar_end_to_end(gpu, tiny_path, precision):
    ds, app = _tiny_app(gpu, tiny_path, precision)
    U, M = app.factors()                                                # ascending raw ids
    movie_ids, user_ids = ds.ids(SIDE_MOVIE), ds.ids(SIDE_USER)
    pos = np.arange(len(movie_ids))
    want_idx, want_score = ref.expected_lists(ref.similar_scores(M, pos, pos, "cosine"), pos, pos, 10, True)
    ids, nb, score = app.similar_movies()
    assert np.array_equal(ids, movie_ids) and nb.dtype == np.int64
    assert np.array_equal(nb, movie_ids[want_idx]) and np.array_equal(score, want_score)
    # a few users by raw id, out of order and one twice; dot product, self included
    some = user_ids[[200, 3, 3, 57]]
    upos, allu = np.searchsorted(user_ids, some), np.arange(len(user_ids))
    want_idx, want_score = ref.expected_lists(ref.similar_scores(U, upos, allu, "dot"), upos, allu, 4, False)
    ids, nb, score = app.similar_users(some, top_n=4, metric="dot", exclude_self=False)
    assert np.array_equal(ids, some) and np.array_equal(nb, user_ids[want_idx]) and np.array_equal(score, want_score)
    with pytest.raises(ValueError, match="unknown movie id"):
        app.similar_movies([int(movie_ids[0]), int(movie_ids.max()) + 1])


def _cli(tiny_path, out, *flags):
    app_bin = os.path.join(ROOT, "collaborative-filtering-kafka_amd", "build", "als_app")
    res = subprocess.run([app_bin, "4", "10", "0.05", "2", tiny_path, "426", "302", "--gpus", "1", "--out", str(out),
                          *flags], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return sorted(os.listdir(out))


def test_cli_similar_and_no_matrix(gpu, tiny_path, tmp_path):
    files = _cli(tiny_path, tmp_path / "sim", "--similar", "3", "--no-matrix")
    assert len(files) == 1 and files[0].startswith("similar_")           # no prediction_matrix_* file
    lines = [ln.split(",") for ln in (tmp_path / "sim" / files[0]).read_text().splitlines()]
    _, app = _tiny_app(gpu, tiny_path, "f32")
    ids, nb, score = app.similar_movies(top_n=3)
    assert len(lines) == 3 * len(ids)
    assert [(int(a), int(b)) for a, b, _ in lines] == [(int(ids[i]), int(nb[i, j])) for i in range(len(ids)) for j in range(3)]
    assert [np.float32(float(s)) for _, _, s in lines] == [score[i, j] for i in range(len(ids)) for j in range(3)]
