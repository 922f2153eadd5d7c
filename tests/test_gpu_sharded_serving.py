"""ALSApp's serving calls on sharded, chunk-major factor tables (world_size > 1), every result against numpy.

Part A, in one process. exchange="none" needs no process group and no serving method issues a collective, so one process
stands in for every rank: for each case of sharded_ref.CASES and each rank an app is set up on a Dataset of its own, and
the replicas the all-gathers would have produced are written into it from given factors -- U_id, M_id of a one-rank app
trained on the same ratings -- through sharded_ref.scatter, which puts 1e30 into every slot no entity owns. The spare
user rows and the sentinel stay as setup left them. Every expected value is numpy on U_id / M_id and the raw ratings
(java_float_dots, expected_topn, similar_ref, _numpy_evaluation, the fp64 oracles), never a result of the code under
test; the slots come from sharded_ref.slots, which test_sharded_host.py holds equal to the native layout.

Two worlds are built: the whole tiny sample (3,415 ratings) for everything but evaluate, and the training part of
test_gpu_rank's tiny_split for evaluate, whose probe would otherwise consist of training ratings only. Both rate the same
302 users and 426 movies, so the layouts are the same.

The implicit-feedback solve adds the Gram of the whole movie table, summed in table-row order. On the replica that sum
would depend on the layout (measured before ALSApp._solve_implicit_users: 20 of 40 words of the four rows differed from
the one-rank rows at G = 2, 18 at G = 3, 1.1e-6 relative) and would read the padding slots; the app now solves against
the movies gathered in ascending id, and fold_in_implicit is held to the one-rank bits with the poison in place.

No user of the sample has rated more than 426 - 64 movies, so recommend() never pads here; the -1 / -inf padding is
reached through recommend_for, whose fourth user has rated all but three movies.

Tolerances: _close of test_gpu_rank.py (n 2^-53, relative) for the double sums that the ranks add in another order, and
rowshapes.BOUND for the fold-in rows against the fp64 oracles. Everything else is array_equal.

Part B, one spawned run: two ranks on cuda:0 with gloo carrying the all-gathers (as test_gpu_parity.py's sharded test),
G = 2 with 3 user chunks; each rank saves what it serves after app.run() and the parent compares it with numpy.

Measured on an MI355X: fold-in rows against the fp64 oracle 1.2e-6 at most (explicit) and 1.0e-6 (implicit), bound 1e-4;
the double sums of evaluate agree with numpy's to the last bit or two. The module takes 6 s, 4 s of it the spawned run.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import implicit_ref as ir
import rowshapes as rs
import sharded_ref as sr
import similar_ref as sim
from test_gpu_rank import _close, _numpy_evaluation, tiny_split  # noqa: F401  (tiny_split: a fixture)
from test_gpu_recommend import expected_topn
from test_host import java_float_dots

pytestmark = pytest.mark.gpu

SIDE_MOVIE, SIDE_USER = 0, 1
K, LAM, ITERS, SEED = 10, 0.05, 2, 42
N_MOVIES, N_USERS, SPARE = 426, 302, 3
ALPHA = 40.0
CASE_IDS = ["G{}-u{}-m{}".format(*c) for c in sr.CASES]


@pytest.fixture(scope="module")
def gpu(cfk):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return cfk


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def new_users(movie_ids, variant=0):
    """Four users that are not in the data, as (movie id, rating) lists: one with an unknown movie id among known ones,
    one that lists a movie twice, one without any known movie, one that has rated all but three movies (fewer eligible
    movies than any top_n used here). variant shifts the ratings."""
    mid = [int(x) for x in movie_ids]
    unknown = max(mid) + 7
    r = lambda i: 1 + (i + variant) % 5                                                         # noqa: E731
    return [[(mid[3], r(4)), (unknown, r(3)), (mid[200], r(0)), (mid[77], r(2)), (mid[425], r(1))],
            [(mid[10], r(3)), (mid[11], r(1)), (mid[10], r(4)), (mid[300], r(2))],
            [(unknown, r(2)), (unknown + 1, r(4))],
            [(m, r(i)) for i, m in enumerate(mid) if i not in (0, 100, 424)]]


def user_queries(movie_ids, users):
    """(q_ptr, q_idx, q_ratings) with q_idx = positions in the ascending movie ids, unknown ids skipped, and the
    exclusion CSR (ascending positions, each once) -- from a dictionary."""
    pos_of = {int(m): i for i, m in enumerate(movie_ids)}
    known = [[(pos_of[m], r) for m, r in u if m in pos_of] for u in users]
    q_ptr = np.zeros(len(users) + 1, np.int64)
    q_ptr[1:] = np.cumsum([len(x) for x in known])
    q_idx = np.array([p for x in known for p, _ in x], np.int32)
    q_rat = np.array([r for x in known for _, r in x], np.int16)
    seen = [sorted({p for p, _ in x}) for x in known]
    e_ptr = np.zeros(len(users) + 1, np.int64)
    e_ptr[1:] = np.cumsum([len(x) for x in seen])
    return (q_ptr, q_idx, q_rat), (e_ptr, np.array([p for x in seen for p in x], np.int32))


def seen_csr(movie_ids, user_ids, m, u):
    """Per user (ascending id) the ascending positions of the movies of its raw (movie, user) pairs."""
    ui, mi = np.searchsorted(user_ids, u), np.searchsorted(movie_ids, m)
    key = np.unique(ui.astype(np.int64) * len(movie_ids) + mi)
    ptr = np.zeros(len(user_ids) + 1, np.int64)
    np.cumsum(np.bincount(key // len(movie_ids), minlength=len(user_ids)), out=ptr[1:])
    return ptr, (key % len(movie_ids)).astype(np.int32)


class _Ids:
    """What _numpy_evaluation asks of a dataset: the ascending ids of both sides."""

    def __init__(self, movie_ids, user_ids):
        self._ids = {SIDE_MOVIE: movie_ids, SIDE_USER: user_ids}

    def ids(self, side):
        return self._ids[side]


class World:
    """One set of ratings: the one-rank baseline app, its factors by id, and per case one sharded app per rank that
    holds those factors as poisoned replicas. References are computed once and kept."""

    def __init__(self, cfk, ratings):
        self.cfk = cfk
        self.m, self.u, self.r = (np.asarray(a) for a in ratings)
        self.movie_ids = np.unique(self.m).astype(np.int64)
        self.user_ids = np.unique(self.u).astype(np.int64)
        assert len(self.movie_ids) == N_MOVIES and len(self.user_ids) == N_USERS
        self.base = self._app(0, 1, 4, None, "torch")
        self.base.run()
        self.U, self.M = self.base.factors()
        assert self.U.dtype == np.float32 and self.U.shape == (N_USERS, K) and self.M.shape == (N_MOVIES, K)
        assert np.all(np.isfinite(self.U)) and np.all(np.isfinite(self.M)) and np.abs(self.M).max() < 1e3
        self.S = java_float_dots(self.U, self.M)
        self.seen = seen_csr(self.movie_ids, self.user_ids, self.m, self.u)
        self.users = new_users(self.movie_ids)
        self.queries, self.user_excl = user_queries(self.movie_ids, self.users)
        self.X = self.base.fold_in(self.users)
        self.X_implicit = self.base.fold_in_implicit(self.users, ALPHA)
        self._apps, self._topn, self._similar = {}, {}, {}

    def _app(self, rank, G, cu, cm, exchange):
        ds = self.cfk.Dataset.from_ratings(self.m, self.u, self.r)        # one Dataset per app: setup stores the chunks
        app = self.cfk.ALSApp(4, K, LAM, ITERS, N_MOVIES, N_USERS, precision="f32", seed=SEED, rank=rank, world_size=G,
                              overlap_chunks=cu, movie_chunks=cm, exchange=exchange)
        return app.setup(ds, spare_user_rows=SPARE)

    def layout(self, case):
        """(user slots, n user slots, movie slots, n movie slots) of a case, restated."""
        G, cu, cm = case
        us, _, nu = sr.slots(self.user_ids, G, cu)
        ms, _, nm = sr.slots(self.movie_ids, G, cm)
        return us, nu, ms, nm

    def apps(self, case):
        if case not in self._apps:
            G, cu, cm = case
            us, nu, ms, nm = self.layout(case)
            out = []
            for rank in range(G):
                app = self._app(rank, G, cu, cm, "none")
                assert app.info[SIDE_USER]["n_slots"] == nu and app.info[SIDE_MOVIE]["n_slots"] == nm
                assert raw_table(app, SIDE_USER).shape[0] == nu + SPARE + 1
                assert raw_table(app, SIDE_MOVIE).shape[0] == nm + 1
                assert not raw_table(app, SIDE_USER)[nu:].any() and not raw_table(app, SIDE_MOVIE)[nm:].any()
                app.engine.write_factors(SIDE_USER, sr.scatter(self.U, us, nu, sr.POISON))
                app.engine.write_factors(SIDE_MOVIE, sr.scatter(self.M, ms, nm, sr.POISON))
                assert not raw_table(app, SIDE_USER)[nu:].any() and not raw_table(app, SIDE_MOVIE)[nm:].any()
                out.append(app)
            self._apps[case] = out
        return self._apps[case]

    def topn(self, n, exclude_seen):
        key = (n, exclude_seen)
        if key not in self._topn:
            self._topn[key] = expected_topn(self.S, n, self.seen if exclude_seen else None)
        return self._topn[key]

    def similar_movies(self, metric, exclude_self):
        key = (metric, exclude_self)
        if key not in self._similar:
            pos = np.arange(N_MOVIES)
            self._similar[key] = sim.expected_lists(sim.similar_scores(self.M, pos, pos, metric), pos, pos, 10,
                                                    exclude_self)
        return self._similar[key]


def raw_table(app, side):
    """The whole device table of a side, padded columns, spare rows and the sentinel included."""
    app.engine.synchronize()
    return app.engine.factors[side].cpu().numpy()


def to_ids(ids, idx):
    return np.where(idx >= 0, ids[np.maximum(idx, 0)], -1).astype(np.int64)


@pytest.fixture(scope="module")
def full(gpu, oracle_mod, tiny_path):
    return World(gpu, oracle_mod.parse_netflix(tiny_path))


@pytest.fixture(scope="module")
def split(gpu, tiny_split):
    return World(gpu, tiny_split[0])


# ---------------------------------------------------------------------------------------------------------------------
# A: factors, prediction matrix, recommend
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_factors_and_prediction_matrix(full, case):
    us, nu, ms, nm = full.layout(case)
    assert len(sr.padding(us, nu)) >= 1 and len(sr.padding(ms, nm)) >= 1
    for app in full.apps(case):
        U, M = app.factors()
        assert np.array_equal(bits(U), bits(full.U)) and np.array_equal(bits(M), bits(full.M))
        P = app.prediction_matrix()
        assert P.dtype == np.float32 and np.array_equal(P, full.S)


@pytest.mark.parametrize("exclude_seen", [True, False], ids=["unseen", "all"])
@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_recommend(full, case, exclude_seen):
    G = case[0]
    for top_n in (1, 10, 64):
        got = [app.recommend(top_n, exclude_seen=exclude_seen) for app in full.apps(case)]
        for rank, (uid, _, _) in enumerate(got):
            assert np.array_equal(uid, full.user_ids[full.user_ids % G == rank])      # its own users, ascending
        uid = np.concatenate([g[0] for g in got])
        order = np.argsort(uid, kind="stable")
        assert np.array_equal(uid[order], full.user_ids)
        mid = np.concatenate([g[1] for g in got])[order]
        score = np.concatenate([g[2] for g in got])[order]
        want_idx, want_score = full.topn(top_n, exclude_seen)
        assert mid.dtype == np.int64 and np.array_equal(mid, to_ids(full.movie_ids, want_idx))
        assert np.array_equal(bits(score), bits(want_score))
        assert np.array_equal(mid == -1, np.isneginf(score))


# ---------------------------------------------------------------------------------------------------------------------
# A: similar
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude_self", [True, False], ids=["others", "self"])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_similar_movies(full, case, metric, exclude_self):
    want_idx, want_score = full.similar_movies(metric, exclude_self)
    got = [app.similar_movies(None, 10, metric, exclude_self) for app in full.apps(case)]
    for ids, nb, score in got:
        assert np.array_equal(ids, full.movie_ids)
        assert nb.dtype == np.int64 and np.array_equal(nb, to_ids(full.movie_ids, want_idx))
        assert np.array_equal(bits(score), bits(want_score))
    for other in got[1:]:                                                          # every rank the same answer
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], other))


@pytest.mark.parametrize("exclude_self", [True, False], ids=["others", "self"])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_similar_users(full, case, metric, exclude_self):
    G = case[0]
    by_shard = [full.user_ids[full.user_ids % G == s] for s in range(G)]
    some = np.array([sh[j] for j in (40, 0, -1) for sh in reversed(by_shard)] + [by_shard[0][40]], np.int64)
    assert set((some % G).tolist()) == set(range(G)) and len(np.unique(some)) == len(some) - 1     # one id twice
    pos, everyone = np.searchsorted(full.user_ids, some), np.arange(N_USERS)
    want_idx, want_score = sim.expected_lists(sim.similar_scores(full.U, pos, everyone, metric), pos, everyone, 7,
                                              exclude_self)
    bad = int(full.user_ids.max()) + G + 1
    for app in full.apps(case):
        ids, nb, score = app.similar_users(some, 7, metric, exclude_self)
        assert np.array_equal(ids, some) and np.array_equal(nb, to_ids(full.user_ids, want_idx))
        assert np.array_equal(bits(score), bits(want_score))
        with pytest.raises(ValueError, match=f"unknown user id {bad}$"):
            app.similar_users([int(some[0]), bad, int(some[1])], 7, metric, exclude_self)


# ---------------------------------------------------------------------------------------------------------------------
# A: evaluate
# ---------------------------------------------------------------------------------------------------------------------
EXACT = ("n", "n_unknown", "n_seen", "n_ranked", "hr_sum")


def check_evaluation(per_rank, G, movie_ids, user_ids, S, train, probe, exclude_seen, top_n=10):
    """The ranks' evaluate() results, added up, against _numpy_evaluation on the dense score matrix S."""
    ref = _numpy_evaluation(_Ids(movie_ids, user_ids), S, train, probe, exclude_seen)
    err, rank, elig = np.array(ref["err"]), np.array(ref["rank"], np.float64), np.array(ref["elig"], np.float64)
    hit = rank < top_n
    want = {"n": len(err), "n_unknown": ref["n_unknown"], "n_seen": ref["n_seen"], "n_ranked": len(rank),
            "hr_sum": int(np.count_nonzero(hit)), "se": float(np.sum(err * err)), "ae": float(np.sum(np.abs(err))),
            "mrr_sum": float(np.sum(1 / (rank + 1))), "ndcg_sum": float(np.sum(np.where(hit, 1 / np.log2(rank + 2), 0))),
            "mpr_sum": float(np.sum(rank / np.maximum(1, elig - 1)))}
    assert want["n_unknown"] == 3 and want["n_seen"] == 2 and want["n"] == 739
    assert 0 < want["hr_sum"] < want["n_ranked"] == (737 if exclude_seen else 739)
    total = {key: sum(res[key] for res in per_rank) for key in want}
    print(f"\n[sharded evaluate] G={G} exclude_seen={exclude_seen}: " +
          ", ".join(f"{key} {total[key]!r} / {want[key]!r}" for key in want))
    for key in EXACT:
        assert total[key] == want[key], key
    for key in ("se", "ae"):
        assert _close(total[key], want[key], want["n"]), key
    for key in ("mrr_sum", "ndcg_sum", "mpr_sum"):
        assert want[key] > 0 and _close(total[key], want[key], want["n_ranked"]), key
    # every pair is counted by the rank its user id maps to, and by no other
    pm, pu, _ = probe
    unknown = ~np.isin(pu, user_ids) | ~np.isin(pm, movie_ids)
    assert np.count_nonzero(unknown) == want["n_unknown"]
    for r, res in enumerate(per_rank):
        assert res["n_unknown"] == np.count_nonzero(unknown & (pu % G == r)), r
        assert res["n"] == np.count_nonzero(~unknown & (pu % G == r)), r
        assert res["top_n"] == top_n


@pytest.mark.parametrize("exclude_seen", [True, False], ids=["unseen", "all"])
@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_evaluate(split, tiny_split, case, exclude_seen):
    train, probe = tiny_split
    got = [app.evaluate(*probe, top_n=10, exclude_seen=exclude_seen) for app in split.apps(case)]
    check_evaluation(got, case[0], split.movie_ids, split.user_ids, split.S, train, probe, exclude_seen)


# ---------------------------------------------------------------------------------------------------------------------
# A: fold-in
# ---------------------------------------------------------------------------------------------------------------------
def check_fold_rows(name, X, ref64):
    rel = rs.row_errors(X, ref64)
    print(f"\n[sharded {name}] per-row errors against fp64 {rel}")
    assert X.shape == (4, K) and X.dtype == np.float32
    assert (rel <= rs.BOUND["f32"]).all() and not X[2].any() and X[[0, 1, 3]].any(axis=1).all()


def explicit_oracle(oracle_mod, queries, M):
    side = oracle_mod.Side(np.arange(1, len(queries[0]), dtype=np.int64), queries[0].copy(), queries[1].copy(),
                           queries[2].copy())
    return oracle_mod.update_side(side, np.asarray(M, np.float64), LAM, "f64")


@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_fold_in(full, oracle_mod, case):
    assert np.array_equal(np.diff(full.queries[0]), [4, 4, 0, N_MOVIES - 3])
    check_fold_rows("fold_in", full.X, explicit_oracle(oracle_mod, full.queries, full.M))
    for app in full.apps(case):
        before = raw_table(app, SIDE_USER)
        X = app.fold_in(full.users)
        assert np.array_equal(bits(X), bits(full.X))                                # the one-rank app's rows
        assert np.array_equal(bits(raw_table(app, SIDE_USER)), bits(before))        # no dst_rows: nothing written


@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_fold_in_implicit(full, case):
    """The one-rank app's rows bit for bit on every rank, with the poison in both tables' padding slots; those rows within
    the bound of the fp64 oracle."""
    ref64 = ir.solve_rows(full.queries, full.M.astype(np.float64), LAM, ALPHA)
    check_fold_rows("fold_in_implicit", full.X_implicit, ref64)
    assert not np.array_equal(full.X_implicit, full.X)
    for app in full.apps(case):
        before = [raw_table(app, s) for s in (SIDE_MOVIE, SIDE_USER)]
        X = app.fold_in_implicit(full.users, ALPHA)
        assert X.dtype == np.float32 and np.array_equal(bits(X), bits(full.X_implicit))
        for s in (SIDE_MOVIE, SIDE_USER):                                       # no dst_rows: nothing written
            assert np.array_equal(bits(raw_table(app, s)), bits(before[s]))


# ---------------------------------------------------------------------------------------------------------------------
# A: recommend_for
# ---------------------------------------------------------------------------------------------------------------------
def check_recommend_for(app, world, case, X, exclude_seen, implicit_alpha=None):
    """One recommend_for call of four users through three spare rows: the lists, the spare rows afterwards (the second
    batch, user 3, has reused row 0; rows 1 and 2 keep users 1 and 2) and every other row of both tables."""
    us, nu, ms, nm = world.layout(case)
    u_before, m_before = raw_table(app, SIDE_USER), raw_table(app, SIDE_MOVIE)
    mids, score = app.recommend_for(world.users, 5, exclude_seen=exclude_seen, implicit_alpha=implicit_alpha)
    want_idx, want_score = expected_topn(java_float_dots(X, world.M), 5, world.user_excl if exclude_seen else None)
    assert mids.dtype == np.int64 and np.array_equal(mids, to_ids(world.movie_ids, want_idx))
    assert np.array_equal(bits(score), bits(want_score))
    if exclude_seen:
        assert np.all(mids[3, :3] >= 0) and np.all(mids[3, 3:] == -1) and np.all(np.isneginf(score[3, 3:]))
        assert np.all(mids[2] >= 0) and not score[2].any()                  # no known movie: zeros, nothing excluded
    u_after = raw_table(app, SIDE_USER)
    assert np.array_equal(bits(u_after[nu:nu + SPARE, :K]), bits(X[[3, 1, 2]]))
    assert not u_after[nu:nu + SPARE, K:].any()
    others = np.setdiff1d(np.arange(len(u_after)), nu + np.arange(SPARE))
    assert np.array_equal(bits(u_after[others]), bits(u_before[others]))   # entity rows, poisoned padding, sentinel
    assert not u_after[-1].any() and np.all(u_after[sr.padding(us, nu), :K] == np.float32(sr.POISON))
    assert np.array_equal(bits(raw_table(app, SIDE_MOVIE)), bits(m_before))


@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_recommend_for(full, case):
    for app in full.apps(case):
        for exclude_seen in (True, False):
            check_recommend_for(app, full, case, full.X, exclude_seen)
        check_recommend_for(app, full, case, full.X_implicit, True, implicit_alpha=ALPHA)


# ---------------------------------------------------------------------------------------------------------------------
# A: what is not built raises, and the self-check
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_implicit_training_is_refused_when_sharded(full, case):
    for app in full.apps(case):
        before = [raw_table(app, s) for s in (SIDE_MOVIE, SIDE_USER)]
        for call in (lambda: app.implicit_half(SIDE_USER, ALPHA), lambda: app.implicit_half("movie", ALPHA),
                     lambda: app.implicit_iteration(ALPHA), lambda: app.implicit_objective(ALPHA),
                     lambda: app.implicit_loss(ALPHA), lambda: app.implicit_fit(ALPHA, 2)):
            with pytest.raises(NotImplementedError):
                call()
        for s in (SIDE_MOVIE, SIDE_USER):
            assert np.array_equal(bits(raw_table(app, s)), bits(before[s]))


@pytest.mark.parametrize("case", sr.CASES, ids=CASE_IDS)
def test_verify_replicas_without_a_process_group(full, case):
    import torch.distributed as dist
    assert not dist.is_initialized()
    got = [app.verify_replicas() for app in full.apps(case)]
    for res in got:
        assert res["replicas_agree"] is True and res["integrity_clean"] is True and res["integrity_failures"] == 0
        assert res["digest"] == got[0]["digest"]                            # the ranks were given the same replicas
    assert got[0]["digest"] != full.base.verify_replicas()["digest"]        # and the digest reads the tables


# ---------------------------------------------------------------------------------------------------------------------
# B: one real sharded run, two ranks on one GPU
# ---------------------------------------------------------------------------------------------------------------------
B_WORLD, B_CHUNKS = 2, 3
EVAL_KEYS = ("n", "n_unknown", "n_seen", "n_ranked", "hr_sum", "se", "ae", "mrr_sum", "ndcg_sum", "mpr_sum", "top_n")


def _serving_worker(rank, world, port, in_path, out_dir):
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import __graft_entry__
    cfk = __graft_entry__.load_package()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        inp = np.load(in_path)
        ds = cfk.Dataset.from_ratings(inp["tm"], inp["tu"], inp["tr"])
        app = cfk.ALSApp(4, K, LAM, ITERS, N_MOVIES, N_USERS, precision="f32", seed=SEED, device=0, rank=rank,
                         world_size=world, overlap_chunks=B_CHUNKS)
        app.setup(ds, spare_user_rows=SPARE)
        app.run()
        users = new_users(np.unique(inp["tm"]), variant=rank)              # its own users: the spare rows are local
        U, M = app.factors()
        rec = app.recommend(10)
        simm = app.similar_movies(None, 5)
        ev = app.evaluate(inp["pm"], inp["pu"], inp["pr"], top_n=10)
        X = app.fold_in(users)
        Xi = app.fold_in_implicit(users, ALPHA)
        rf = app.recommend_for(users, 5)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), U=U, M=M, rec_uid=rec[0], rec_mid=rec[1], rec_score=rec[2],
                 sim_ids=simm[0], sim_nb=simm[1], sim_score=simm[2], ev=np.array([ev[key] for key in EVAL_KEYS], np.float64),
                 X=X, Xi=Xi, rf_mid=rf[0], rf_score=rf[1], u_table=raw_table(app, SIDE_USER), m_table=raw_table(app, SIDE_MOVIE))
    finally:
        dist.destroy_process_group()


def test_sharded_run_serves_what_numpy_computes(gpu, oracle_mod, tiny_split, tmp_path):
    import socket
    import torch.multiprocessing as mp
    (tm, tu, tr), probe = tiny_split
    in_path = str(tmp_path / "inputs.npz")
    np.savez(in_path, tm=tm, tu=tu, tr=tr, pm=probe[0], pu=probe[1], pr=probe[2])
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_serving_worker, args=(B_WORLD, port, in_path, str(tmp_path)), nprocs=B_WORLD, join=True)
    res = [np.load(os.path.join(tmp_path, f"rank{rank}.npz")) for rank in range(B_WORLD)]
    U, M = res[0]["U"], res[0]["M"]
    assert U.dtype == np.float32 and U.shape == (N_USERS, K) and M.shape == (N_MOVIES, K) and U.any() and M.any()
    assert np.array_equal(bits(res[1]["U"]), bits(U)) and np.array_equal(bits(res[1]["M"]), bits(M))
    movie_ids, user_ids = np.unique(tm).astype(np.int64), np.unique(tu).astype(np.int64)
    S = java_float_dots(U, M)
    # recommend
    for rank in range(B_WORLD):
        assert np.array_equal(res[rank]["rec_uid"], user_ids[user_ids % B_WORLD == rank])
    order = np.argsort(np.concatenate([r["rec_uid"] for r in res]), kind="stable")
    want_idx, want_score = expected_topn(S, 10, seen_csr(movie_ids, user_ids, tm, tu))
    assert np.array_equal(np.concatenate([r["rec_mid"] for r in res])[order], to_ids(movie_ids, want_idx))
    assert np.array_equal(bits(np.concatenate([r["rec_score"] for r in res])[order]), bits(want_score))
    # similar movies
    pos = np.arange(N_MOVIES)
    want_idx, want_score = sim.expected_lists(sim.similar_scores(M, pos, pos, "cosine"), pos, pos, 5, True)
    for r in res:
        assert np.array_equal(r["sim_ids"], movie_ids) and np.array_equal(r["sim_nb"], to_ids(movie_ids, want_idx))
        assert np.array_equal(bits(r["sim_score"]), bits(want_score))
    # evaluate
    evs = [dict(zip(EVAL_KEYS, r["ev"].tolist())) for r in res]
    check_evaluation(evs, B_WORLD, movie_ids, user_ids, S, (tm, tu, tr), probe, True)
    # fold-in and recommend_for, per rank its own users; the tables
    us, _, nu = sr.slots(user_ids, B_WORLD, B_CHUNKS)
    ms, _, nm = sr.slots(movie_ids, B_WORLD, 1)
    assert len(sr.padding(us, nu)) >= 1 and len(sr.padding(ms, nm)) >= 1
    for rank, r in enumerate(res):
        queries, excl = user_queries(movie_ids, new_users(movie_ids, variant=rank))
        X = r["X"]
        check_fold_rows(f"fold_in, rank {rank} of the run", X, explicit_oracle(oracle_mod, queries, M))
        check_fold_rows(f"fold_in_implicit, rank {rank} of the run", r["Xi"],
                        ir.solve_rows(queries, M.astype(np.float64), LAM, ALPHA))
        want_idx, want_score = expected_topn(java_float_dots(X, M), 5, excl)
        assert np.array_equal(r["rf_mid"], to_ids(movie_ids, want_idx))
        assert np.array_equal(bits(r["rf_score"]), bits(want_score))
        ut, mt = r["u_table"], r["m_table"]
        assert ut.shape[0] == nu + SPARE + 1 and mt.shape[0] == nm + 1
        assert np.array_equal(bits(ut[us, :K]), bits(U)) and np.array_equal(bits(mt[ms, :K]), bits(M))
        assert not ut[sr.padding(us, nu)].any() and not mt[sr.padding(ms, nm)].any()       # never written
        assert not ut[-1].any() and not mt[-1].any()                                         # the sentinels
        assert np.array_equal(bits(ut[nu:nu + SPARE, :K]), bits(X[[3, 1, 2]])) and not ut[nu:nu + SPARE, K:].any()
    assert not np.array_equal(res[0]["X"], res[1]["X"])                    # two ranks, two sets of spare rows
