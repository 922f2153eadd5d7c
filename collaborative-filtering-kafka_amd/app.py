"""ALSApp: the reference topology's iteration semantics on 1..G GPUs (one process per GPU).

Reference: apps/ALSApp.java:41-48 (configuration), :115-163 (the unrolled ALS loop),
processors/UFeatureInitializer.java:36-66 (U0 after the EOF barrier), processors/FeatureCollector.java:72-110.

Bulk-synchronous restatement: U0 -> for i in 0..N-1 { M_i = solve(movies | U_i); U_{i+1} = solve(users | M_i) }.
The reference fires each entity's solve as soon as its last factor row arrives (MFeatureCalculator.java:65);
every solve of a half depends only on the previous half's factors, so the results are identical.
Final output = (U_N, M_{N-1}) as in the reference's movie-features-N / user-features-N topics.

Multi-GPU: entities are sharded by raw id % G (PureModStreamPartitioner.java:9-10 with numPartitions = G,
equal to (id % P) % G when G divides P). Every rank holds its shard's in-blocks and a full replica of both
factor matrices in slot order; each half-iteration ends with ONE RCCL all-gather (torch.distributed, backend
"nccl" = RCCL over xGMI) of the updated shard -- the replacement for the feature topics' block-to-block
fan-out (ALSApp.java:105-148, README.md:157).
"""
from __future__ import annotations

import time

import numpy as np
import torch

from .engine import ALSEngine, Dataset, SIDE_MOVIE, SIDE_USER, SIDES


def _table_digest(t: torch.Tensor) -> int:
    """Bitwise digest of a factor table (all rows incl. the sentinel): sum over its 32-bit words w_i of
    w_i * (2 i + 1) * 0x9E3779B1 in wrapping int64 -- any change of one word changes it."""
    w = t.detach().contiguous().view(torch.int32).flatten().to(torch.int64)
    i = torch.arange(w.numel(), dtype=torch.int64, device=w.device)
    return int((w * ((2 * i + 1) * 0x9E3779B1)).sum().item())


def shard_user_rows(ds: Dataset, world: int, rank: int) -> np.ndarray:
    """Factor rows (slots) of rank `rank`'s users in local-row order (ascending raw id), under the chunk-major slot
    layout: local row i -> row_offset + (i // Sc) G Sc + i % Sc (include/als_host.h "Slot layout")."""
    info = ds.shard_info(SIDE_USER, world, rank)
    i = np.arange(info["n_rows"], dtype=np.int64)
    sc, nc = ds.slot_layout(SIDE_USER, world)
    return (info["row_offset"] + ((i // sc) * (world * sc) + i % sc if nc > 1 else i)).astype(np.int64)


def seen_exclusions(ds: Dataset, world: int, rank: int, movie_rows) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """What ALSEngine.recommend needs to leave out the movies a user has already rated. For rank `rank`'s users in
    local-row order (ascending raw id): (user_factor_rows, excl_ptr, excl_idx), excl_idx[excl_ptr[i]:excl_ptr[i + 1]]
    = the positions in `movie_rows` (movie factor rows = slots, any subset, repeats allowed) of user i's rated movies,
    ascending; rated movies outside the candidate set are dropped. Pure host code; the factor rows honour the
    chunk-major slot layout (shard_user_rows)."""
    blk = ds.shard_block(SIDE_USER, world, rank)
    n = blk["n_rows"]
    i = np.arange(n, dtype=np.int64)
    rows = shard_user_rows(ds, world, rank)
    mr = np.ascontiguousarray(movie_rows, np.int64)
    order = np.argsort(mr, kind="stable")              # positions grouped by slot: the inverse of movie_rows
    by_slot = mr[order]
    col = blk["col"].astype(np.int64)
    lo = np.searchsorted(by_slot, col, "left")
    cnt = np.searchsorted(by_slot, col, "right") - lo    # 0: not a candidate; > 1: the slot is listed several times
    user = np.repeat(np.repeat(i, np.diff(blk["row_ptr"])), cnt)
    start = np.cumsum(cnt) - cnt
    pos = order[np.repeat(lo, cnt) + (np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(start, cnt))]
    keep = np.lexsort((pos, user))                       # ascending position inside every user
    excl_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(user, minlength=n), out=excl_ptr[1:])
    return rows, excl_ptr, pos[keep].astype(np.int32)


def ids_to_slots(ds: Dataset, side: int, world: int, ids) -> np.ndarray:
    """Factor rows (slots under `world` shards) of the entities of `side` with the given raw ids, in the order given;
    repeats allowed. Raises ValueError naming the first id that is not in `ds`. Pure host code."""
    want = np.ascontiguousarray(ids, np.int64).reshape(-1)
    known = ds.ids(side)                                        # ascending
    at = np.minimum(np.searchsorted(known, want), max(len(known) - 1, 0))
    bad = np.nonzero(known[at] != want)[0] if len(known) else np.arange(len(want))
    if len(bad):
        raise ValueError(f"unknown {'user' if side == SIDE_USER else 'movie'} id {int(want[bad[0]])}")
    return ds.slots(side, world)[at].astype(np.int64)


def heldout_queries(ds: Dataset, movie_ids, user_ids, world: int, rank: int, movie_rows):
    """What ALSEngine.rank_targets needs to evaluate held-out (movie id, user id) pairs. For rank `rank`'s users in
    shard_user_rows order (ascending raw id): (tgt_ptr, tgt_idx, entry, seen, n_unknown, n_seen).
    tgt_idx[tgt_ptr[i]:tgt_ptr[i + 1]] = the positions in `movie_rows` (movie factor rows = slots, any subset, repeats
    allowed: a slot listed several times is taken at its first position) of user i's held-out movies, in input order;
    entry[t] = the index of the input pair behind target t. Only pairs of this rank's shard (user id % world == rank)
    are looked at. n_unknown of them are skipped: the user or the movie is not in `ds`, or the movie is not in
    `movie_rows`. seen[t] marks the n_seen targets that are also training ratings of that user: they keep their score
    but a caller that excludes seen movies leaves them out of the ranks. Pure host code."""
    mid = np.ascontiguousarray(movie_ids, np.int64)
    uid = np.ascontiguousarray(user_ids, np.int64)
    if mid.shape != uid.shape or mid.ndim != 1:
        raise ValueError("movie_ids and user_ids must be one-dimensional and of equal length")
    blk = ds.shard_block(SIDE_USER, world, rank)
    mine = np.asarray(blk["row_ids"], np.int64)               # ascending raw id = local-row order
    all_movies = ds.ids(SIDE_MOVIE)
    slot_of = ds.slots(SIDE_MOVIE, world)
    mr = np.ascontiguousarray(movie_rows, np.int64)
    order = np.argsort(mr, kind="stable")                     # stable: the first position of a repeated slot first
    by_slot = mr[order]
    own = np.nonzero(uid % world == rank)[0] if world > 1 else np.arange(len(uid), dtype=np.int64)
    u, m = uid[own], mid[own]
    ui = np.minimum(np.searchsorted(mine, u), max(len(mine) - 1, 0))
    mi = np.minimum(np.searchsorted(all_movies, m), max(len(all_movies) - 1, 0))
    known = (mine[ui] == u if len(mine) else np.zeros(len(u), bool)) & \
        (all_movies[mi] == m if len(all_movies) else np.zeros(len(u), bool))
    slot = slot_of[mi] if len(all_movies) else np.zeros(len(u), np.int64)
    at = np.minimum(np.searchsorted(by_slot, slot, "left"), max(len(mr) - 1, 0))
    known &= (by_slot[at] == slot) if len(mr) else False
    pos = order[at] if len(mr) else np.zeros(len(u), np.int64)
    own, ui, pos, slot = own[known], ui[known], pos[known], slot[known]
    keep = np.argsort(ui, kind="stable")                      # by user, input order inside a user
    own, ui, pos, slot = own[keep], ui[keep], pos[keep], slot[keep]
    tgt_ptr = np.zeros(len(mine) + 1, np.int64)
    np.cumsum(np.bincount(ui, minlength=len(mine)), out=tgt_ptr[1:])
    # seen: (local row, movie slot) is an entry of this shard's user in-block
    n_slots = int(slot_of.max()) + 1 if len(slot_of) else 1
    rated = np.repeat(np.arange(len(mine), dtype=np.int64), np.diff(blk["row_ptr"])) * n_slots + blk["col"].astype(np.int64)
    seen = np.isin(ui * n_slots + slot, rated)
    return tgt_ptr, pos.astype(np.int32), own.astype(np.int64), seen, int(len(u) - len(own)), int(seen.sum())


def foldin_queries(ds: Dataset, world: int, movie_rows, users):
    """What ALSEngine.fold_in and a following ALSEngine.recommend need for users that are not in `ds`. users: one
    sequence of (movie id, rating) pairs per new user. Returns (q_ptr, q_idx, q_ratings, excl_ptr, excl_idx, n_unknown):
    q_idx[q_ptr[i]:q_ptr[i + 1]] = the movie factor rows (slots under `world` shards) of user i's rated movies with their
    ratings, in input order (a movie listed twice counts twice, as als_set_block would count it); n_unknown pairs are
    skipped because their movie is not in `ds`, and a user with no known movie keeps an empty range (fold-in gives the
    zero vector). excl_idx[excl_ptr[i]:excl_ptr[i + 1]] = the positions in `movie_rows` (movie factor rows, any subset,
    repeats allowed: every position of a repeated slot) of those movies, strictly ascending: the exclusion list that
    keeps recommend from returning what the user has rated; rated movies outside `movie_rows` are dropped from it.
    Pure host code."""
    n = len(users)
    pairs = [np.asarray(u, np.int64).reshape(-1, 2) for u in users]
    cnt = np.array([len(p) for p in pairs], np.int64)
    allp = np.concatenate(pairs) if n else np.zeros((0, 2), np.int64)
    user = np.repeat(np.arange(n, dtype=np.int64), cnt)
    mid, rat = allp[:, 0], allp[:, 1]
    if len(rat) and (rat.min() < -32768 or rat.max() > 32767):
        raise ValueError("ratings must fit a Java short")
    all_movies = ds.ids(SIDE_MOVIE)
    slot_of = ds.slots(SIDE_MOVIE, world)
    mi = np.minimum(np.searchsorted(all_movies, mid), max(len(all_movies) - 1, 0))
    known = all_movies[mi] == mid if len(all_movies) else np.zeros(len(mid), bool)
    user, slot, rat = user[known], (slot_of[mi[known]] if len(all_movies) else np.zeros(0, np.int64)), rat[known]
    q_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(user, minlength=n), out=q_ptr[1:])
    mr = np.ascontiguousarray(movie_rows, np.int64)
    order = np.argsort(mr, kind="stable")              # positions grouped by slot: the inverse of movie_rows
    by_slot = mr[order]
    lo = np.searchsorted(by_slot, slot, "left")
    c = np.searchsorted(by_slot, slot, "right") - lo     # 0: not a candidate; > 1: the slot is listed several times
    eu = np.repeat(user, c)
    start = np.cumsum(c) - c
    pos = order[np.repeat(lo, c) + (np.arange(int(c.sum()), dtype=np.int64) - np.repeat(start, c))]
    key = np.unique(eu * max(len(mr), 1) + pos)          # ascending position inside every user, each once
    eu, pos = key // max(len(mr), 1), key % max(len(mr), 1)
    excl_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(eu, minlength=n), out=excl_ptr[1:])
    return (q_ptr, slot.astype(np.int32), rat.astype(np.int16), excl_ptr, pos.astype(np.int32),
            int(len(known) - int(known.sum())))


def ranking_metrics(rank, n_eligible, top_n: int) -> dict:
    """Ranking quality from exact 0-based ranks (ALSEngine.rank_targets), pure numpy in float64: HR@N = mean(rank < N),
    NDCG@N = mean(1 / log2(rank + 2) where rank < N, else 0), MRR = mean(1 / (rank + 1)), MPR = mean(rank /
    max(1, n_eligible - 1)) with n_eligible per target = the candidates its user may be recommended (n_movies minus the
    user's exclusions). Returns the means ("hr", "ndcg", "mrr", "mpr"; nan without targets), "n_ranked" and the sums
    ("hr_sum", ...), which add across ranks."""
    r = np.asarray(rank, np.float64)
    ne = np.broadcast_to(np.asarray(n_eligible, np.float64), r.shape)
    hit = r < top_n
    sums = {"hr_sum": float(np.count_nonzero(hit)),
            "ndcg_sum": float(np.sum(np.where(hit, 1.0 / np.log2(r + 2.0), 0.0))),
            "mrr_sum": float(np.sum(1.0 / (r + 1.0))),
            "mpr_sum": float(np.sum(r / np.maximum(1.0, ne - 1.0)))}
    n = int(r.size)
    out = {"n_ranked": n, **sums}
    for key in ("hr", "ndcg", "mrr", "mpr"):
        out[key] = sums[key + "_sum"] / n if n else float("nan")
    return out


class ALSApp:
    # a movie factor table above this is exchanged in chunks (N > 1): configs[4]'s 256 MB item table (all-gather ~1.7 ms
    # at G = 8), not the 9 MB k = 128 Netflix one -- its 4 chunk launches cost more in launch tails than the overlap of a
    # ~0.1 ms all-gather saves (one rank's k = 128 movie half at G = 2: 7.2 ms in 4 launches vs 5.4 ms in one,
    # profiles/r06a)
    MOVIE_CHUNK_BYTES = 64 << 20

    def __init__(self, num_partitions: int, num_features: int, als_lambda: float, num_als_iterations: int,
                 num_movies: int | None = None, num_users: int | None = None, *, precision: str = "f32",
                 seed: int = 42, device: int = 0, rank: int = 0, world_size: int = 1, group=None,
                 overlap_chunks: int = 4, exchange: str = "torch", movie_chunks: int | None = None):
        self.NUM_PARTITIONS = num_partitions
        self.NUM_FEATURES = num_features
        self.ALS_LAMBDA = float(np.float32(als_lambda))     # Float.parseFloat (ALSAppRunner.java:19)
        self.NUM_ALS_ITERATIONS = num_als_iterations
        self.NUM_MOVIES = num_movies
        self.NUM_USERS = num_users
        self.precision = precision
        self.seed = seed
        self.device = device
        self.rank = rank
        self.world = world_size
        self.group = group
        self.engine = None
        self.ds = None
        self.info = [None, None]
        # user half on > 1 GPU: solve in `overlap_chunks` row ranges and all-gather each range while the
        # next one is solved (1 = one launch, then one all-gather)
        self.overlap_chunks = max(1, int(overlap_chunks))
        # movie half on > 1 GPU: the same chunked exchange once the movie table is large (None: overlap_chunks
        # chunks when the movie factor table exceeds MOVIE_CHUNK_BYTES, e.g. configs[4]'s 1M items; 1 = unchunked)
        self.movie_chunks = None if movie_chunks is None else max(1, int(movie_chunks))
        self.chunk_slots = [None, None]   # per side: chunk indices of a chunked half, or None
        # "torch": torch.distributed collectives on the factor tensors (backend "nccl" = RCCL); "native": the
        # engine's own RCCL communicator through the C ABI (als_comm_init / als_allgather_shard), the path a
        # JNI caller uses. The rendezvous (sharing the RCCL unique id) uses the torch process group either way.
        # "none": no exchange at all -- one rank of a sharded run timed alone (its halves, not the all-gathers).
        if exchange not in ("torch", "native", "none"):
            raise ValueError("exchange must be 'torch', 'native' or 'none'")
        self.exchange = exchange

    # -------------------------------------------------------------------------------------------------
    def setup(self, ds: Dataset, check_duplicates: bool = True, engine_factory=None,
              block_build: str = "device", spare_user_rows: int = 0) -> "ALSApp":
        """Blocks of this rank's shard + factor replicas + U0 (UFeatureInitializer after the EOF barrier).

        spare_user_rows > 0: that many extra rows of U after all shard slots (and before the sentinel), zero until
        fold_in / recommend_for put users there that are not in `ds`. They are local to this rank: no half solves them
        and no all-gather covers them.

        ``engine_factory(k, precision, device)`` replaces the HIP engine with another object of the same
        interface; only the multi-rank CPU rehearsal tests (gloo) use it, to exercise the sharding and the
        all-gather on machines without a GPU. The product path is always the HIP engine."""
        nm, nu, nnz = ds.counts()
        if self.NUM_MOVIES is not None and (nm, nu) != (self.NUM_MOVIES, self.NUM_USERS):
            raise ValueError(f"NUM_MOVIES/NUM_USERS = {self.NUM_MOVIES}/{self.NUM_USERS} but the dataset rates "
                             f"{nm} movies and {nu} users (the reference collector would never fire, "
                             f"FeatureCollector.java:43)")
        if check_duplicates and ds.count_duplicates():
            raise ValueError("duplicate (user, movie) pairs: the reference never completes such an entity "
                             "(MFeatureCalculator.java:65)")
        self.ds = ds
        # user half on > 1 GPU in `overlap_chunks` row ranges: chunk-major user slots (include/als_host.h "Slot
        # layout"), so each range's exchange is one contiguous all-gather; the movie half too once its table is big
        kp = (self.NUM_FEATURES + 15) // 16 * 16
        if self.world == 1:
            n_chunks = [1, 1]
        else:
            mc = self.movie_chunks
            if mc is None:
                mc = self.overlap_chunks if nm * kp * 4 > self.MOVIE_CHUNK_BYTES else 1
            n_chunks = [mc, self.overlap_chunks]
        ds.set_slot_chunks(SIDE_USER, n_chunks[SIDE_USER])
        ds.set_slot_chunks(SIDE_MOVIE, n_chunks[SIDE_MOVIE])
        def new_engine():
            if engine_factory is None:
                torch.cuda.set_device(self.device)
                eng = ALSEngine(self.NUM_FEATURES, self.precision, self.device)
            else:
                eng = engine_factory(self.NUM_FEATURES, self.precision, self.device)
            eng.use_torch_stream()
            return eng
        self._new_engine = new_engine
        self._by_id_engine = None
        eng = new_engine()
        self.spare_user_rows = max(0, int(spare_user_rows))
        spare = [0, self.spare_user_rows]                   # per side: rows after the shard slots
        for side in (SIDE_MOVIE, SIDE_USER):
            opp = ds.shard_info(1 - side, self.world, self.rank)
            n_opp = opp["n_slots"] + spare[1 - side]            # the sentinel row follows the spare rows
            if block_build == "device" and hasattr(eng, "set_block_coo"):
                # block builders on the GPU: arrival-order COO -> stable radix sort by row (als_set_block_coo)
                blk = ds.shard_coo(side, self.world, self.rank)
                eng.alloc_factors(side, blk["n_slots"] + spare[side])
                eng.set_block_coo(side, blk["n_rows"], blk["rows"], blk["cols"], blk["ratings"], blk["row_offset"],
                                  n_opp)
            else:
                blk = ds.shard_block(side, self.world, self.rank)
                eng.alloc_factors(side, blk["n_slots"] + spare[side])
                eng.set_block(side, blk["row_ptr"], blk["col"], blk["ratings"], blk["row_offset"], n_opp)
            sc, nc = ds.slot_layout(side, self.world)
            blk["slots_per_chunk"], blk["n_chunks"] = sc, nc
            if nc > 1:
                eng.set_row_layout(side, sc, self.world * sc)
            self.info[side] = {k: blk[k] for k in ("n_rows", "row_offset", "nnz", "slots_per_shard", "n_slots",
                                                   "slots_per_chunk", "n_chunks")}
        for side in (SIDE_MOVIE, SIDE_USER):
            nc = self.info[side]["n_chunks"]
            if nc > 1:
                sc, n = self.info[side]["slots_per_chunk"], self.info[side]["n_rows"]
                # chunk c = this rank's local rows [c Sc, (c+1) Sc) = factor rows [c G Sc + rank Sc, + Sc)
                self.chunk_slots[side] = list(range(nc))
                eng.set_chunks(side, [min(c * sc, n) for c in range(nc)] + [n])
        u0 = ds.init_user_factors(self.NUM_FEATURES, self.seed, self.world)
        eng.write_factors(SIDE_USER, u0)
        if self.exchange == "native" and self.world > 1:
            import torch.distributed as dist
            uid = [eng.comm_unique_id() if self.rank == 0 else None]
            dist.broadcast_object_list(uid, src=0, group=self.group)
            eng.comm_init(self.world, self.rank, uid[0])
        self.engine = eng
        self.nnz_total = nnz
        return self

    # -------------------------------------------------------------------------------------------------
    def _stream_ordered(self) -> bool:
        """RCCL ("nccl") orders its kernels after the work already queued on the current stream. gloo on CUDA
        tensors reads them with host-side copies, so the engine's stream is drained before each collective."""
        import torch.distributed as dist
        if not hasattr(self, "_ordered"):
            self._ordered = dist.get_backend(self.group) == "nccl"
        return self._ordered

    def _allgather(self, side: int, chunk: int = 0):
        """Exchange chunk `chunk` of `side` (the whole shard when the side is unchunked): one all-gather of the G
        ranks' Sc-row pieces, which are contiguous in the chunk-major slot layout."""
        if self.world == 1 or self.exchange == "none":   # "none": one rank's work alone (bench.py --shard-of)
            return
        sc = self.info[side]["slots_per_chunk"]
        if self.exchange == "native":
            self.engine.allgather_shard(side, sc, chunk)
            return
        import torch.distributed as dist
        if not self._stream_ordered():
            self.engine.synchronize()
        full = self.engine.factors[side]            # [n_slots + 1, kp]: last row = sentinel, not exchanged
        base = chunk * self.world * sc
        return dist.all_gather_into_tensor(full[base:base + self.world * sc],
                                           full[base + self.rank * sc:base + (self.rank + 1) * sc],
                                           group=self.group, async_op=True)

    def _half(self, side):
        if self.chunk_slots[side] is None:
            self.engine.solve_half(side, self.ALS_LAMBDA)
            w = self._allgather(side)
            if w is not None:
                w.wait()
            return
        # chunk c's all-gather (RCCL, ordered after chunk c's solve on the stream) overlaps chunk c+1's solve
        works = []
        for c in self.chunk_slots[side]:
            self.engine.solve_half_chunk(side, self.ALS_LAMBDA, c)
            works.append(self._allgather(side, c))
        for w in works:
            if w is not None:
                w.wait()

    def movie_half(self):
        """MFeatureCalculator-i over this rank's movies + all-gather (movie-features-i topic)."""
        self._half(SIDE_MOVIE)

    def user_half(self):
        """UFeatureCalculator-i over this rank's users + all-gather (user-features-(i+1) topic)."""
        self._half(SIDE_USER)

    def iteration(self):
        self.movie_half()
        self.user_half()

    def run(self, iterations: int | None = None) -> float:
        n = self.NUM_ALS_ITERATIONS if iterations is None else iterations
        self.engine.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.iteration()
        self.engine.synchronize()
        return time.perf_counter() - t0

    # -------------------------------------------------------------------------------------------------
    def verify_replicas(self) -> dict:
        """Self-check of a sharded run (N > 1), after the exchange has settled: every rank's full replicas of both
        factor matrices must be bitwise identical (what the all-gathers promise: the reference's feature topics
        deliver the same rows to every partition, ALSApp.java:105-148), and every rank's partial-slot integrity
        record clean. One digest per side and rank -- a position-weighted int64 sum of the tables' 32-bit words --
        compared by MIN/MAX all-reduces. Returns {"replicas_agree", "integrity_clean", "digest": [movie, user],
        "integrity_failures"}; at N = 1 trivially true (one replica)."""
        self.engine.synchronize()
        # the shard slots only: spare user rows are rank-local (the all-zero sentinel adds nothing to the digest)
        digests = [_table_digest(self.engine.factors[s][:self.info[s]["n_slots"]]) for s in (SIDE_MOVIE, SIDE_USER)]
        bad = int(self.engine.integrity_status()[0]) if hasattr(self.engine, "integrity_status") else 0
        if self.world == 1 or self.exchange == "none":
            return {"replicas_agree": True, "integrity_clean": bad == 0, "digest": [f"{d:016x}" for d in digests],
                    "integrity_failures": bad}
        import torch.distributed as dist
        dev = "cpu" if dist.get_backend(self.group) == "gloo" else self.engine.factors[0].device
        t = torch.tensor(digests + [bad], dtype=torch.int64, device=dev)
        hi, lo = t.clone(), t.clone()
        dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=self.group)
        dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=self.group)
        agree = bool(torch.equal(hi[:2], lo[:2]))
        return {"replicas_agree": agree, "integrity_clean": int(hi[2]) == 0,
                "digest": [f"{d & 0xFFFFFFFFFFFFFFFF:016x}" for d in digests], "integrity_failures": int(hi[2])}

    def factors(self):
        """(U, M) in ascending raw-id order (FeatureCollector.constructFeatureMatrices, :72-88)."""
        U = self.engine.read_factors(SIDE_USER, 0, self.info[SIDE_USER]["n_slots"])
        M = self.engine.read_factors(SIDE_MOVIE)
        return U[self.ds.slots(SIDE_USER, self.world)], M[self.ds.slots(SIDE_MOVIE, self.world)]

    def prediction_matrix(self) -> np.ndarray:
        """FeatureCollector.calculatePredictionMatrix (FeatureCollector.java:90-101): users x movies, both in
        ascending id order, computed on the GPU from the (gathered) factor replicas."""
        return self.engine.predict(self.ds.slots(SIDE_USER, self.world), self.ds.slots(SIDE_MOVIE, self.world))

    def recommend(self, top_n: int, exclude_seen: bool = True) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Top-N movies of every user of this rank's shard against all movies, from the (gathered) factor replicas:
        (user_ids [n], movie_ids [n, top_n], scores [n, top_n]) in raw ids, users ascending, best first. Candidates are
        taken in ascending movie id, so equal scores go to the smaller movie id; movie id -1 / score -inf where a user
        has fewer than top_n eligible movies. exclude_seen leaves out the movies the user has rated. No collective:
        every rank answers for its own users."""
        movie_ids = self.ds.ids(SIDE_MOVIE)
        movie_rows = self.ds.slots(SIDE_MOVIE, self.world)       # ascending id -> factor row
        if exclude_seen:
            user_rows, excl_ptr, excl_idx = seen_exclusions(self.ds, self.world, self.rank, movie_rows)
            idx, score = self.engine.recommend(user_rows, movie_rows, top_n, (excl_ptr, excl_idx))
        else:
            idx, score = self.engine.recommend(shard_user_rows(self.ds, self.world, self.rank), movie_rows, top_n)
        user_ids = self.ds.ids(SIDE_USER)
        if self.world > 1:
            user_ids = user_ids[user_ids % self.world == self.rank]
        out = np.where(idx >= 0, movie_ids[np.maximum(idx, 0)], -1)
        return user_ids, out.astype(np.int64), score

    def _similar(self, side, ids, top_n, metric, exclude_self):
        all_ids = self.ds.ids(side)
        cand_rows = self.ds.slots(side, self.world)              # ascending id -> factor row; no spare rows
        ids = all_ids if ids is None else np.ascontiguousarray(ids, np.int64).reshape(-1)
        idx, score = self.engine.similar(side, ids_to_slots(self.ds, side, self.world, ids), cand_rows, top_n, metric,
                                         exclude_self)
        return ids, np.where(idx >= 0, all_ids[np.maximum(idx, 0)], -1).astype(np.int64), score

    def similar_movies(self, movie_ids=None, top_n: int = 10, metric: str = "cosine",
                       exclude_self: bool = True) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The top_n nearest movies of the given movies (raw ids; None: every movie, ascending) by the cosine or the dot
        product of their factor rows (ALSEngine.similar): (ids [n], neighbour_ids [n, top_n], scores [n, top_n]), best
        first. Candidates are all movies in ascending id, so equal scores go to the smaller id; -1 / -inf where there
        are fewer than top_n. An unknown id raises ValueError. No collective: after the all-gather every rank holds the
        whole table and returns the same answer."""
        return self._similar(SIDE_MOVIE, movie_ids, top_n, metric, exclude_self)

    def similar_users(self, user_ids, top_n: int = 10, metric: str = "cosine",
                      exclude_self: bool = True) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """similar_movies for users: the nearest users of the given users among all users of the dataset (spare rows are
        not candidates)."""
        return self._similar(SIDE_USER, user_ids, top_n, metric, exclude_self)

    # ---- implicit feedback (Hu, Koren, Volinsky 2008): single rank --------------------------------------------------
    def _implicit_csr(self, side):
        """The side's whole host CSR (row_ptr, col = opposite factor rows, int16 ratings), taken once and kept."""
        if self.world > 1:
            raise NotImplementedError("implicit-feedback training is single-rank: G = Y^T Y is additive over shards, "
                                      "but the all-reduce of k x k per half is not built")
        if not hasattr(self, "_implicit_blocks"):
            self._implicit_blocks = [None, None]
        if self._implicit_blocks[side] is None:
            blk = self.ds.shard_block(side, 1, 0)
            self._implicit_blocks[side] = (np.ascontiguousarray(blk["row_ptr"], np.int64),
                                           np.ascontiguousarray(blk["col"], np.int32),
                                           np.ascontiguousarray(blk["ratings"], np.int16),
                                           int(blk["row_offset"]), int(blk["n_rows"]))
        return self._implicit_blocks[side]

    def implicit_half(self, side, alpha: float):
        """One half of implicit-feedback ALS: every row of `side` from its ratings (confidence 1 + alpha r) and the
        Gram of the whole opposite table, stored into the resident factors (ALSEngine.solve_implicit, this app's
        lambda as the plain lambda of the model)."""
        side = SIDES[side] if isinstance(side, str) else int(side)
        row_ptr, col, rat, row_offset, n_rows = self._implicit_csr(side)
        self.engine.solve_implicit(side, (row_ptr, col, rat), self.ALS_LAMBDA, alpha,
                                   dst_rows=row_offset + np.arange(n_rows, dtype=np.int64), return_host=False)

    def implicit_iteration(self, alpha: float):
        self.implicit_half(SIDE_MOVIE, alpha)
        self.implicit_half(SIDE_USER, alpha)

    def implicit_loss(self, alpha: float) -> float:
        """sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + lambda (|U|^2 + |M|^2) over the dense users x movies grid, c = 1 +
        alpha r, p = [r > 0]. Host-side and fp64, for small data: the grid is materialised."""
        row_ptr, col, rat, row_offset, n_rows = self._implicit_csr(SIDE_USER)
        U = self.engine.read_factors(SIDE_USER, 0, self.info[SIDE_USER]["n_slots"]).astype(np.float64)
        M = self.engine.read_factors(SIDE_MOVIE).astype(np.float64)
        R = np.zeros((U.shape[0], M.shape[0]))
        np.add.at(R, (row_offset + np.repeat(np.arange(n_rows), np.diff(row_ptr)), col), rat.astype(np.float64))
        us, ms = self.ds.slots(SIDE_USER, 1), self.ds.slots(SIDE_MOVIE, 1)
        U, M, R = U[us], M[ms], R[us][:, ms]
        err = (R > 0).astype(np.float64) - U @ M.T
        return float(np.sum((1.0 + alpha * R) * err * err) + self.ALS_LAMBDA * (np.sum(U * U) + np.sum(M * M)))

    def implicit_objective(self, alpha: float) -> dict:
        """The implicit-feedback loss of the current factors, on the device and without the grid
        (ALSEngine.implicit_objective over the cached user-side CSR, this app's lambda): {"quad", "observed", "ridge",
        "ridge_opp", "loss"}, "loss" being implicit_loss()'s number. One pass over the ratings plus k^2 per user; no
        factors are read back."""
        row_ptr, col, rat, row_offset, n_rows = self._implicit_csr(SIDE_USER)
        return self.engine.implicit_objective(SIDE_USER, (row_ptr, col, rat),
                                              row_offset + np.arange(n_rows, dtype=np.int64), self.ALS_LAMBDA, alpha)

    def implicit_fit(self, alpha: float, max_iterations: int, rel_tol: float = 0.0) -> list[float]:
        """Implicit-feedback training with a convergence check: the loss before training, then implicit_iteration() and
        the loss after each iteration, stopping after the first iteration whose drop prev - cur is <= rel_tol * prev (or
        after max_iterations). Returns the losses, the one before training first."""
        losses = [self.implicit_objective(alpha)["loss"]]
        for _ in range(int(max_iterations)):
            self.implicit_iteration(alpha)
            losses.append(self.implicit_objective(alpha)["loss"])
            if losses[-2] - losses[-1] <= rel_tol * losses[-2]:
                break
        return losses

    def _solve_implicit_users(self, queries, alpha: float, dst_rows, return_host: bool):
        """ALSEngine.solve_implicit for user queries (q_ptr, q_idx = movie factor rows under self.world, ratings).

        One rank: the engine's own movie table, whose rows are in ascending id. Sharded: the solve adds the Gram of the
        WHOLE movie table, which als_gram_table sums in table-row order, so on the chunk-major replica the result would
        depend on the layout in its last bits (and read the padding slots). The movies are therefore gathered in
        ascending id into the table of a second engine, kept for this purpose, which shares this engine's user table
        (dst_rows land in the same spare rows): the rows are bit for bit those of a one-rank app with the same factors.
        One gather of the movie table per call."""
        q_ptr, q_idx, q_rat = queries
        if self.world == 1:
            return self.engine.solve_implicit(SIDE_USER, (q_ptr, q_idx, q_rat), self.ALS_LAMBDA, alpha,
                                              dst_rows=dst_rows, return_host=return_host)
        movie_rows = self.ds.slots(SIDE_MOVIE, self.world)       # ascending id -> factor row
        if getattr(self, "_by_id_engine", None) is None:
            eng = self._new_engine()
            eng.alloc_factors(SIDE_MOVIE, len(movie_rows))
            eng.bind_factors(SIDE_USER, self.engine.factors[SIDE_USER])
            self._by_id_engine = eng
        eng = self._by_id_engine
        self.engine.synchronize()                                  # pending exchanges of the replica included
        table = self.engine.factors[SIDE_MOVIE]
        rows = torch.as_tensor(movie_rows, dtype=torch.int64, device=table.device)
        eng.factors[SIDE_MOVIE][:len(movie_rows)].copy_(table.index_select(0, rows))
        by_id = np.full(self.info[SIDE_MOVIE]["n_slots"], -1, np.int64)
        by_id[movie_rows] = np.arange(len(movie_rows), dtype=np.int64)
        return eng.solve_implicit(SIDE_USER, (q_ptr, by_id[np.asarray(q_idx, np.int64)], q_rat), self.ALS_LAMBDA, alpha,
                                  dst_rows=dst_rows, return_host=return_host)

    def fold_in_implicit(self, users, alpha: float, dst_rows=None) -> np.ndarray:
        """fold_in() under the implicit-feedback model: the users' factors from ALSEngine.solve_implicit against the
        resident movie factors; the same bits whatever the number of ranks (_solve_implicit_users)."""
        movie_rows = self.ds.slots(SIDE_MOVIE, self.world)
        q_ptr, q_idx, q_rat, _, _, _ = foldin_queries(self.ds, self.world, movie_rows, users)
        return self._solve_implicit_users((q_ptr, q_idx, q_rat), alpha, dst_rows, True)

    def fold_in(self, users, dst_rows=None) -> np.ndarray:
        """User factors [n, k] of users that are not in the training data, from their (movie id, rating) lists and the
        resident movie factors (ALSEngine.fold_in with this app's lambda; foldin_queries maps the movie ids and skips
        unknown ones; a user without a known movie gets zeros). dst_rows: rows of U that also receive them."""
        movie_rows = self.ds.slots(SIDE_MOVIE, self.world)
        q_ptr, q_idx, q_rat, _, _, _ = foldin_queries(self.ds, self.world, movie_rows, users)
        return self.engine.fold_in(SIDE_USER, (q_ptr, q_idx, q_rat), self.ALS_LAMBDA, dst_rows=dst_rows)

    def recommend_for(self, users, top_n: int, exclude_seen: bool = True,
                      implicit_alpha: float | None = None) -> tuple[np.ndarray, np.ndarray]:
        """Top-N movies for users that are not in the training data: their (movie id, rating) lists are folded into the
        spare rows of U (setup(spare_user_rows=...), as many users at a time as there are spare rows) and recommend()
        runs on those rows against all movies in ascending id. Returns (movie_ids [n, top_n], scores [n, top_n]) as
        ALSApp.recommend does; exclude_seen leaves out the movies a user has rated. implicit_alpha: fold in under the
        implicit-feedback model with that alpha (fold_in_implicit) instead of the explicit one."""
        if self.spare_user_rows < 1:
            raise ValueError("recommend_for needs spare user rows: setup(..., spare_user_rows=n)")
        movie_ids = self.ds.ids(SIDE_MOVIE)
        movie_rows = self.ds.slots(SIDE_MOVIE, self.world)       # ascending id -> factor row
        base = self.info[SIDE_USER]["n_slots"]
        n = len(users)
        out = np.full((n, top_n), -1, np.int64)
        score = np.full((n, top_n), -np.inf, np.float32)
        for u0 in range(0, n, self.spare_user_rows):
            part = users[u0:u0 + self.spare_user_rows]
            q_ptr, q_idx, q_rat, excl_ptr, excl_idx, _ = foldin_queries(self.ds, self.world, movie_rows, part)
            rows = base + np.arange(len(part), dtype=np.int64)
            if implicit_alpha is None:
                self.engine.fold_in(SIDE_USER, (q_ptr, q_idx, q_rat), self.ALS_LAMBDA, dst_rows=rows, return_host=False)
            else:
                self._solve_implicit_users((q_ptr, q_idx, q_rat), implicit_alpha, rows, False)
            idx, sc = self.engine.recommend(rows, movie_rows, top_n, (excl_ptr, excl_idx) if exclude_seen else None)
            out[u0:u0 + len(part)] = np.where(idx >= 0, movie_ids[np.maximum(idx, 0)], -1)
            score[u0:u0 + len(part)] = sc
        return out, score

    def evaluate(self, movie_ids, user_ids, ratings, top_n: int = 10, exclude_seen: bool = True,
                 ranks: bool = True) -> dict:
        """Held-out evaluation of the (movie id, user id, rating) triples that belong to this rank's users, from the
        (gathered) factor replicas and against all movies in ascending id (ALSEngine.rank_targets: exact scores, exact
        ranks under recommend()'s order). No collective: every rank answers for its own users and the sums add across
        ranks. Returns the sums se, ae (errors (double)r - (double)score, summed in float64) and n over the scored
        triples; n_unknown (user or movie not in the training data: skipped) and n_seen (also a training rating: scored,
        but with exclude_seen left out of the ranks); n_ranked and hr_sum, ndcg_sum, mrr_sum, mpr_sum over the ranked
        ones (ranking_metrics, n_eligible = the movies minus the user's seen ones); and the derived rmse, mae, hr, ndcg,
        mrr, mpr (nan where nothing was counted). ranks=False: errors only, no candidate sweep."""
        movie_rows = self.ds.slots(SIDE_MOVIE, self.world)       # ascending id -> factor row
        user_rows, excl_ptr, excl_idx = seen_exclusions(self.ds, self.world, self.rank, movie_rows)
        tgt_ptr, tgt_idx, entry, seen, n_unknown, n_seen = heldout_queries(self.ds, movie_ids, user_ids, self.world,
                                                                           self.rank, movie_rows)
        excl = (excl_ptr, excl_idx) if exclude_seen else None
        score, rank = self.engine.rank_targets(user_rows, movie_rows, (tgt_ptr, tgt_idx), excl, ranks=ranks)
        err = np.asarray(ratings, np.float64)[entry] - score.astype(np.float64)
        out = {"top_n": int(top_n), "se": float(np.sum(err * err)), "ae": float(np.sum(np.abs(err))), "n": int(len(err)),
               "n_unknown": n_unknown, "n_seen": n_seen}
        if ranks:
            counted = ~seen if exclude_seen else np.ones(len(seen), bool)
            n_excl = np.diff(excl_ptr) if exclude_seen else np.zeros(len(user_rows), np.int64)
            n_eligible = np.repeat(len(movie_rows) - n_excl, np.diff(tgt_ptr))
            out.update(ranking_metrics(rank[counted], n_eligible[counted], top_n))
        else:
            out.update(ranking_metrics(np.zeros(0), np.zeros(0), top_n))
        out["rmse"] = float(np.sqrt(out["se"] / out["n"])) if out["n"] else float("nan")
        out["mae"] = out["ae"] / out["n"] if out["n"] else float("nan")
        return out

    def sq_error(self):
        """Sum of squared errors over all observed ratings (all ranks) and the rating count."""
        se, cnt = self.engine.sq_error(SIDE_MOVIE)
        if self.world > 1:
            import torch.distributed as dist
            t = torch.tensor([se, float(cnt)], dtype=torch.float64, device=self.engine.factors[0].device)
            dist.all_reduce(t, group=self.group)
            se, cnt = float(t[0]), int(t[1])
        return se, cnt

    def mse(self) -> float:
        se, cnt = self.sq_error()
        return se / cnt
