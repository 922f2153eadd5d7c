"""CPU side of the sharded serving tests (no kernel launch): the native slot layout against its numpy restatement
(sharded_ref.slots) for every case of sharded_ref.CASES, with the chunk counts set the way ALSApp.setup sets them, and the
proof that the poison test_gpu_sharded_serving.py puts into the padding slots would be noticed.

Ids come from the oracle's own parser of the sample file, never from the dataset under test.
"""
import numpy as np
import pytest

import sharded_ref as sr
from test_gpu_recommend import expected_topn
from test_host import java_float_dots

SIDE_MOVIE, SIDE_USER = 0, 1
K, LAM, ITERS, SEED = 10, 0.05, 2, 42


@pytest.fixture(scope="module")
def sample(oracle_mod, tiny_path):
    """(movie ids, user ids) ascending, and the by-id factors (U, M) of the serving tests' configuration (f32, k = 10,
    2 iterations, seed 42) from the CPU oracle."""
    m, u, r = oracle_mod.parse_netflix(tiny_path)
    U, M = oracle_mod.run_als(oracle_mod.build_blocks(m, u, r, 4), K, LAM, ITERS, seed=SEED, precision="f32")
    ids = [np.unique(m).astype(np.int64), np.unique(u).astype(np.int64)]
    assert len(ids[SIDE_MOVIE]) == 426 and len(ids[SIDE_USER]) == 302
    return ids, np.asarray(U, np.float32), np.asarray(M, np.float32)


def _dataset(cfk, tiny_path, case):
    """A Dataset of its own with the chunk counts ALSApp.setup stores for this case."""
    _, cu, cm = case
    ds = cfk.Dataset.load_netflix(tiny_path)
    ds.set_slot_chunks(SIDE_USER, cu)
    ds.set_slot_chunks(SIDE_MOVIE, cm)
    return ds


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: "G{}-u{}-m{}".format(*c))
def test_native_layout_equals_the_restatement(cfk, tiny_path, sample, case):
    G, cu, cm = case
    ids, _, _ = sample
    ds = _dataset(cfk, tiny_path, case)
    for side, C in ((SIDE_MOVIE, cm), (SIDE_USER, cu)):
        want, Sc, n_slots = sr.slots(ids[side], G, C)
        assert np.array_equal(ds.ids(side), ids[side])
        assert np.array_equal(ds.slots(side, G), want)
        assert ds.slot_layout(side, G) == (Sc, C)
        shard_sizes = np.bincount(ids[side] % G, minlength=G)
        for rank in range(G):
            info = ds.shard_info(side, G, rank)
            assert info["n_slots"] == n_slots == C * G * Sc
            assert info["n_rows"] == shard_sizes[rank] and info["row_offset"] == rank * Sc
        pad = sr.padding(want, n_slots)
        assert len(pad) >= 1 and len(pad) == n_slots - len(ids[side])       # every case pads both tables
        assert len(np.unique(want)) == len(want) and want.min() >= 0 and want.max() < n_slots


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: "G{}-u{}-m{}".format(*c))
def test_shard_user_rows_partition_the_user_slots(cfk, tiny_path, sample, case):
    G, cu, _ = case
    ids, _, _ = sample
    ds = _dataset(cfk, tiny_path, case)
    want, _, _ = sr.slots(ids[SIDE_USER], G, cu)
    rows = [cfk.shard_user_rows(ds, G, rank) for rank in range(G)]
    for rank in range(G):
        assert rows[rank].dtype == np.int64
        assert np.array_equal(rows[rank], want[ids[SIDE_USER] % G == rank])      # local-row order = ascending raw id
    assert np.array_equal(np.sort(np.concatenate(rows)), np.sort(want))          # a permutation of the user slots


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: "G{}-u{}-m{}".format(*c))
def test_a_padding_slot_among_the_candidates_would_be_noticed(sample, case):
    """One padding slot of the poisoned movie table listed as a candidate (in place of the movie at that position) is
    every user's best movie under the numpy top-N the GPU tests compare with: an index that lands on a padding slot
    cannot go unnoticed. Without it the same lists hold real movies only."""
    G, _, cm = case
    ids, U, M = sample
    slot, _, n_slots = sr.slots(ids[SIDE_MOVIE], G, cm)
    table = sr.scatter(M, slot, n_slots)
    pad = sr.padding(slot, n_slots)
    assert np.all(table[pad] == np.float32(sr.POISON)) and np.array_equal(table[slot], M)
    at = 211                                                  # neither the first nor the last position
    cand = slot.copy()
    cand[at] = pad[0]
    idx, score = expected_topn(java_float_dots(U, table[cand]), 10)
    clean_idx, clean_score = expected_topn(java_float_dots(U, table[slot]), 10)
    assert np.all(idx[:, 0] == at) and not np.all(clean_idx[:, 0] == at)
    assert np.all(clean_score < 1e3) and np.all(score[:, 0] > 1e20)          # real scores are ratings, the poison is not
