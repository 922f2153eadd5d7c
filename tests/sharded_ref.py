"""The chunk-major slot layout of a sharded run ("Slot layout", include/als_host.h), restated in numpy.

Imports nothing from the package under test: test_sharded_host.py holds the native layout equal to slots(), and
test_gpu_sharded_serving.py builds with scatter() the factor tables every rank of a sharded run would hold after its
all-gathers -- with a poison value in every slot that no entity owns, so that a serving call that touched one shows.
"""
import numpy as np

# (G shards, user chunks, movie chunks). On the tiny golden sample (302 users, 426 movies) no shard's size is a multiple
# of its chunk count, so both tables of every case hold padding slots (asserted in test_sharded_host.py).
CASES = [(2, 1, 1), (2, 3, 1), (3, 4, 2)]
POISON = 1e30     # as a padding slot's factors it beats every real score (the factors are O(1), k = 10)


def slots(ids, G, C):
    """(slot of every id in the order given, Sc, n_slots) for G shards and C chunks: shard = id % G, r = the id's rank
    among its shard's ids (ascending), S = the largest shard, Sc = ceil(S / C), slot = (r // Sc) G Sc + shard Sc +
    r % Sc, n_slots = C G Sc."""
    ids = np.asarray(ids, np.int64)
    assert ids.ndim == 1 and len(np.unique(ids)) == len(ids)
    shard = ids % G
    r = np.zeros(len(ids), np.int64)
    for s in range(G):
        mine = np.nonzero(shard == s)[0]
        r[mine[np.argsort(ids[mine], kind="stable")]] = np.arange(len(mine))
    S = int(np.bincount(shard, minlength=G).max()) if len(ids) else 0
    Sc = -(-S // C)
    return (r // Sc) * (G * Sc) + shard * Sc + r % Sc, Sc, C * G * Sc


def scatter(F_by_id, slot, n_slots, poison=POISON):
    """[n_slots, k] table with row i of F_by_id at slot[i] and `poison` in every slot no entity owns."""
    F = np.asarray(F_by_id)
    slot = np.asarray(slot, np.int64)
    assert len(slot) == len(F) and len(np.unique(slot)) == len(slot) and slot.min() >= 0 and slot.max() < n_slots
    T = np.full((n_slots, F.shape[1]), poison, F.dtype)
    T[slot] = F
    return T


def padding(slot, n_slots):
    """The slots in [0, n_slots) that no entity owns, ascending."""
    return np.setdiff1d(np.arange(n_slots, dtype=np.int64), np.asarray(slot, np.int64))
