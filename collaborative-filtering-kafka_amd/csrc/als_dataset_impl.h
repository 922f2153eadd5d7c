// als_dataset_impl.h -- the dataset of the host data layer (include/als_host.h) and what its translation units share:
// als_dataset.cpp (lifetime, Netflix-format ingest, the plain queries), als_dataset_synth.cpp (the synthetic
// generators) and als_dataset_shard.cpp (id % G sharding into slot order, in-blocks, seeded U0). Private to csrc/.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "als_error.h"
#include "als_host.h"

struct als_dataset {
    // arrival order (the producer's send order, NetflixDataFormatProducer.java:58)
    std::vector<int32_t> movie, user;
    std::vector<int16_t> rating;
    // derived
    std::vector<int64_t> ids[2];      // ascending raw ids per side (0 = movie, 1 = user)
    std::vector<int32_t> dense[2];    // per rating: dense (ascending-id rank) index of its movie / user
    int chunks[2] = {1, 1};           // chunk-major slot layout per side (als_dataset_set_slot_chunks)
    // a shard-restricted synthetic dataset (als_dataset_synthetic_powerlaw_shard) holds only the ratings of its
    // shard's in-blocks, so U0's rating means come from every user's full rating sum, kept here (per dense user)
    std::vector<int64_t> user_sum, user_cnt;
};

namespace cfk_detail {

inline bool check_side(int side) { return side == 0 || side == 1; }

// The arguments of a query about shard `shard` of `side` under n_shards shards (a query about all shards: shard 0).
inline bool check_shard_args(const als_dataset* ds, int side, int n_shards, int64_t shard = 0) {
    return ds && check_side(side) && n_shards >= 1 && shard >= 0 && shard < n_shards;
}

// Shard geometry of one side under G shards and C chunks (als_host.h "Slot layout"): entity i of shard
// sh = id % G with rank r among that shard's ids (ascending) sits at slot (r / Sc) * (G * Sc) + sh * Sc + r % Sc,
// Sc = ceil(S / C), S = the largest shard. C = 1: slot = sh * S + r (shard-major).
struct ShardMap {
    int G = 1, C = 1;
    int64_t S = 0;                        // rows of the largest shard
    int64_t Sc = 0;                       // slots per shard and chunk
    std::vector<int64_t> slot;            // per dense entity
    std::vector<int32_t> shard;           // per dense entity
    std::vector<int64_t> local;           // per dense entity: its row in its shard's block (= rank)
    std::vector<int64_t> count;           // entities per shard
    int64_t n_slots() const { return (int64_t)C * G * Sc; }
};

inline ShardMap shard_map(const als_dataset* ds, int side, int G) {
    ShardMap m;
    m.G = G;
    m.C = ds->chunks[side];
    const auto& ids = ds->ids[side];
    m.count.assign(G, 0);
    m.slot.resize(ids.size());
    m.shard.resize(ids.size());
    m.local.resize(ids.size());
    for (size_t i = 0; i < ids.size(); ++i) {
        const int sh = (int)(ids[i] % G);   // PureModStreamPartitioner.java:10
        m.shard[i] = sh;
        m.local[i] = m.count[sh]++;
    }
    m.S = 0;
    for (int64_t c : m.count) m.S = std::max(m.S, c);
    m.Sc = (m.S + m.C - 1) / m.C;
    for (size_t i = 0; i < ids.size(); ++i) {
        const int64_t r = m.local[i];
        m.slot[i] = (r / m.Sc) * ((int64_t)G * m.Sc) + (int64_t)m.shard[i] * m.Sc + r % m.Sc;
    }
    return m;
}

inline uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

struct Rng {   // xoshiro256** seeded by splitmix64
    uint64_t s[4];
    explicit Rng(uint64_t seed) {
        for (auto& w : s) w = seed = mix64(seed);
    }
    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    uint64_t next() {
        const uint64_t r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
        s[2] ^= s[0];
        s[3] ^= s[1];
        s[1] ^= s[2];
        s[0] ^= s[3];
        s[2] ^= t;
        s[3] = rotl(s[3], 45);
        return r;
    }
    double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    uint64_t below(uint64_t n) { return (uint64_t)(((__uint128_t)next() * n) >> 64); }
};

}  // namespace cfk_detail
