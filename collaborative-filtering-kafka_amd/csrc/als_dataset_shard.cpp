// als_dataset_shard.cpp -- host data layer, the shard and slot geometry (als_dataset_impl.h: ShardMap): id % G sharding
// into slot order, a shard's in-blocks as CSR or arrival-order COO, and the seeded U0.
#include "als_dataset_impl.h"

using namespace cfk_detail;

extern "C" {

float als_u01(uint64_t seed, int64_t raw_id, int32_t feature) {
    const uint64_t h = mix64(seed ^ mix64((uint64_t)raw_id * 0x100000001B3ULL + (uint64_t)(uint32_t)feature));
    return (float)(h >> 40) * (1.0f / 16777216.0f);
}

int als_dataset_shard_info(const als_dataset* ds, int side, int n_shards, int shard, int64_t* n_rows,
                           int64_t* row_offset, int64_t* nnz, int64_t* slots_per_shard, int64_t* n_slots) {
    if (!check_shard_args(ds, side, n_shards, shard)) return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    const ShardMap m = shard_map(ds, side, n_shards);
    int64_t z = 0;
    const auto& raw = side == 0 ? ds->movie : ds->user;
    for (int32_t v : raw) z += (v % n_shards) == shard;
    if (n_rows) *n_rows = m.count[shard];
    if (row_offset) *row_offset = shard * m.Sc;
    if (nnz) *nnz = z;
    if (slots_per_shard) *slots_per_shard = m.Sc * m.C;
    if (n_slots) *n_slots = m.n_slots();
    return ALS_OK;
}

int als_dataset_set_slot_chunks(als_dataset* ds, int side, int n_chunks) {
    if (!ds || !check_side(side) || n_chunks < 1) return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    ds->chunks[side] = n_chunks;
    return ALS_OK;
}

int als_dataset_slot_layout(const als_dataset* ds, int side, int n_shards, int64_t* slots_per_chunk, int* n_chunks) {
    if (!check_shard_args(ds, side, n_shards)) return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    const ShardMap m = shard_map(ds, side, n_shards);
    if (slots_per_chunk) *slots_per_chunk = m.Sc;
    if (n_chunks) *n_chunks = m.C;
    return ALS_OK;
}

int als_dataset_shard_block(const als_dataset* ds, int side, int n_shards, int64_t shard, int64_t* row_ptr,
                            int32_t* col_idx, int16_t* ratings, int64_t* row_ids) {
    if (!check_shard_args(ds, side, n_shards, shard) || !row_ptr) return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    const int opp = 1 - side;
    const ShardMap ms = shard_map(ds, side, n_shards);
    const ShardMap mo = shard_map(ds, opp, n_shards);
    const int64_t nr = ms.count[shard];
    const auto& dn = ds->dense[side];
    const auto& dop = ds->dense[opp];
    const int64_t n = (int64_t)dn.size();
    // stable counting sort of arrival order by local row: in-block order = arrival order
    std::fill(row_ptr, row_ptr + nr + 1, 0);
    for (int64_t t = 0; t < n; ++t)
        if (ms.shard[dn[t]] == shard) ++row_ptr[ms.local[dn[t]] + 1];
    for (int64_t i = 0; i < nr; ++i) row_ptr[i + 1] += row_ptr[i];
    if (col_idx || ratings) {
        std::vector<int64_t> pos(row_ptr, row_ptr + nr);
        for (int64_t t = 0; t < n; ++t) {
            if (ms.shard[dn[t]] != shard) continue;
            const int64_t p = pos[ms.local[dn[t]]]++;
            if (col_idx) col_idx[p] = (int32_t)mo.slot[dop[t]];
            if (ratings) ratings[p] = ds->rating[t];
        }
    }
    if (row_ids) {
        const auto& ids = ds->ids[side];
        for (size_t i = 0; i < ids.size(); ++i)
            if (ms.shard[i] == shard) row_ids[ms.local[i]] = ids[i];
    }
    return ALS_OK;
}

int als_dataset_shard_coo(const als_dataset* ds, int side, int n_shards, int64_t shard, int32_t* rows,
                          int32_t* cols, int16_t* ratings) {
    if (!check_shard_args(ds, side, n_shards, shard) || !rows || !cols || !ratings)
        return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    const int opp = 1 - side;
    const ShardMap ms = shard_map(ds, side, n_shards);
    const ShardMap mo = shard_map(ds, opp, n_shards);
    const auto& dn = ds->dense[side];
    const auto& dop = ds->dense[opp];
    const int64_t n = (int64_t)dn.size();
    int64_t p = 0;
    for (int64_t t = 0; t < n; ++t) {   // arrival order: the order the block builder sees the ratings
        if (ms.shard[dn[t]] != shard) continue;
        rows[p] = (int32_t)ms.local[dn[t]];
        cols[p] = (int32_t)mo.slot[dop[t]];
        ratings[p] = ds->rating[t];
        ++p;
    }
    return ALS_OK;
}

int als_dataset_slots(const als_dataset* ds, int side, int n_shards, int64_t* slot_of) {
    if (!check_shard_args(ds, side, n_shards) || !slot_of) return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    const ShardMap m = shard_map(ds, side, n_shards);
    std::copy(m.slot.begin(), m.slot.end(), slot_of);
    return ALS_OK;
}

int als_dataset_init_user_factors(const als_dataset* ds, int num_features, uint64_t seed, int n_shards, float* out,
                                  int64_t ld, int64_t n_out_rows) {
    if (!ds || num_features < 1 || n_shards < 1 || !out || ld < num_features)
        return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    const ShardMap m = shard_map(ds, 1, n_shards);
    if (n_out_rows < m.n_slots()) return fail(ALS_ERR_INVALID_ARGUMENT, "output has too few rows");
    std::fill(out, out + n_out_rows * ld, 0.f);
    const int64_t nu = (int64_t)ds->ids[1].size();
    std::vector<int64_t> sum(nu, 0), cnt(nu, 0);
    if (!ds->user_cnt.empty()) {   // shard-restricted synthetic data: the full sums were kept at generation
        sum = ds->user_sum;
        cnt = ds->user_cnt;
    } else {
        for (size_t t = 0; t < ds->rating.size(); ++t) {
            sum[ds->dense[1][t]] += ds->rating[t];
            ++cnt[ds->dense[1][t]];
        }
    }
    for (int64_t u = 0; u < nu; ++u) {
        float* f = out + m.slot[u] * ld;
        // DoubleStream.average() (exact for short ratings) cast to float; orElse(1.0)
        const double mean = cnt[u] > 0 ? (double)sum[u] / (double)cnt[u] : 1.0;
        f[0] = (float)mean;
        for (int c = 1; c < num_features; ++c) f[c] = als_u01(seed, ds->ids[1][u], c);
    }
    return ALS_OK;
}

}  // extern "C"
