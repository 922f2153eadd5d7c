// als_engine_comm.cpp -- the multi-GPU exchange (RCCL over xGMI): communicators, caller-level groups and the per-chunk
// all-gather of a side's shards.
#include <utility>

#include "als_engine_impl.h"

using namespace cfk_detail;

namespace {

// The exchange's stream and events, made before the communicator: an engine never holds a communicator without them.
int comm_streams(als_engine* e) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(e->comm_stream.create());
    HIP_TRY(e->solved.create(hipEventDisableTiming));
    for (auto& ev : e->gathered) HIP_TRY(ev.create(hipEventDisableTiming));
    return ALS_OK;
}

// Caller-level RCCL groups (als_comm_group_start / _end, one host thread driving several engines): inside a
// group a collective is only placed on its stream at the OUTERMOST ncclGroupEnd, so the "gathered" event of an
// all-gather issued inside a group must be recorded after that end, not at the call (recorded earlier it would
// order nothing). The thread's open-group depth and the (engine, side) pairs whose record is deferred:
thread_local int g_group_depth = 0;
thread_local std::vector<std::pair<als_engine*, int>> g_group_gathers;

int record_gathered(als_engine* e, int side) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventRecord(e->gathered[side], e->comm_stream));
    e->gather_pending[side] = true;
    return ALS_OK;
}

}  // namespace

extern "C" {

int als_comm_unique_id(void* id_out, int nbytes) {
    if (!id_out || nbytes < (int)sizeof(ncclUniqueId))
        return fail(ALS_ERR_INVALID_ARGUMENT, "unique id buffer must hold %d bytes", (int)sizeof(ncclUniqueId));
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return ALS_OK;
}

int als_comm_init(als_engine* e, int world, int rank, const void* unique_id) {
    if (int r = check_engine(e)) return r;
    if (world < 1 || rank < 0 || rank >= world || !unique_id)
        return fail(ALS_ERR_INVALID_ARGUMENT, "bad world/rank/unique_id (world %d, rank %d)", world, rank);
    if (e->comm) return fail(ALS_ERR_STATE, "engine already has a communicator");
    if (int r = comm_streams(e)) return r;
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    NCCL_TRY(ncclCommInitRank(&e->comm, world, id, rank));
    e->world = world;
    e->rank = rank;
    return ALS_OK;
}

int als_comm_init_group(als_engine** engines, int n) {
    if (!engines || n < 1) return fail(ALS_ERR_INVALID_ARGUMENT, "need >= 1 engines");
    std::vector<int> devs(n);
    for (int i = 0; i < n; ++i) {
        if (int r = check_engine(engines[i])) return r;
        if (engines[i]->comm) return fail(ALS_ERR_STATE, "engine %d already has a communicator", i);
        devs[i] = engines[i]->device;
        for (int j = 0; j < i; ++j)
            if (devs[j] == devs[i]) return fail(ALS_ERR_INVALID_ARGUMENT, "engines %d and %d share device %d", j, i, devs[i]);
    }
    for (int i = 0; i < n; ++i)
        if (int r = comm_streams(engines[i])) return r;
    std::vector<ncclComm_t> comms(n);
    NCCL_TRY(ncclCommInitAll(comms.data(), n, devs.data()));
    for (int i = 0; i < n; ++i) {
        engines[i]->comm = comms[i];
        engines[i]->world = n;
        engines[i]->rank = i;
    }
    return ALS_OK;
}

int als_comm_info(const als_engine* e, int* world, int* rank) {
    if (int r = check_engine(e)) return r;
    if (world) *world = e->world;
    if (rank) *rank = e->rank;
    return ALS_OK;
}

int als_comm_group_start(void) {
    NCCL_TRY(ncclGroupStart());
    ++g_group_depth;
    return ALS_OK;
}

int als_comm_group_end(void) {
    if (g_group_depth <= 0) return fail(ALS_ERR_STATE, "als_comm_group_end without als_comm_group_start");
    const ncclResult_t r = ncclGroupEnd();
    if (--g_group_depth > 0) {
        if (r != ncclSuccess) return fail(ALS_ERR_COMM, "ncclGroupEnd failed: %s", ncclGetErrorString(r));
        return ALS_OK;
    }
    // outermost end: the grouped all-gathers are on their streams now; record their events behind them
    std::vector<std::pair<als_engine*, int>> touched;
    touched.swap(g_group_gathers);
    if (r != ncclSuccess) return fail(ALS_ERR_COMM, "ncclGroupEnd failed: %s", ncclGetErrorString(r));
    for (auto& eg : touched)
        if (int rc = record_gathered(eg.first, eg.second)) return rc;
    return ALS_OK;
}

int als_allgather_shard(als_engine* e, int side, int64_t slots_per_chunk, int64_t chunk) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (e->world == 1 && !e->comm) return ALS_OK;   // one shard: the replica is the matrix
    if (!e->comm) return fail(ALS_ERR_STATE, "als_allgather_shard: no communicator (als_comm_init)");
    const Factors& f = e->fac[side];
    if (!f.ptr) return fail(ALS_ERR_STATE, "factors of side %d not allocated/bound", side);
    const int64_t Sc = slots_per_chunk;
    if (Sc < 0 || chunk < 0 || (chunk + 1) * Sc * e->world > f.n_rows)
        return fail(ALS_ERR_INVALID_ARGUMENT, "chunk %lld of %lld slots per shard x %d shards exceeds %lld rows",
                    (long long)chunk, (long long)Sc, e->world, (long long)f.n_rows);
    if (Sc == 0) return ALS_OK;
    HIP_TRY(hipSetDevice(e->device));
    // after this engine's solve (stream) on comm_stream; the next solve that reads this side waits for it
    HIP_TRY(hipEventRecord(e->solved, e->stream));
    HIP_TRY(hipStreamWaitEvent(e->comm_stream, e->solved, 0));
    const ncclDataType_t dt = e->precision == ALS_F64 ? ncclFloat64 : ncclFloat32;
    const size_t row = (size_t)e->kp * e->elem();
    // chunk-major slots: chunk c holds the G shards' Sc-row pieces back to back, so its exchange is ONE
    // contiguous in-place all-gather
    char* cbase = (char*)f.ptr + (size_t)chunk * (size_t)(Sc * e->world) * row;
    e->last_gather_side = side;
    e->last_gather_chunk = chunk;
    e->last_gather_rows = Sc;
    NCCL_TRY(ncclAllGather(cbase + (size_t)e->rank * Sc * row, cbase, (size_t)Sc * e->kp, dt, e->comm,
                           e->comm_stream));
    if (g_group_depth > 0) {   // placed on the stream at the outermost group end: record the event there
        g_group_gathers.emplace_back(e, side);
        return ALS_OK;
    }
    return record_gathered(e, side);
}

int als_comm_wait(als_engine* e) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    return wait_gathers(e, true, true);
}

int als_comm_set_timeout(als_engine* e, int64_t timeout_ms) {
    if (int r = check_engine(e)) return r;
    e->cfg.comm_timeout_ms = timeout_ms;
    return ALS_OK;
}

}  // extern "C"
