// als_engine_call.h -- the host path of the engine's synchronous calls (als_engine_score.cpp, als_engine_query.cpp): lay
// out the workspace in d_rec, enqueue uploads, launches and downloads on the engine's stream until one fails, wait
// once. Private to csrc/.
#pragma once
#include <utility>

#include "als_args.h"
#include "als_engine_impl.h"

namespace cfk_detail {

// Offsets of a call's parts in d_rec, every part 256-byte aligned, after `need` bytes laid out elsewhere (a launch plan).
struct Workspace {
    int64_t need = 0;
    int64_t part(bool used, int64_t bytes) {   // the part's offset; a part not used takes no room
        const int64_t off = need;
        if (used) need += (bytes + 255) / 256 * 256;
        return off;
    }
};

// Make d_rec hold `need` bytes. Grow-only; the stream may still be reading the old one, so it is drained first.
inline int reserve_workspace(als_engine* e, const char* fn, int64_t need) {
    if ((size_t)need <= e->d_rec.size()) return ALS_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    const hipError_t st = e->d_rec.reserve((size_t)need);
    if (st != hipSuccess)
        return fail(ALS_ERR_OUT_OF_MEMORY, "%s: device allocation (%zu bytes): %s", fn, (size_t)need, hipGetErrorString(st));
    return ALS_OK;
}

// What a call enqueues on the engine's stream, up to the first failure: after it nothing more is enqueued and no
// launch function is entered.
struct StreamChain {
    als_engine* e;
    hipError_t st = hipSuccess;
    void upload(void* dev, const void* host, size_t bytes) {
        if (st == hipSuccess) st = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, e->stream);
    }
    void download(void* host, const void* dev, size_t bytes) {
        if (st == hipSuccess) st = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, e->stream);
    }
    template <class Launch, class... Args>
    void run(Launch launch, Args&&... args) {   // a cfk::launch_* function and its arguments before the stream
        if (st == hipSuccess) st = launch(std::forward<Args>(args)..., e->stream);
    }
    // The caller's host arrays are pageable: the stream has to pass the copies before the call returns, failed or not.
    int wait(const char* fn) {
        const hipError_t st2 = hipStreamSynchronize(e->stream);
        if (st == hipSuccess) st = st2;
        if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(st));
        return ALS_OK;
    }
    int finish(const char* fn) {
        if (int r = wait(fn)) return r;
        return sync_checked(e);
    }
};

// The exclusion CSR (check_exclusions) to d_eptr / d_eidx: the slice the ranges cover, the ranges rebased to it
// (`store` has to outlive the wait).
inline void upload_exclusions(StreamChain& c, const int64_t* excl_ptr, const int32_t* excl_idx, int64_t n_users,
                              int64_t* d_eptr, int32_t* d_eidx, std::vector<int64_t>& store) {
    const int64_t ex0 = excl_ptr[0], ex_nnz = excl_ptr[n_users] - ex0;
    c.upload(d_eptr, rebase_ptr(excl_ptr, n_users, store), (size_t)(n_users + 1) * sizeof(int64_t));
    if (ex_nnz > 0) c.upload(d_eidx, excl_idx + ex0, (size_t)ex_nnz * sizeof(int32_t));
}

// What a *_plan call reports.
inline int plan_info(int64_t info[4], int64_t threads_or_tile, int64_t groups, int64_t per_group, int64_t lds_bytes) {
    info[0] = threads_or_tile;
    info[1] = groups;
    info[2] = per_group;
    info[3] = lds_bytes;
    return ALS_OK;
}

}  // namespace cfk_detail
