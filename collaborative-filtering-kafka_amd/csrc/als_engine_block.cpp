// als_engine_block.cpp -- in-block upload (its work plan: als_plan.h), chunking and the row layout of a side. A block
// is built aside and committed only when everything succeeded: a failed call leaves the side as it was.
#include "als_engine_impl.h"

using namespace cfk_detail;

namespace {

int check_block_shape(als_engine* e, int64_t n_rows, int64_t row_offset, int64_t n_opp_rows) {
    if (n_rows < 0 || row_offset < 0 || n_opp_rows < 0)
        return fail(ALS_ERR_INVALID_ARGUMENT, "negative size (n_rows=%lld row_offset=%lld n_opp_rows=%lld)",
                    (long long)n_rows, (long long)row_offset, (long long)n_opp_rows);
    if (n_rows > INT32_MAX) return fail(ALS_ERR_UNSUPPORTED, "n_rows exceeds 2^31-1");
    if (n_opp_rows >= INT32_MAX) return fail(ALS_ERR_UNSUPPORTED, "n_opp_rows must be < 2^31-1 (int32 column indices)");
    if ((n_opp_rows + 1) * (int64_t)e->kp * (int64_t)e->elem() > (int64_t)UINT32_MAX)
        return fail(ALS_ERR_UNSUPPORTED, "opposite factor matrix exceeds 4 GiB (32-bit gather offsets)");
    return ALS_OK;
}

// Padded entries of a row of degree d (every row starts on a 32-entry block).
inline int64_t padded(int64_t d) { return (d + cfk::BLOCK_ENTRIES - 1) / cfk::BLOCK_ENTRIES * cfk::BLOCK_ENTRIES; }

// Device copy of a task list (none for an empty list).
int upload_tasks(DeviceBuf<Task>& dst, const std::vector<Task>& src) {
    const size_t bytes = src.size() * sizeof(Task);
    hipError_t st = dst.alloc(src.size());
    if (st != hipSuccess)
        return fail(ALS_ERR_OUT_OF_MEMORY, "device allocation (%zu bytes): %s", bytes, hipGetErrorString(st));
    if (bytes == 0) return ALS_OK;
    st = hipMemcpy(dst.get(), src.data(), bytes, hipMemcpyHostToDevice);
    if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "hipMemcpy: %s", hipGetErrorString(st));
    return ALS_OK;
}

int upload_list(TaskList& l, std::vector<Task>&& planned) {
    l.host = std::move(planned);
    return upload_tasks(l.dev, l.host);
}

// The long rows' blocks chunk-major: dst block i <- src block perm[i], into new buffers that replace d_col / d_rat.
hipError_t permute_blocks(const std::vector<int32_t>& perm, DeviceBuf<int32_t>& d_col, DeviceBuf<float>& d_rat) {
    DeviceBuf<int32_t> d_perm, col2;
    DeviceBuf<float> rat2;
    hipError_t st = d_perm.alloc(perm.size());
    if (st == hipSuccess) st = col2.alloc(d_col.size());
    if (st == hipSuccess) st = rat2.alloc(d_rat.size());
    if (st == hipSuccess) st = hipMemcpy(d_perm.get(), perm.data(), perm.size() * 4, hipMemcpyHostToDevice);
    if (st == hipSuccess)
        st = cfk::launch_permute_blocks(d_col.get(), d_rat.get(), col2.get(), rat2.get(), d_perm.get(),
                                        (int64_t)perm.size(), nullptr);
    if (st == hipSuccess) st = hipDeviceSynchronize();
    d_perm.reset();
    if (st == hipSuccess) {
        d_col = std::move(col2);
        d_rat = std::move(rat2);
    }
    return st;
}

// The device side of a block whose padded in-block (d_col / d_rat, device, already laid out) has row degrees deg[]
// and row starts begin[]: plans it (als_plan.h: layout, then the task lists), permutes the interleaved rows' blocks,
// packs the pre-split operands, uploads the plan, sizes the partial and pre-split workspaces, and only then replaces
// the side's block.
int finish_block(als_engine* e, int side, int64_t n_rows, int64_t row_offset, int64_t n_opp_rows, int64_t nnz,
                 const std::vector<int64_t>& deg, const std::vector<int64_t>& begin, DeviceBuf<int32_t> d_col,
                 DeviceBuf<float> d_rat) {
    const int64_t nnz_padded = begin[n_rows];
    cfk::BlockShape shape;
    shape.path = e->path;
    shape.k = e->k;
    shape.kp = e->kp;
    shape.cu_count = e->cu_count;
    shape.n_opp_rows = n_opp_rows;
    const cfk::BlockLayout layout = cfk::plan_layout(e->cfg.plan, shape, deg);
    std::vector<int32_t> bfirst;   // opposite slot of every block's first entry (physical position 0 of the block)
    if (layout.ranges && nnz_padded > 0) {
        bfirst.resize((size_t)(nnz_padded / cfk::BLOCK_ENTRIES));
        hipError_t st = hipMemcpy2D(bfirst.data(), 4, d_col.get(), cfk::BLOCK_ENTRIES * 4, 4, bfirst.size(),
                                    hipMemcpyDeviceToHost);
        if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "set_block: block heads: %s", hipGetErrorString(st));
    }
    cfk::BlockPlan plan = cfk::plan_build(e->cfg.plan, shape, layout, deg, begin, bfirst);
    if (plan.error) return fail(ALS_ERR_UNSUPPORTED, "%s", plan.error);

    hipError_t st0 = hipSetDevice(e->device);
    if (st0 == hipSuccess) st0 = hipStreamSynchronize(e->stream);
    // (before the pre-split packing below derives its arrays from the permuted blocks)
    if (st0 == hipSuccess && !plan.perm.empty()) st0 = permute_blocks(plan.perm, d_col, d_rat);
    if (st0 != hipSuccess) return fail(ALS_ERR_DEVICE, "set_block: %s", hipGetErrorString(st0));
    Block blk;
    blk.d_col = std::move(d_col);
    blk.d_rat = std::move(d_rat);
    blk.n_rows = n_rows;
    blk.row_offset = row_offset;
    blk.n_opp_rows = n_opp_rows;
    blk.nnz = nnz;
    blk.nnz_padded = nnz_padded;
    blk.layout = layout;
    blk.ilv_rows = plan.ilv_rows;
    blk.ilv_tasks = plan.ilv_tasks;
    // The workspaces both sides share only grow (each freed before its larger successor is allocated), so a grown one
    // still serves the blocks already set; a failure to grow leaves it too small for them and unsets both sides.
    auto grow = [&](DeviceBuf<char>& buf, size_t bytes, const char* what) {
        const hipError_t st = buf.reserve(bytes);
        if (st == hipSuccess) return (int)ALS_OK;
        for (auto& b : e->blk) b = Block();
        return fail(ALS_ERR_OUT_OF_MEMORY, "%s device allocation (%zu bytes): %s", what, bytes, hipGetErrorString(st));
    };
    // the pre-split copy of the opposite table (cfk::launch_presplit_prepare, once per half), sized for the larger side
    if (layout.presplit)
        if (int r = grow(e->d_split, (size_t)((n_opp_rows + 1) * (int64_t)cfk::presplit_row_bytes(e->kp)), "pre-split"))
            return r;
    if (layout.presplit && nnz_padded > 0) {
        // the RHS operand's ratings, packed once (setup time): fp16 rh pairs, then rm pairs
        hipError_t st = blk.d_rat_pk.alloc((size_t)nnz_padded);
        if (st != hipSuccess)
            return fail(ALS_ERR_OUT_OF_MEMORY, "device allocation (%zu bytes): %s", (size_t)nnz_padded * 4,
                        hipGetErrorString(st));
        st = cfk::launch_pack_ratings(blk.d_rat.get(), blk.d_rat_pk.get(), nnz_padded / 2, nullptr);
        // and the column indices in the order of the LDS-DMA gather (one 16-B load per loader row)
        if (st == hipSuccess) st = blk.d_col_ps.alloc((size_t)nnz_padded);
        if (st == hipSuccess) st = cfk::launch_pack_cols_ps(blk.d_col.get(), blk.d_col_ps.get(), nnz_padded, nullptr);
        if (st == hipSuccess) st = hipDeviceSynchronize();
        if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "pack ratings: %s", hipGetErrorString(st));
    }
    if (int r = upload_list(blk.tasks, std::move(plan.tasks))) return r;
    if (int r = upload_list(blk.reduce, std::move(plan.reduce))) return r;
    for (int c = 0; c < 3; ++c)
        if (int r = upload_list(blk.dual[c], std::move(plan.dual[c]))) return r;
    if (int r = upload_tasks(blk.sq_tasks, plan.sq_all)) return r;
    HIP_TRY(blk.d_task_se.alloc(plan.sq_all.size()));
    // Partial workspace sized for the larger side (the generic path: its per-workgroup Gram slabs, when the packed
    // triangle does not fit in LDS -- up to 1024 workgroups within 4 GiB)
    size_t need = (size_t)plan.slots * cfk::partial_words_per_lane(e->precision, e->kp, e->path) * 64 * e->elem();
    if (e->path == Path::GENERIC) {
        const cfk::GenericPlan gp = cfk::generic_plan(e->precision, e->kp);
        if (!gp.g_in_lds) {
            const int64_t slab = gp.slab_elems * (int64_t)e->elem();
            e->generic_slabs = std::max<int64_t>(1, std::min<int64_t>(1024, (4ll << 30) / slab));
            need = (size_t)(e->generic_slabs * slab);
        }
    }
    if (int r = grow(e->d_partials, need, "partials")) return r;
    blk.set = true;
    e->blk[side] = std::move(blk);
    return ALS_OK;
}

}  // namespace

extern "C" {

int als_set_block(als_engine* e, int side, int64_t n_rows, int64_t row_offset, int64_t n_opp_rows,
                  const int64_t* row_ptr, const int32_t* col_idx, const int16_t* ratings) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (int r = check_block_shape(e, n_rows, row_offset, n_opp_rows)) return r;
    if (n_rows > 0 && !row_ptr) return fail(ALS_ERR_INVALID_ARGUMENT, "row_ptr is NULL");
    const int64_t nnz = n_rows > 0 ? row_ptr[n_rows] : 0;
    if (n_rows > 0 && row_ptr[0] != 0) return fail(ALS_ERR_INVALID_ARGUMENT, "row_ptr[0] must be 0");
    if (nnz > 0 && (!col_idx || !ratings)) return fail(ALS_ERR_INVALID_ARGUMENT, "col_idx/ratings NULL");
    // Validate the block on the host: a bad index would fault the GPU.
    std::vector<int64_t> deg(n_rows), begin(n_rows + 1);
    int64_t o = 0;
    for (int64_t i = 0; i < n_rows; ++i) {
        const int64_t d = row_ptr[i + 1] - row_ptr[i];
        if (d < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "row_ptr not monotone at row %lld", (long long)i);
        if (d > INT32_MAX / 2) return fail(ALS_ERR_UNSUPPORTED, "row %lld has %lld entries", (long long)i, (long long)d);
        deg[i] = d;
        begin[i] = o;
        o += padded(d);
    }
    begin[n_rows] = o;
    for (int64_t t = 0; t < nnz; ++t)
        if (col_idx[t] < 0 || col_idx[t] >= n_opp_rows)
            return fail(ALS_ERR_INVALID_ARGUMENT, "col_idx[%lld]=%d outside [0, %lld)", (long long)t, col_idx[t],
                        (long long)n_opp_rows);
    // Padded, block-interleaved device in-block (see cfk::block_position): every row starts on a
    // 32-entry block; padding entries point at the sentinel zero row (col = n_opp_rows) with rating 0.
    std::vector<int32_t> col(o, (int32_t)n_opp_rows);
    std::vector<float> rat(o, 0.f);
    for (int64_t i = 0; i < n_rows; ++i)
        for (int64_t t = 0; t < deg[i]; ++t) {
            const int64_t pos = begin[i] + cfk::block_position(t);
            col[pos] = col_idx[row_ptr[i] + t];
            rat[pos] = (float)ratings[row_ptr[i] + t];
        }
    HIP_TRY(hipSetDevice(e->device));
    DeviceBuf<int32_t> d_col;
    DeviceBuf<float> d_rat;
    if (o > 0) {
        hipError_t st = d_col.alloc((size_t)o);
        if (st == hipSuccess) st = d_rat.alloc((size_t)o);
        if (st == hipSuccess) st = hipMemcpy(d_col.get(), col.data(), o * 4, hipMemcpyHostToDevice);
        if (st == hipSuccess) st = hipMemcpy(d_rat.get(), rat.data(), o * 4, hipMemcpyHostToDevice);
        if (st != hipSuccess) return fail(ALS_ERR_OUT_OF_MEMORY, "in-block upload: %s", hipGetErrorString(st));
    }
    return finish_block(e, side, n_rows, row_offset, n_opp_rows, nnz, deg, begin, std::move(d_col), std::move(d_rat));
}

int als_set_block_coo(als_engine* e, int side, int64_t n_rows, int64_t row_offset, int64_t n_opp_rows, int64_t nnz,
                      const int32_t* rows, const int32_t* cols, const int16_t* ratings) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (int r = check_block_shape(e, n_rows, row_offset, n_opp_rows)) return r;
    if (nnz < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "nnz < 0");
    if (nnz > 0 && (!rows || !cols || !ratings)) return fail(ALS_ERR_INVALID_ARGUMENT, "rows/cols/ratings NULL");
    if (nnz >= INT32_MAX) return fail(ALS_ERR_UNSUPPORTED, "nnz per block must be < 2^31-1 (shard the side)");
    HIP_TRY(hipSetDevice(e->device));
    std::vector<int64_t> deg, begin;
    DeviceBuf<int32_t> d_col;
    DeviceBuf<float> d_rat;
    std::string err;
    const int code = cfk::build_block_device(rows, cols, ratings, nnz, n_rows, n_opp_rows, e->stream, deg, begin,
                                             d_col, d_rat, err);
    if (code != ALS_OK) return fail(code, "als_set_block_coo: %s", err.c_str());
    return finish_block(e, side, n_rows, row_offset, n_opp_rows, nnz, deg, begin, std::move(d_col), std::move(d_rat));
}

int als_set_chunks(als_engine* e, int side, int n_chunks, const int64_t* row_bounds) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    Block& b = e->blk[side];
    if (!b.set) return fail(ALS_ERR_STATE, "als_set_chunks: no block set for side %d", side);
    if (n_chunks < 1 || !row_bounds) return fail(ALS_ERR_INVALID_ARGUMENT, "n_chunks must be >= 1 with row_bounds");
    if (row_bounds[0] != 0 || row_bounds[n_chunks] != b.n_rows)
        return fail(ALS_ERR_INVALID_ARGUMENT, "row_bounds must run from 0 to n_rows (%lld)", (long long)b.n_rows);
    for (int c = 0; c < n_chunks; ++c)
        if (row_bounds[c + 1] < row_bounds[c]) return fail(ALS_ERR_INVALID_ARGUMENT, "row_bounds not monotone");
    // stable partition by chunk keeps the longest-first order inside every chunk; all five lists are partitioned and
    // uploaded aside, then committed together
    TaskList* lists[5] = {&b.tasks, &b.reduce, &b.dual[0], &b.dual[1], &b.dual[2]};
    DeviceBuf<Task> chunked[5];
    std::vector<int32_t> coff[5];
    HIP_TRY(hipSetDevice(e->device));
    for (int l = 0; l < 5; ++l) {
        std::vector<Task> ct;
        cfk::partition_by_chunk(lists[l]->host, n_chunks, row_bounds, ct, coff[l]);
        if (int r = upload_tasks(chunked[l], ct)) return r;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));   // a chunk in flight reads the lists being replaced
    for (int l = 0; l < 5; ++l) {
        lists[l]->chunked = std::move(chunked[l]);
        lists[l]->coff = std::move(coff[l]);
    }
    return ALS_OK;
}

int als_set_row_layout(als_engine* e, int side, int64_t rows_per_chunk, int64_t chunk_stride) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    Block& b = e->blk[side];
    if (!b.set) return fail(ALS_ERR_STATE, "als_set_row_layout: no block set for side %d", side);
    if (rows_per_chunk < 0 || (rows_per_chunk > 0 && chunk_stride < rows_per_chunk) || rows_per_chunk > INT32_MAX)
        return fail(ALS_ERR_INVALID_ARGUMENT, "rows_per_chunk %lld / chunk_stride %lld", (long long)rows_per_chunk,
                    (long long)chunk_stride);
    b.rows_per_chunk = rows_per_chunk;
    b.chunk_stride = rows_per_chunk > 0 ? chunk_stride : 0;
    return ALS_OK;
}

}  // extern "C"
