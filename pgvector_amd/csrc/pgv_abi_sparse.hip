// pgv_abi_sparse.hip -- extern "C" entry points of libpgv_hip (include/pgv_hip.h): the sparsevec distances and the exact
// top-k over CSR vectors.  The kernels are kernels_sparse.hip's; the selection is launch_topk_segments, as in pgv_bit_topk.
#include "pgv_abi_common.h"

namespace {

constexpr int kSparseMaxDim = 1000000000;  // SPARSEVEC_MAX_DIM (src/sparsevec.h:8)
constexpr int kSparseMaxNnz = 16000;       // SPARSEVEC_MAX_NNZ (src/sparsevec.h:9)

}  // namespace

// (check_sparse_dim and stage_csr are declared in pgv_abi_common.h: the sparse HNSW entries of pgv_abi_hnsw.hip validate
// and stage their CSR arguments with them)
int check_sparse_dim(const char *who, int dim) {
    if (dim < 1 || dim > kSparseMaxDim) PGV_FAIL(PGV_ERR_DIMS, "%s: dimensions %d outside 1..%d", who, dim, kSparseMaxDim);
    return PGV_OK;
}

namespace {

// ptr [n + 1] on the host: starts at 0, monotone, no vector above the reference's limit of stored elements
int check_sparse_ptr(const char *who, const char *what, const int64_t *ptr, int64_t n) {
    if (ptr[0] != 0) PGV_FAIL(PGV_ERR_ARG, "%s: %s: ptr[0] is %lld, not 0", who, what, (long long)ptr[0]);
    for (int64_t v = 0; v < n; v++) {
        const int64_t nnz = ptr[v + 1] - ptr[v];
        if (nnz < 0)
            PGV_FAIL(PGV_ERR_ARG, "%s: %s: ptr is not monotone at vector %lld (%lld after %lld)", who, what, (long long)v,
                     (long long)ptr[v + 1], (long long)ptr[v]);
        if (nnz > kSparseMaxNnz)
            PGV_FAIL(PGV_ERR_DIMS, "%s: %s: vector %lld has %lld stored elements, more than %d", who, what, (long long)v,
                     (long long)nnz, kSparseMaxNnz);
    }
    return PGV_OK;
}

// the elements of host arrays under a checked host ptr: indices strictly ascending inside 0 .. dim - 1, values finite
// (either array may be device memory: null here, not checked)
int check_sparse_elements(const char *who, const char *what, int dim, const int64_t *ptr, int64_t n, const int32_t *idx,
                          const float *val) {
    for (int64_t v = 0; v < n; v++) {
        for (int64_t e = ptr[v]; e < ptr[v + 1]; e++) {
            const long long pos = (long long)(e - ptr[v]);
            if (idx) {
                if (idx[e] < 0 || idx[e] >= dim)
                    PGV_FAIL(PGV_ERR_ARG, "%s: %s: vector %lld position %lld: index %d outside 0..%d", who, what, (long long)v,
                             pos, (int)idx[e], dim - 1);
                if (e > ptr[v] && idx[e] <= idx[e - 1])
                    PGV_FAIL(PGV_ERR_ARG, "%s: %s: vector %lld position %lld: index %d does not ascend from %d", who, what,
                             (long long)v, pos, (int)idx[e], (int)idx[e - 1]);
            }
            if (val && !std::isfinite(val[e]))
                PGV_FAIL(PGV_ERR_ARG, "%s: %s: vector %lld position %lld: value is not finite", who, what, (long long)v, pos);
        }
    }
    return PGV_OK;
}

}  // namespace

// A caller's CSR triple on the device (StagedCsr: pgv_abi_common.h).  Host arrays are validated before anything is
// launched; device arrays are used in place, unchecked (pgv_rerank's rule for cand) -- except ptr when the host needs it
// anyway (want_host_ptr: the queries' tiles are planned from it), whose copy is checked like a host ptr, since the
// kernel's LDS is sized from it
int stage_csr(pgv_ctx *ctx, const char *who, const char *what, int dim, const int64_t *ptr, const int32_t *idx, const float *val,
              int64_t n, bool want_host_ptr, DBuf &buf_ptr, DBuf &buf_idx, DBuf &buf_val, StagedCsr *out) {
    out->dev.n = n;
    const bool ptr_dev = is_device_ptr(ptr), idx_dev = idx && is_device_ptr(idx), val_dev = val && is_device_ptr(val);
    int64_t total = -1;
    if (!ptr_dev) {
        out->host_ptr = ptr;
    } else if (want_host_ptr) {
        out->ptr_copy.resize((size_t)n + 1);
        PGV_HIP(hipMemcpyAsync(out->ptr_copy.data(), ptr, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
        PGV_HIP(hipStreamSynchronize(ctx->stream));
        out->host_ptr = out->ptr_copy.data();
    } else if (!idx_dev || !val_dev) {
        PGV_HIP(hipMemcpyAsync(&total, ptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        PGV_HIP(hipStreamSynchronize(ctx->stream));
        if (total < 0) PGV_FAIL(PGV_ERR_ARG, "%s: %s: ptr[n] is negative", who, what);
    }
    if (out->host_ptr) {
        PGV_TRY(check_sparse_ptr(who, what, out->host_ptr, n));
        total = out->host_ptr[n];
        if (total > 0 && (!idx || !val)) PGV_FAIL(PGV_ERR_ARG, "%s: %s: idx/val is NULL", who, what);
        if (!idx_dev || !val_dev)
            PGV_TRY(check_sparse_elements(who, what, dim, out->host_ptr, n, idx_dev ? nullptr : idx, val_dev ? nullptr : val));
    }
    const void *p;
    PGV_TRY(stage_flat(ctx, ptr, sizeof(int64_t) * ((size_t)n + 1), buf_ptr, &p));
    out->dev.ptr = static_cast<const int64_t *>(p);
    PGV_TRY(stage_flat(ctx, idx, idx_dev ? 0 : sizeof(int32_t) * (size_t)total, buf_idx, &p));
    out->dev.idx = static_cast<const int32_t *>(p);
    PGV_TRY(stage_flat(ctx, val, val_dev ? 0 : sizeof(float) * (size_t)total, buf_val, &p));
    out->dev.val = static_cast<const float *>(p);
    return PGV_OK;
}

namespace {

// the tiles of one launch: queries [q0, q0 + nq) of the staged query CSR
struct TileRun {
    size_t first;
    int ntiles, max_tile_nnz, max_tile_nq, max_q_nnz, q0, nq;
};
void plan_run(const int64_t *q_ptr, int q0, int nq, std::vector<SparseTile> *all, TileRun *run) {
    std::vector<SparseTile> tiles;
    int max_q = 0;
    sparse_plan_tiles(q_ptr + q0, nq, &tiles, &max_q);
    *run = {all->size(), (int)tiles.size(), 0, 0, max_q, q0, nq};
    for (const SparseTile &t : tiles) {
        run->max_tile_nnz = std::max(run->max_tile_nnz, t.nnz);
        run->max_tile_nq = std::max(run->max_tile_nq, t.nq);
        all->push_back(t);
    }
}
int upload_tiles(pgv_ctx *ctx, const std::vector<SparseTile> &all, const SparseTile **dev) {
    const void *p;
    PGV_TRY(stage_flat(ctx, all.data(), sizeof(SparseTile) * all.size(), ctx->plan_a, &p));
    *dev = static_cast<const SparseTile *>(p);
    return PGV_OK;
}
int launch_run(pgv_ctx *ctx, int mode, const SparseTile *tiles_dev, const TileRun &run, const StagedCsr &q, const StagedCsr &r,
               void *out, int64_t out_stride) {
    ScanTimer timer{ctx};
    PGV_TRY(timer.begin((double)r.dev.n * run.nq, (double)r.dev.n * run.ntiles, true));
    SparseCsr qv = q.dev;
    qv.ptr += run.q0;  // a tile counts its queries from the run's first
    qv.n = run.nq;
    PGV_TRY(launch_sparse_tiles(ctx, mode, tiles_dev + run.first, run.ntiles, run.max_tile_nnz, run.max_tile_nq, run.max_q_nnz,
                                qv, r.dev, out, out_stride));
    return timer.end();
}

// the floats of a query chunk's distance matrix at most: 2^30, or PGV_SPARSE_MATRIX_FLOATS (tests reach the split
// with small shapes through it; read at every call)
int64_t sparse_matrix_floats() {
    const char *e = getenv("PGV_SPARSE_MATRIX_FLOATS");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (int64_t)v : (int64_t)1 << 30;
}

// one query (q_nnz, q_idx, q_val) against the rows: pgv_sparse_distance_batch and pgv_sparse_cosine_distance_batch
int sparse_one_query(pgv_ctx *ctx, const char *who, int mode, int dim, int q_nnz, const int32_t *q_idx, const float *q_val,
                     const int64_t *row_ptr, const int32_t *row_idx, const float *row_val, int64_t n, void *out,
                     size_t out_elem) {
    PGV_TRY(check_sparse_dim(who, dim));
    if (n < 0) PGV_FAIL(PGV_ERR_ARG, "%s: n < 0", who);
    if (q_nnz < 0) PGV_FAIL(PGV_ERR_ARG, "%s: q_nnz < 0", who);
    if (q_nnz > kSparseMaxNnz)
        PGV_FAIL(PGV_ERR_DIMS, "%s: query: vector 0 has %d stored elements, more than %d", who, q_nnz, kSparseMaxNnz);
    if (n == 0) return PGV_OK;
    if (!row_ptr) PGV_FAIL(PGV_ERR_ARG, "%s: row_ptr is NULL", who);
    PGV_HIP(hipSetDevice(ctx->device));
    const int64_t q_ptr[2] = {0, q_nnz};
    StagedCsr q, r;
    PGV_TRY(stage_csr(ctx, who, "query", dim, q_ptr, q_idx, q_val, 1, true, ctx->plan_c, ctx->q_stage, ctx->centers_stage, &q));
    PGV_TRY(stage_csr(ctx, who, "rows", dim, row_ptr, row_idx, row_val, n, false, ctx->plan_b, ctx->rows_stage, ctx->idx_stage, &r));
    std::vector<SparseTile> tiles;
    TileRun run;
    plan_run(q_ptr, 0, 1, &tiles, &run);
    const SparseTile *tiles_dev;
    PGV_TRY(upload_tiles(ctx, tiles, &tiles_dev));
    OutArg od;
    PGV_TRY(od.init(out, out_elem * (size_t)n, ctx->out_stage));
    PGV_TRY(launch_run(ctx, mode, tiles_dev, run, q, r, od.dev, n));
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    return sync_if(ctx, need);
}

}  // namespace

extern "C" {

int pgv_sparse_distance_batch(pgv_ctx *ctx, pgv_metric metric, int dim, int q_nnz, const int32_t *q_idx, const float *q_val,
                              const int64_t *row_ptr, const int32_t *row_idx, const float *row_val, int64_t n, float *out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_sparse_distance_batch: ctx/out is NULL");
    PGV_TRY(check_metric(metric));
    return sparse_one_query(ctx, "pgv_sparse_distance_batch", (int)metric, dim, q_nnz, q_idx, q_val, row_ptr, row_idx, row_val,
                            n, out, sizeof(float));
}

int pgv_sparse_cosine_distance_batch(pgv_ctx *ctx, int dim, int q_nnz, const int32_t *q_idx, const float *q_val,
                                     const int64_t *row_ptr, const int32_t *row_idx, const float *row_val, int64_t n,
                                     double *out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_sparse_cosine_distance_batch: ctx/out is NULL");
    return sparse_one_query(ctx, "pgv_sparse_cosine_distance_batch", 3, dim, q_nnz, q_idx, q_val, row_ptr, row_idx, row_val, n,
                            out, sizeof(double));
}

// `ORDER BY emb <op> $1 LIMIT k` over a sparsevec column without an index, for a batch of queries: pgv_bit_topk's
// structure over CSR vectors.  sparse_tile_kernel fills the chunk's distance matrix mat[q * n + row],
// launch_topk_segments selects with ties to the lower row.
int pgv_sparse_topk(pgv_ctx *ctx, pgv_metric metric, int dim, const int64_t *q_ptr, const int32_t *q_idx, const float *q_val,
                    int nq, const int64_t *row_ptr, const int32_t *row_idx, const float *row_val, int64_t n, int k,
                    float *out_dist, int64_t *out_idx) {
    const char *who = "pgv_sparse_topk";
    if (!ctx || !out_dist || !out_idx) PGV_FAIL(PGV_ERR_ARG, "pgv_sparse_topk: ctx/out_dist/out_idx is NULL");
    PGV_TRY(check_metric(metric));
    PGV_TRY(check_sparse_dim(who, dim));
    if (nq < 0 || n < 0) PGV_FAIL(PGV_ERR_ARG, "pgv_sparse_topk: nq/n < 0");
    if (k < 1 || k > 4096) PGV_FAIL(PGV_ERR_ARG, "pgv_sparse_topk: k %d outside 1..4096", k);
    if (n > 0xffffffffll) PGV_FAIL(PGV_ERR_ARG, "pgv_sparse_topk: more than 2^32 rows");
    if (nq == 0) return PGV_OK;
    if (!q_ptr || (n > 0 && !row_ptr)) PGV_FAIL(PGV_ERR_ARG, "pgv_sparse_topk: q_ptr/row_ptr is NULL");
    PGV_HIP(hipSetDevice(ctx->device));
    StagedCsr q, r;
    PGV_TRY(stage_csr(ctx, who, "queries", dim, q_ptr, q_idx, q_val, nq, true, ctx->plan_c, ctx->q_stage, ctx->centers_stage, &q));
    if (n > 0)
        PGV_TRY(stage_csr(ctx, who, "rows", dim, row_ptr, row_idx, row_val, n, false, ctx->plan_b, ctx->rows_stage, ctx->idx_stage, &r));
    OutArg od, oi;
    PGV_TRY(od.init(out_dist, sizeof(float) * (size_t)nq * k, ctx->out_stage));
    PGV_TRY(oi.init(out_idx, sizeof(int64_t) * (size_t)nq * k, ctx->out_stage2));

    // the distance matrix of a query chunk stays at or under 2^30 floats; the tiles of every chunk go up in one copy
    const int chunk = n > 0 ? (int)std::min<int64_t>(nq, std::max<int64_t>(1, sparse_matrix_floats() / n)) : nq;
    std::vector<SparseTile> tiles;
    std::vector<TileRun> runs;
    if (n > 0)
        for (int q0 = 0; q0 < nq; q0 += chunk) {
            runs.emplace_back();
            plan_run(q.host_ptr, q0, std::min(chunk, nq - q0), &tiles, &runs.back());
        }
    const SparseTile *tiles_dev = nullptr;
    if (!tiles.empty()) PGV_TRY(upload_tiles(ctx, tiles, &tiles_dev));
    size_t ri = 0;
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int cn = std::min(chunk, nq - q0);
        PGV_TRY(ctx->dist_mat.ensure(sizeof(float) * std::max<size_t>((size_t)cn * (size_t)n, 4)));
        float *mat = ctx->dist_mat.as<float>();
        if (n > 0) PGV_TRY(launch_run(ctx, (int)metric, tiles_dev, runs[ri++], q, r, mat, n));
        PGV_TRY(launch_topk_segments(ctx, mat, nullptr, cn, n, k, od.as<float>() + (size_t)q0 * k,
                                     oi.as<int64_t>() + (size_t)q0 * k));
    }
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    PGV_TRY(oi.finish(ctx, &need));
    return sync_if(ctx, need);
}

}  // extern "C"
