// pgv_abi_build.hip -- extern "C" entry points of libpgv_hip (include/pgv_hip.h): assignment, distance batches, the exact scan, k-means.
// Split out of pgv_abi.hip in round 5 (one unit per area, so that an edit recompiles one of them).
#include "pgv_abi_common.h"

namespace {

// The caller's rows [n x tight bytes] to their centers, for pgv_assign and pgv_bit_assign: host rows are staged in slabs
// (BuildCallback batches), device rows that need no padding go in one piece; out_list / out_dist are written
// in place when they are device memory, staged and copied back otherwise.  score(r_dev, cnt, idx, val) scores one
// staged slab into device idx / val (val may be null)
template <typename Score>
int assign_in_slabs(pgv_ctx *ctx, const void *rows, int64_t n, size_t tight, size_t padded, int32_t *out_list,
                    float *out_dist, Score score) {
    const bool out_dev = is_device_ptr(out_list);
    const bool dist_dev = out_dist && is_device_ptr(out_dist);
    const int64_t slab = (is_device_ptr(rows) && padded == tight) ? n : (int64_t)1 << 18;
    bool need = false;
    for (int64_t r0 = 0; r0 < n; r0 += slab) {
        const int64_t cnt = n - r0 < slab ? n - r0 : slab;
        const void *r_dev;
        PGV_TRY(stage_rows(ctx, static_cast<const char *>(rows) + (size_t)r0 * tight, cnt, tight, padded, ctx->rows_stage,
                           &r_dev));
        int32_t *idx = out_list + r0;
        float *val = out_dist ? out_dist + r0 : nullptr;
        if (!out_dev) {
            PGV_TRY(ctx->out_stage.ensure(sizeof(int32_t) * (size_t)cnt));
            idx = ctx->out_stage.as<int32_t>();
        }
        if (out_dist && !dist_dev) {
            PGV_TRY(ctx->out_stage2.ensure(sizeof(float) * (size_t)cnt));
            val = ctx->out_stage2.as<float>();
        }
        PGV_TRY(score(r_dev, cnt, idx, val));
        if (!out_dev) {
            PGV_HIP(hipMemcpyAsync(out_list + r0, idx, sizeof(int32_t) * (size_t)cnt, hipMemcpyDeviceToHost, ctx->stream));
            need = true;
        }
        if (out_dist && !dist_dev) {
            PGV_HIP(hipMemcpyAsync(out_dist + r0, val, sizeof(float) * (size_t)cnt, hipMemcpyDeviceToHost, ctx->stream));
            need = true;
        }
        if (need && r0 + slab < n) PGV_HIP(hipStreamSynchronize(ctx->stream));  // scratch is reused
    }
    return sync_if(ctx, need);
}

// The empty clusters of a Lloyd iteration (counts_host[c] <= 0) take draws from the rng, clusters in center order
// (src/ivfkmeans.c:222-227).  On the host, in h_b: row[k] (row_bytes; -1, or the cluster's row among the refills) |
// fill[nempty x fill_bytes], zeroed, then draw(fill row) once per empty cluster.  On the device the same layout goes
// behind head_bytes of km_e, which is sized here, in one copy and one sync (h_b may be rewritten by the next step).
// *nempty: how many there were
template <typename Draw>
int refill_empty_clusters(pgv_ctx *ctx, const int32_t *counts_host, int k, size_t head_bytes, size_t row_bytes,
                          size_t fill_bytes, Draw draw, int *nempty) {
    int ne = 0;
    for (int c = 0; c < k; c++)
        if (counts_host[c] <= 0) ne++;
    *nempty = ne;
    const size_t bytes = row_bytes + (size_t)ne * fill_bytes;
    PGV_TRY(ctx->km_e.ensure(head_bytes + bytes + 16));
    if (ne == 0) return PGV_OK;
    PGV_TRY(ctx->h_b.ensure(bytes));
    int32_t *h_row = ctx->h_b.as<int32_t>();
    char *h_fill = ctx->h_b.as<char>() + row_bytes;
    memset(h_fill, 0, (size_t)ne * fill_bytes);
    int e = 0;
    for (int c = 0; c < k; c++) {
        h_row[c] = -1;
        if (counts_host[c] <= 0) {
            draw(static_cast<void *>(h_fill + (size_t)e * fill_bytes));
            h_row[c] = e++;
        }
    }
    PGV_HIP(hipMemcpyAsync(ctx->km_e.as<char>() + head_bytes, h_row, bytes, hipMemcpyHostToDevice, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    return PGV_OK;
}

}  // namespace

extern "C" {

// ================================================================= build side

int pgv_assign(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, int dim, const void *centers, int k,
               const void *rows, int64_t n, int32_t *out_list, float *out_dist) {
    if (!ctx || !out_list) PGV_FAIL(PGV_ERR_ARG, "pgv_assign: ctx/out_list is NULL");
    PGV_TRY(check_common(dtype, dim));
    PGV_TRY(check_metric(metric));
    if (k < 1 || !centers) PGV_FAIL(PGV_ERR_ARG, "need at least one center");
    if (n < 0) PGV_FAIL(PGV_ERR_ARG, "n < 0");
    if (n == 0) return PGV_OK;
    if (!rows) PGV_FAIL(PGV_ERR_ARG, "rows is NULL");
    PGV_HIP(hipSetDevice(ctx->device));
    const RowGeom g = row_geom(dim, dtype);
    const void *c_dev;
    PGV_TRY(stage_rows(ctx, centers, k, dim, dtype, g, ctx->centers_stage, &c_dev));
    const size_t es = elem_size(dtype);
    return assign_in_slabs(ctx, rows, n, (size_t)dim * es, (size_t)g.ld * es, out_list, out_dist,
                           [&](const void *r_dev, int64_t cnt, int32_t *idx, float *val) {
                               return launch_argmin(ctx, metric, dtype, g, r_dev, cnt, c_dev, k, idx, val);
                           });
}

int pgv_distance_batch(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, int dim, const void *query,
                       const void *rows, int64_t n, float *out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_distance_batch: ctx/out is NULL");
    PGV_TRY(check_common(dtype, dim));
    PGV_TRY(check_metric(metric));
    if (n < 0) PGV_FAIL(PGV_ERR_ARG, "n < 0");
    if (n == 0) return PGV_OK;
    if (!query || !rows) PGV_FAIL(PGV_ERR_ARG, "query/rows is NULL");
    PGV_HIP(hipSetDevice(ctx->device));
    const RowGeom g = row_geom(dim, dtype);
    const void *q_dev, *r_dev;
    PGV_TRY(stage_rows(ctx, query, 1, dim, dtype, g, ctx->q_stage, &q_dev));
    PGV_TRY(stage_rows(ctx, rows, n, dim, dtype, g, ctx->rows_stage, &r_dev));
    OutArg od;
    PGV_TRY(od.init(out, sizeof(float) * (size_t)n, ctx->out_stage));
    PGV_TRY(dense_scan(ctx, RowsView{r_dev, n, g, row_kind(dtype), metric}, q_dev, 1, 0, od.as<float>()));
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    return sync_if(ctx, need);
}

// The sequential scan + top-N heapsort of `ORDER BY embedding <op> $1 LIMIT k` without an index (the per-row
// l2_distance / vector_negative_inner_product / l1_distance calls of src/vector.c:579-697 and their halfvec twins),
// for a batch of queries against the same rows: one dense "list".  L2 and inner product run on the matrix cores
// (L2: candidates by the expansion, the reference's sum((q - x)^2) for those, queries that cannot be proven
// complete redone exactly -- the scheme of the list scan), L1 and small batches on the vector-ALU kernels.
int pgv_exact_topk(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, int dim, const void *queries, int nq,
                   const void *rows, int64_t n, int k, float *out_dist, int64_t *out_idx) {
    if (!ctx || !out_dist || !out_idx) PGV_FAIL(PGV_ERR_ARG, "pgv_exact_topk: ctx/out_dist/out_idx is NULL");
    PGV_TRY(check_common(dtype, dim));
    PGV_TRY(check_metric(metric));
    if (nq < 0 || n < 0) PGV_FAIL(PGV_ERR_ARG, "pgv_exact_topk: nq/n < 0");
    if (k < 1 || k > 4096) PGV_FAIL(PGV_ERR_ARG, "pgv_exact_topk: k %d outside 1..4096", k);
    if (n > 0xffffffffll) PGV_FAIL(PGV_ERR_ARG, "pgv_exact_topk: more than 2^32 rows");
    if (nq == 0) return PGV_OK;
    if (!queries || (n > 0 && !rows)) PGV_FAIL(PGV_ERR_ARG, "pgv_exact_topk: queries/rows is NULL");
    PGV_HIP(hipSetDevice(ctx->device));
    const RowGeom g = row_geom(dim, dtype);
    const void *q_dev, *r_dev = nullptr;
    PGV_TRY(stage_rows(ctx, queries, nq, dim, dtype, g, ctx->q_stage, &q_dev));
    if (n > 0) PGV_TRY(stage_rows(ctx, rows, n, dim, dtype, g, ctx->rows_stage, &r_dev));
    const RowsView rv{r_dev, n, g, row_kind(dtype), metric};
    const size_t row_bytes = rv.row_bytes();
    OutArg od, oi;
    PGV_TRY(od.init(out_dist, sizeof(float) * (size_t)nq * k, ctx->out_stage));
    PGV_TRY(oi.init(out_idx, sizeof(int64_t) * (size_t)nq * k, ctx->out_stage2));

    // the distance matrix of a query chunk stays under 4 GiB (whole 128-query tiles of the dense kernel when it is that
    // large: 1024 queries x 1 M rows are ONE pass, every row tile read from HBM once)
    int chunk = n > 0 ? (int)std::min<int64_t>(nq, std::max<int64_t>(1, ((int64_t)1 << 30) / n)) : nq;
    if (chunk >= 128)
        chunk = chunk / 128 * 128;
    else if (chunk >= 64)
        chunk = chunk / 32 * 32;
    static const bool no_dense = [] {
        const char *e = getenv("PGV_NO_DENSE128");
        return e && atoi(e) != 0;
    }();
    const int kprime = approx_candidates(k);
    const bool l2_mfma = metric == PGV_L2SQ && kprime <= 256 && n > kprime;
    const bool mfma_ok = !ctx->no_mfma_scan && n >= 64 && (metric == PGV_NEG_IP || l2_mfma);
    float *norms = nullptr;
    if (mfma_ok && l2_mfma && nq >= 64) {
        PGV_TRY(ctx->xt_norms.ensure(sizeof(float) * ((size_t)n + 1)));
        norms = ctx->xt_norms.as<float>();
        PGV_HIP(hipMemsetAsync(norms + n, 0, sizeof(float), ctx->stream));
        PGV_TRY(launch_row_norms(ctx, rv, norms, reinterpret_cast<unsigned *>(norms + n)));
    }
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int cn = std::min(chunk, nq - q0);
        const char *qp = static_cast<const char *>(q_dev) + (size_t)q0 * row_bytes;
        float *cd = od.as<float>() + (size_t)q0 * k;
        int64_t *ci = oi.as<int64_t>() + (size_t)q0 * k;
        PGV_TRY(ctx->dist_mat.ensure(sizeof(float) * std::max<size_t>((size_t)cn * (size_t)n, 4)));
        float *mat = ctx->dist_mat.as<float>();
        const bool mfma = mfma_ok && cn >= 64;
        // 128 queries x 128 rows per workgroup (kernels_dense.hip) from 128 queries on: the rows are streamed once per
        // 128 queries instead of once per 32
        const bool dense128 = mfma && cn >= 128 && n >= 128 && !no_dense;
        if (mfma && metric == PGV_L2SQ) {
            ExactTail tail;
            tail.rows = {r_dev, nullptr, nullptr, g, dtype, reinterpret_cast<const unsigned *>(norms + n)};
            tail.queries = qp;
            tail.nq = cn;
            tail.kprime = kprime;
            tail.k = k;
            tail.approx = mat;
            tail.fixed_len = n;  // a row's position in the matrix row is its index
            // the candidates are proven complete with the rounding bound of the kernel that produced the values
            tail.bound = scan_bound_chain(ctx, g.ld, dense128 ? dense_chain_length(g, dtype)
                                                              : scan_chain_length(g, dtype, false));
            tail.out_dist = cd;
            tail.out_slot = ci;
            if (dense128)
                PGV_TRY(launch_mfma_dense(ctx, metric, dtype, g, r_dev, n, qp, cn, norms, mat, n));
            else
                PGV_TRY(dense_scan(ctx, rv, qp, cn, n, mat, true, norms, nullptr));
            PGV_TRY(launch_exact_tail(ctx, tail, ctx->ms_b));
        } else {
            if (dense128)
                PGV_TRY(launch_mfma_dense(ctx, metric, dtype, g, r_dev, n, qp, cn, nullptr, mat, n));
            else
                PGV_TRY(dense_scan(ctx, rv, qp, cn, n, mat, mfma, nullptr, nullptr));
            PGV_TRY(launch_topk_segments(ctx, mat, nullptr, cn, n, k, cd, ci));
        }
    }
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    PGV_TRY(oi.finish(ctx, &need));
    return sync_if(ctx, need);
}

int pgv_cosine_distance_batch(pgv_ctx *ctx, pgv_dtype dtype, int dim, const void *query, const void *rows,
                              int64_t n, double *out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_cosine_distance_batch: ctx/out is NULL");
    PGV_TRY(check_common(dtype, dim));
    if (n < 0) PGV_FAIL(PGV_ERR_ARG, "n < 0");
    if (n == 0) return PGV_OK;
    if (!query || !rows) PGV_FAIL(PGV_ERR_ARG, "query/rows is NULL");
    PGV_HIP(hipSetDevice(ctx->device));
    const RowGeom g = row_geom(dim, dtype);
    const void *q_dev, *r_dev;
    PGV_TRY(stage_rows(ctx, query, 1, dim, dtype, g, ctx->q_stage, &q_dev));
    PGV_TRY(stage_rows(ctx, rows, n, dim, dtype, g, ctx->rows_stage, &r_dev));
    OutArg od;
    PGV_TRY(od.init(out, sizeof(double) * (size_t)n, ctx->out_stage));
    PGV_TRY(launch_cosine(ctx, dtype, g, r_dev, q_dev, n, od.as<double>()));
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    return sync_if(ctx, need);
}

int pgv_bit_distance_batch(pgv_ctx *ctx, pgv_bit_metric metric, int nbits, const void *query, const void *rows,
                           int64_t n, double *out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_bit_distance_batch: ctx/out is NULL");
    if (metric != PGV_BIT_HAMMING && metric != PGV_BIT_JACCARD) PGV_FAIL(PGV_ERR_ARG, "unknown bit metric %d", (int)metric);
    if (nbits < 0 || nbits > 64000 * 8) PGV_FAIL(PGV_ERR_DIMS, "bit length %d out of range", nbits);
    if (n < 0) PGV_FAIL(PGV_ERR_ARG, "n < 0");
    if (n == 0) return PGV_OK;
    if (!rows || (nbits > 0 && !query)) PGV_FAIL(PGV_ERR_ARG, "query/rows is NULL");
    PGV_HIP(hipSetDevice(ctx->device));
    OutArg od;
    PGV_TRY(od.init(out, sizeof(double) * (size_t)n, ctx->out_stage));
    const int bytes = (nbits + 7) / 8;  // VARBITBYTES
    if (bytes == 0) {
        // empty bit strings: hamming 0, jaccard 1 (no common bit), src/bitutils.c:71, :127-128
        std::vector<double> v((size_t)n, metric == PGV_BIT_HAMMING ? 0.0 : 1.0);
        PGV_HIP(hipMemcpyAsync(od.as<double>(), v.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        PGV_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        // bytes are staged like fp16 elements of a (bytes / 2)-dimensional row would be: zero-padded to whole
        // 16-byte vectors (an odd byte count is padded by the 2-D copy as well)
        const RowGeom g = bit_row_geom(nbits);
        const void *q_dev, *r_dev;
        PGV_TRY(stage_rows(ctx, query, 1, bytes, g.ld, ctx->q_stage, &q_dev));
        PGV_TRY(stage_rows(ctx, rows, n, bytes, g.ld, ctx->rows_stage, &r_dev));
        PGV_TRY(launch_bit_distance(ctx, metric == PGV_BIT_HAMMING ? 0 : 1, g, r_dev, q_dev, n, od.as<double>()));
    }
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    return sync_if(ctx, need);
}

namespace {
struct BitGeom {
    int bytes, row_ld, q_ld;  // VARBITBYTES | padded to 16-byte vectors | padded to the kernels' register slices
};
BitGeom bit_geom(int nbits) {
    BitGeom g;
    g.bytes = (nbits + 7) / 8;
    g.row_ld = (g.bytes + 15) / 16 * 16;
    g.q_ld = bit_query_bytes(nbits);
    return g;
}
// staged bit rows [n x ld bytes] (ld: row_ld or q_ld) as the Hamming kernels take them
RowsView bit_rows(const void *rows, int64_t n, int ld) { return {rows, n, bit_row_geom(ld * 8), RowKind::Bits, PGV_L1}; }
}  // namespace

// `ORDER BY b <~> $1 LIMIT k` without an index for a batch of queries: pgv_exact_topk's structure over packed bits.  The
// scan (hamming_tile_kernel, kernels_bit.hip) fills the chunk's distance matrix mat[q * n + row] with the integer counts
// as floats (exact: at most 512 000), launch_topk_segments selects with ties to the lower row.
int pgv_bit_topk(pgv_ctx *ctx, int nbits, const void *queries, int nq, const void *rows, int64_t n, int k, float *out_dist,
                 int64_t *out_idx) {
    if (!ctx || !out_dist || !out_idx) PGV_FAIL(PGV_ERR_ARG, "pgv_bit_topk: ctx/out_dist/out_idx is NULL");
    if (nbits < 0 || nbits > 64000 * 8) PGV_FAIL(PGV_ERR_DIMS, "bit length %d out of range", nbits);
    if (nq < 0 || n < 0) PGV_FAIL(PGV_ERR_ARG, "pgv_bit_topk: nq/n < 0");
    if (k < 1 || k > 4096) PGV_FAIL(PGV_ERR_ARG, "pgv_bit_topk: k %d outside 1..4096", k);
    if (n > 0xffffffffll) PGV_FAIL(PGV_ERR_ARG, "pgv_bit_topk: more than 2^32 rows");
    if (nq == 0) return PGV_OK;
    if (nbits > 0 && (!queries || (n > 0 && !rows))) PGV_FAIL(PGV_ERR_ARG, "pgv_bit_topk: queries/rows is NULL");
    PGV_HIP(hipSetDevice(ctx->device));
    const int bytes = (nbits + 7) / 8;  // VARBITBYTES
    // rows in whole 16-byte vectors like pgv_bit_distance_batch's, queries in whole register slices of the scan kernel
    const BitGeom g = bit_geom(nbits);
    const int q_ld = g.q_ld;
    const void *q_dev = nullptr, *r_dev = nullptr;
    if (bytes > 0 && n > 0) {
        PGV_TRY(stage_rows(ctx, queries, nq, bytes, q_ld, ctx->q_stage, &q_dev));
        PGV_TRY(stage_rows(ctx, rows, n, bytes, g.row_ld, ctx->rows_stage, &r_dev));
    }
    OutArg od, oi;
    PGV_TRY(od.init(out_dist, sizeof(float) * (size_t)nq * k, ctx->out_stage));
    PGV_TRY(oi.init(out_idx, sizeof(int64_t) * (size_t)nq * k, ctx->out_stage2));

    // the distance matrix of a query chunk stays at or under 2^30 floats, in whole 32-query tiles of the scan kernel
    int chunk = n > 0 ? (int)std::min<int64_t>(nq, std::max<int64_t>(1, ((int64_t)1 << 30) / n)) : nq;
    if (chunk >= 32) chunk = chunk / 32 * 32;
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int cn = std::min(chunk, nq - q0);
        PGV_TRY(ctx->dist_mat.ensure(sizeof(float) * std::max<size_t>((size_t)cn * (size_t)n, 4)));
        float *mat = ctx->dist_mat.as<float>();
        if (n > 0 && bytes == 0) {
            // empty bit strings: every distance is 0 (src/bitutils.c:71), so the ties leave rows 0 .. k - 1
            PGV_HIP(hipMemsetAsync(mat, 0, sizeof(float) * (size_t)cn * (size_t)n, ctx->stream));
        } else if (n > 0) {
            ScanTimer timer{ctx};
            PGV_TRY(timer.begin((double)n * cn, (double)n * ((cn + 31) / 32), true));
            PGV_TRY(launch_hamming_tiles(ctx, bit_rows(r_dev, n, g.row_ld), static_cast<const char *>(q_dev) + (size_t)q0 * q_ld,
                                         q_ld, cn, mat));
            PGV_TRY(timer.end());
        }
        PGV_TRY(launch_topk_segments(ctx, mat, nullptr, cn, n, k, od.as<float>() + (size_t)q0 * k,
                                     oi.as<int64_t>() + (size_t)q0 * k));
    }
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    PGV_TRY(oi.finish(ctx, &need));
    return sync_if(ctx, need);
}

int pgv_binary_quantize(pgv_ctx *ctx, pgv_dtype dtype, int dim, const void *rows, int64_t n, void *out_bits) {
    if (!ctx || !out_bits) PGV_FAIL(PGV_ERR_ARG, "pgv_binary_quantize: ctx/out_bits is NULL");
    PGV_TRY(check_common(dtype, dim));
    if (n < 0) PGV_FAIL(PGV_ERR_ARG, "n < 0");
    if (n == 0) return PGV_OK;
    if (!rows) PGV_FAIL(PGV_ERR_ARG, "rows is NULL");
    PGV_HIP(hipSetDevice(ctx->device));
    const void *r_dev;
    PGV_TRY(stage_flat(ctx, rows, (size_t)n * dim * elem_size(dtype), ctx->rows_stage, &r_dev));
    OutArg ob;
    PGV_TRY(ob.init(out_bits, (size_t)n * ((dim + 7) / 8), ctx->out_stage));
    PGV_TRY(launch_binary_quantize(ctx, dtype, dim, r_dev, n, ob.dev));
    bool need = false;
    PGV_TRY(ob.finish(ctx, &need));
    return sync_if(ctx, need);
}

// The outer ORDER BY of the two-stage query: each query's real candidates packed to the front of its row (stably),
// score_gather_kernel (pgv_hnsw_score's exact per-pair kernel) over the nq x kc (candidate, query) pairs, NaN for the
// "none" tail, launch_topk_segments over segments of kc (float8 order, ties to the lower position: every real candidate,
// +inf and NaN ones included, before any "none"), positions back to row indexes and the tail to +inf / -1.
int pgv_rerank(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, int dim, const void *queries, int nq, const void *rows,
               int64_t n, const int64_t *cand, int kc, int k, float *out_dist, int64_t *out_idx) {
    if (!ctx || !out_dist || !out_idx) PGV_FAIL(PGV_ERR_ARG, "pgv_rerank: ctx/out_dist/out_idx is NULL");
    PGV_TRY(check_common(dtype, dim));
    PGV_TRY(check_metric(metric));
    if (nq < 0 || n < 0) PGV_FAIL(PGV_ERR_ARG, "pgv_rerank: nq/n < 0");
    if (kc < 1 || kc > 4096) PGV_FAIL(PGV_ERR_ARG, "pgv_rerank: kc %d outside 1..4096", kc);
    if (k < 1 || k > kc) PGV_FAIL(PGV_ERR_ARG, "pgv_rerank: k %d outside 1..kc = %d", k, kc);
    if (n > 0x7fffffffll) PGV_FAIL(PGV_ERR_ARG, "pgv_rerank: more than 2^31 - 1 rows");
    if (nq == 0) return PGV_OK;
    if (!queries || !cand || (n > 0 && !rows)) PGV_FAIL(PGV_ERR_ARG, "pgv_rerank: queries/cand/rows is NULL");
    PGV_HIP(hipSetDevice(ctx->device));
    const int64_t total = (int64_t)nq * kc;
    if (!is_device_ptr(cand))
        for (int64_t i = 0; i < total; i++)
            if (cand[i] < -1 || cand[i] >= n)
                PGV_FAIL(PGV_ERR_ARG, "pgv_rerank: candidate %lld of query %lld outside -1..%lld", (long long)cand[i],
                         (long long)(i / kc), (long long)n - 1);
    const RowGeom g = row_geom(dim, dtype);
    const void *q_dev, *r_dev = nullptr, *c_dev;
    PGV_TRY(stage_rows(ctx, queries, nq, dim, dtype, g, ctx->q_stage, &q_dev));
    if (n > 0) PGV_TRY(stage_rows(ctx, rows, n, dim, dtype, g, ctx->rows_stage, &r_dev));
    PGV_TRY(stage_flat(ctx, cand, sizeof(int64_t) * (size_t)total, ctx->idx_stage, &c_dev));
    const int64_t *cd = static_cast<const int64_t *>(c_dev);
    OutArg od, oi;
    PGV_TRY(od.init(out_dist, sizeof(float) * (size_t)nq * k, ctx->out_stage));
    PGV_TRY(oi.init(out_idx, sizeof(int64_t) * (size_t)nq * k, ctx->out_stage2));
    // plan_a: packed[total] | slot[total] | query_of[total]   plan_b: values[total]   plan_c: selected positions [nq x k]
    PGV_TRY(ctx->plan_a.ensure((sizeof(int64_t) + sizeof(int32_t) * 2) * (size_t)total));
    PGV_TRY(ctx->plan_b.ensure(sizeof(float) * (size_t)total));
    PGV_TRY(ctx->plan_c.ensure(sizeof(int64_t) * (size_t)nq * k));
    int64_t *packed = ctx->plan_a.as<int64_t>();
    int32_t *slot = reinterpret_cast<int32_t *>(packed + total), *query_of = slot + total;
    float *vals = ctx->plan_b.as<float>();
    int64_t *pos = ctx->plan_c.as<int64_t>();
    PGV_TRY(launch_rerank_pairs(ctx, cd, nq, kc, packed, slot, query_of));
    if (n > 0)
        PGV_TRY(launch_score_gather(ctx, RowsView{r_dev, n, g, row_kind(dtype), metric}, q_dev, slot, query_of, total, vals));
    PGV_TRY(launch_rerank_mask(ctx, packed, total, vals));  // (n == 0: every entry is "none")
    PGV_TRY(launch_topk_segments(ctx, vals, nullptr, nq, kc, k, od.as<float>(), pos));
    PGV_TRY(launch_rerank_map(ctx, packed, nq, kc, k, pos, oi.as<int64_t>(), od.as<float>()));
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    PGV_TRY(oi.finish(ctx, &need));
    return sync_if(ctx, need);
}

// ------------------------------------------------------------- k-means++ seeding
// (prototypes and what the two parts promise: pgv_abi_common.h)
int kmpp_begin(pgv_ctx *ctx, int n_local, int k, int64_t n_total, Rng &rng, KmppState *state, int64_t *first) {
    const size_t nw = n_local > 0 ? (size_t)n_local : 1;
    KmppState &st = *state;
    st.nblocks = n_local > 0 ? kmpp_block_count(n_local) : 0;
    PGV_TRY(ctx->km_a.ensure(sizeof(float) * 2 * nw));
    PGV_TRY(ctx->km_b.ensure(sizeof(double) * ((size_t)st.nblocks + (size_t)k + 1)));
    PGV_TRY(ctx->km_c.ensure(sizeof(int32_t) * (size_t)k));
    st.weight = ctx->km_a.as<float>();
    st.raw = st.weight + nw;
    st.block_sums = ctx->km_b.as<double>();
    st.draws_dev = st.block_sums + st.nblocks;
    st.picked = ctx->km_c.as<int32_t>();

    // the reference draws RandomInt() once, then one RandomDouble() per further center
    // (src/ivfkmeans.c:36, :77): pre-draw them in that order
    *first = (int64_t)(rng.next_u32() % (uint32_t)n_total);
    PGV_TRY(ctx->h_b.ensure(sizeof(double) * (size_t)k + sizeof(float) * nw));
    double *h_draws = ctx->h_b.as<double>();
    for (int i = 0; i + 1 < k; i++) h_draws[i] = rng.next_double();
    float *h_w = reinterpret_cast<float *>(h_draws + k);
    for (int j = 0; j < n_local; j++) h_w[j] = 3.402823466e+38f;  // FLT_MAX (:39-40)
    PGV_HIP(hipMemcpyAsync(st.draws_dev, h_draws, sizeof(double) * (size_t)k, hipMemcpyHostToDevice, ctx->stream));
    if (n_local > 0)
        PGV_HIP(hipMemcpyAsync(st.weight, h_w, sizeof(float) * (size_t)n_local, hipMemcpyHostToDevice, ctx->stream));
    return PGV_OK;
}

int kmpp_round_weights(pgv_ctx *ctx, const RowsView &sv, const void *center_i, const KmppState &st) {
    // distance of every sample to the newest center only (:52-60)
    if (sv.bits())
        PGV_TRY(launch_hamming_tiles(ctx, sv, center_i, (int)sv.row_bytes(), 1, st.raw));
    else
        PGV_TRY(dense_scan(ctx, sv, center_i, 1, 0, st.raw));
    const int mode = sv.bits() ? 2 : (sv.metric == PGV_NEG_IP ? 1 : 0);
    return launch_kmpp_update(ctx, st.raw, st.weight, (int)sv.n, mode, st.block_sums);
}

// k-means++ over staged samples (kmeans_rows, or bit rows at the queries' stride) into device centers at the samples'
// stride
static int kmeanspp_dev(pgv_ctx *ctx, const RowsView &sv, int k, Rng &rng, void *centers_dev) {
    const int n = (int)sv.n;
    const size_t row_bytes = sv.row_bytes();
    KmppState st;
    int64_t first;
    PGV_TRY(kmpp_begin(ctx, n, k, n, rng, &st, &first));
    PGV_HIP(hipMemcpyAsync(centers_dev, static_cast<const char *>(sv.rows) + (size_t)first * row_bytes, row_bytes,
                           hipMemcpyDeviceToDevice, ctx->stream));
    const int32_t first_i = (int32_t)first;
    PGV_HIP(hipMemcpyAsync(st.picked, &first_i, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i + 1 < k; i++) {
        PGV_TRY(kmpp_round_weights(ctx, sv, static_cast<const char *>(centers_dev) + (size_t)i * row_bytes, st));
        PGV_TRY(launch_kmpp_pick(ctx, sv.geom, sv.rows, n, st.weight, st.block_sums, st.draws_dev, i, centers_dev,
                                 st.picked));
    }
    return PGV_OK;
}

// ------------------------------------------------------ k-means over bit strings
// `USING ivfflat (col bit_hamming_ops)` on the build side.  The samples are staged as the QUERIES of hamming_tile_kernel
// (rows of whole register slices, BitGeom::q_ld bytes), the centers as its rows: a chunk's matrix mat[sample][center]
// then holds a sample's distances side by side, launch_topk_segments(k = 1) finds its first minimum (ties to the lower
// center) and bit_closest_kernel decides.  During k-means the centers live at the samples' stride as well, so that a
// center is a row of the assignment, the query of a k-means++ round and the target of launch_kmpp_pick's row copy.
namespace {
int check_bits(int nbits, const char *who) {
    // IVFFLAT_MAX_DIM * 32 (src/ivfutils.c:416)
    if (nbits < 1 || nbits > kIvfMaxBits) PGV_FAIL(PGV_ERR_DIMS, "%s: bit length %d outside 1..%d", who, nbits, kIvfMaxBits);
    return PGV_OK;
}

// samples [n x q_ld] (device, staged) to their centers (device, staged; bit_rows): closest_io / out_dist / counts /
// changes as launch_bit_closest takes them (device).  The matrix stays at or under 2^30 floats per chunk of samples
int bit_closest_dev(pgv_ctx *ctx, const void *s_dev, int q_ld, int64_t n, const RowsView &centers, bool sticky,
                    int32_t *closest_io, float *out_dist, int32_t *counts, unsigned long long *changes) {
    const int k = (int)centers.n;
    int64_t chunk = std::min<int64_t>(n, std::max<int64_t>(1, ((int64_t)1 << 30) / k));
    if (chunk >= 32) chunk = chunk / 32 * 32;
    PGV_TRY(ctx->dist_mat.ensure(sizeof(float) * std::max<size_t>((size_t)chunk * (size_t)k, 4)));
    PGV_TRY(ctx->sel_a.ensure(sizeof(int64_t) * (size_t)chunk));
    PGV_TRY(ctx->sel_b.ensure(sizeof(float) * (size_t)chunk));
    float *mat = ctx->dist_mat.as<float>(), *best_val = ctx->sel_b.as<float>();
    int64_t *best_pos = ctx->sel_a.as<int64_t>();
    for (int64_t j0 = 0; j0 < n; j0 += chunk) {
        const int cn = (int)std::min<int64_t>(chunk, n - j0);
        ScanTimer timer{ctx};
        PGV_TRY(timer.begin((double)cn * k, (double)k * ((cn + 31) / 32), true));
        PGV_TRY(launch_hamming_tiles(ctx, centers, static_cast<const char *>(s_dev) + (size_t)j0 * q_ld, q_ld, cn, mat));
        PGV_TRY(timer.end());
        PGV_TRY(launch_topk_segments(ctx, mat, nullptr, cn, k, 1, best_val, best_pos));
        PGV_TRY(launch_bit_closest(ctx, mat, k, best_val, best_pos, cn, sticky, closest_io + j0, out_dist ? out_dist + j0 : nullptr,
                                   counts, changes));
    }
    return PGV_OK;
}

// ComputeNewCenters + BitUpdateCenter (src/ivfkmeans.c:205-231, src/ivfutils.c:325-339) from the assignment: per-center
// bit counts on the device, the empty clusters' draws on the host -- nbits RandomDouble() each, x = (float) draw,
// bit = x > 0.5, clusters in center order and bits in bit order -- like lloyd_finish_dev.  h_counts: the cluster sizes
// on the host.  centers_dev [k x c_ld] is rewritten.  km_e: sums | refill_row | refill
int bit_update_centers_dev(pgv_ctx *ctx, int nbits, const BitGeom &g, const void *s_dev, int n, const int32_t *closest_dev,
                           const int32_t *counts_dev, const int32_t *h_counts, int k, Rng &rng, void *centers_dev, int c_ld) {
    const size_t sums_bytes = (sizeof(int32_t) * (size_t)k * (size_t)nbits + 255) & ~(size_t)255;
    const size_t row_bytes = (sizeof(int32_t) * (size_t)k + 255) & ~(size_t)255;
    int nempty = 0;
    PGV_TRY(refill_empty_clusters(ctx, h_counts, k, sums_bytes, row_bytes, (size_t)g.bytes, [&](void *row) {
        uint8_t *fill = static_cast<uint8_t *>(row);
        for (int i = 0; i < nbits; i++) {
            const float x = (float)rng.next_double();
            if (x > 0.5f) fill[i / 8] |= (uint8_t)(1u << (7 - i % 8));
        }
    }, &nempty));
    int32_t *sums = ctx->km_e.as<int32_t>();
    int32_t *refill_row = reinterpret_cast<int32_t *>(ctx->km_e.as<char>() + sums_bytes);
    uint8_t *refill = reinterpret_cast<uint8_t *>(ctx->km_e.as<char>() + sums_bytes + row_bytes);
    PGV_HIP(hipMemsetAsync(sums, 0, sums_bytes, ctx->stream));
    PGV_TRY(launch_bit_sums(ctx, s_dev, g.q_ld, nbits, n, closest_dev, sums));
    return launch_bit_centers(ctx, sums, counts_dev, k, nbits, c_ld, nempty > 0 ? refill_row : nullptr, refill, centers_dev);
}

// one iteration on staged samples and centers (both at stride q_ld): assignment, counts, changes, new centers in place.
// km_f: counts[k] | changes.  *out_changes and h_counts (host, [k]) are valid on return
int bit_lloyd_dev(pgv_ctx *ctx, int nbits, const BitGeom &g, const void *s_dev, int n, void *centers_dev, int k,
                  int32_t *closest_dev, Rng &rng, int32_t **counts_dev_out, std::vector<int32_t> &h_counts,
                  unsigned long long *out_changes) {
    const size_t cb = (sizeof(int32_t) * (size_t)k + 7) & ~(size_t)7;
    PGV_TRY(ctx->km_f.ensure(cb + sizeof(unsigned long long)));
    int32_t *counts = ctx->km_f.as<int32_t>();
    unsigned long long *changes = reinterpret_cast<unsigned long long *>(ctx->km_f.as<char>() + cb);
    PGV_HIP(hipMemsetAsync(counts, 0, cb + sizeof(unsigned long long), ctx->stream));
    if (n > 0) PGV_TRY(bit_closest_dev(ctx, s_dev, g.q_ld, n, bit_rows(centers_dev, k, g.q_ld), true, closest_dev, nullptr, counts,
                                       changes));
    h_counts.assign((size_t)k, 0);
    PGV_HIP(hipMemcpyAsync(h_counts.data(), counts, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
    PGV_HIP(hipMemcpyAsync(out_changes, changes, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    PGV_TRY(bit_update_centers_dev(ctx, nbits, g, s_dev, n, closest_dev, counts, h_counts.data(), k, rng, centers_dev, g.q_ld));
    *counts_dev_out = counts;
    return PGV_OK;
}

}  // namespace

// AddTupleToSort's argmin (src/ivfbuild.c:183-192) under hamming_distance: `distance < minDistance` keeps the first
// strictly-smallest center
int pgv_bit_assign(pgv_ctx *ctx, int nbits, const void *centers, int k, const void *rows, int64_t n, int32_t *out_list,
                   float *out_dist) {
    if (!ctx || !out_list) PGV_FAIL(PGV_ERR_ARG, "pgv_bit_assign: ctx/out_list is NULL");
    PGV_TRY(check_bits(nbits, "pgv_bit_assign"));
    if (k < 1 || !centers) PGV_FAIL(PGV_ERR_ARG, "need at least one center");
    if (n < 0) PGV_FAIL(PGV_ERR_ARG, "n < 0");
    if (n == 0) return PGV_OK;
    if (!rows) PGV_FAIL(PGV_ERR_ARG, "rows is NULL");
    PGV_HIP(hipSetDevice(ctx->device));
    const BitGeom g = bit_geom(nbits);
    const void *c_dev;
    PGV_TRY(stage_rows(ctx, centers, k, g.bytes, g.row_ld, ctx->centers_stage, &c_dev));
    const RowsView cv = bit_rows(c_dev, k, g.row_ld);
    return assign_in_slabs(ctx, rows, n, (size_t)g.bytes, (size_t)g.q_ld, out_list, out_dist,
                           [&](const void *r_dev, int64_t cnt, int32_t *idx, float *val) {
                               return bit_closest_dev(ctx, r_dev, g.q_ld, cnt, cv, false, idx, val, nullptr, nullptr);
                           });
}

int pgv_bit_lloyd_step(pgv_ctx *ctx, int nbits, const void *samples, int n, const void *centers, int k, int32_t *io_closest,
                       const pgv_rng *rng, void *out_centers, int32_t *out_counts, int64_t *out_changes) {
    if (!ctx || !io_closest || !out_centers || !out_counts || !out_changes)
        PGV_FAIL(PGV_ERR_ARG, "pgv_bit_lloyd_step: NULL argument");
    PGV_TRY(check_bits(nbits, "pgv_bit_lloyd_step"));
    if (k < 1 || k > 32768 || n < 0 || !centers || (n > 0 && !samples)) PGV_FAIL(PGV_ERR_ARG, "bad sizes");
    if (n >= (1 << 24)) PGV_FAIL(PGV_ERR_ARG, "pgv_bit_lloyd_step: %d samples, at most 2^24 - 1", n);
    PGV_HIP(hipSetDevice(ctx->device));
    const BitGeom g = bit_geom(nbits);
    const void *s_dev = nullptr;
    if (n > 0) PGV_TRY(stage_rows(ctx, samples, n, g.bytes, g.q_ld, ctx->rows_stage, &s_dev));
    // a staging that is a copy even of device rows: the centers are rewritten in place
    PGV_TRY(ctx->centers_stage.ensure((size_t)k * g.q_ld));
    PGV_TRY(put_padded_rows(ctx->stream, ctx->centers_stage.p, g.q_ld, centers, g.bytes, k));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    int32_t *closest_dev = io_closest;
    const bool closest_is_dev = is_device_ptr(io_closest);
    if (!closest_is_dev) {
        // (an assignment on the device is not checked: it comes from an earlier step)
        for (int j = 0; j < n; j++)
            if (io_closest[j] < -1 || io_closest[j] >= k)
                PGV_FAIL(PGV_ERR_ARG, "pgv_bit_lloyd_step: io_closest[%d] = %d outside -1..%d", j, io_closest[j], k - 1);
        PGV_TRY(ctx->idx_stage.ensure(sizeof(int32_t) * (size_t)(n > 0 ? n : 1)));
        closest_dev = ctx->idx_stage.as<int32_t>();
        if (n) PGV_HIP(hipMemcpyAsync(closest_dev, io_closest, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    }
    Rng r(rng);
    int32_t *counts_dev = nullptr;
    std::vector<int32_t> h_counts;
    unsigned long long changes = 0;
    PGV_TRY(bit_lloyd_dev(ctx, nbits, g, s_dev, n, ctx->centers_stage.p, k, closest_dev, r, &counts_dev, h_counts, &changes));
    PGV_TRY(unstage_rows(ctx, ctx->centers_stage.p, k, g.bytes, g.q_ld, out_centers));
    const int64_t ch = (int64_t)changes;
    if (is_device_ptr(out_counts))
        PGV_HIP(hipMemcpyAsync(out_counts, h_counts.data(), sizeof(int32_t) * (size_t)k, hipMemcpyHostToDevice, ctx->stream));
    else
        memcpy(out_counts, h_counts.data(), sizeof(int32_t) * (size_t)k);
    if (is_device_ptr(out_changes))
        PGV_HIP(hipMemcpyAsync(out_changes, &ch, sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    else
        *out_changes = ch;
    if (!closest_is_dev && n)
        PGV_HIP(hipMemcpyAsync(io_closest, closest_dev, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    return pgv_ctx_sync(ctx);
}

int pgv_bit_kmeans(pgv_ctx *ctx, int nbits, const void *samples, int n, int k, int max_iterations, const pgv_rng *rng,
                   void *out_centers, int32_t *out_closest, int *out_iters) {
    if (!ctx || !out_centers) PGV_FAIL(PGV_ERR_ARG, "pgv_bit_kmeans: ctx/out_centers is NULL");
    PGV_TRY(check_bits(nbits, "pgv_bit_kmeans"));
    if (k < 1 || k > 32768) PGV_FAIL(PGV_ERR_ARG, "lists %d outside 1..32768", k);
    // the reference's float sums stop counting at 2^24 (src/ivfutils.c:369): refused before the samples are touched
    if (n >= (1 << 24)) PGV_FAIL(PGV_ERR_ARG, "pgv_bit_kmeans: %d samples, at most 2^24 - 1", n);
    if (n < 0 || (n > 0 && !samples)) PGV_FAIL(PGV_ERR_ARG, "bad samples");
    if (max_iterations <= 0) max_iterations = 500;  // src/ivfkmeans.c:347
    PGV_HIP(hipSetDevice(ctx->device));
    const BitGeom g = bit_geom(nbits);
    Rng r(rng);
    PGV_TRY(ctx->centers_stage.ensure((size_t)k * g.q_ld));
    void *centers_dev = ctx->centers_stage.p;
    PGV_HIP(hipMemsetAsync(centers_dev, 0, (size_t)k * g.q_ld, ctx->stream));
    int iters = 0;
    int32_t *counts_dev = nullptr;
    std::vector<int32_t> h_counts;
    unsigned long long changes = 0;
    if (n == 0) {
        // RandomCenters (src/ivfkmeans.c:110-133): every cluster is drawn
        PGV_TRY(bit_lloyd_dev(ctx, nbits, g, nullptr, 0, centers_dev, k, nullptr, r, &counts_dev, h_counts, &changes));
    } else {
        const void *s_dev;
        PGV_TRY(stage_rows(ctx, samples, n, g.bytes, g.q_ld, ctx->rows_stage, &s_dev));
        // InitCenters (src/ivfkmeans.c:23-91): the distance to the newest center is the Hamming count,
        // weight = min(weight, (float) d^2), the sum and the pick in double
        PGV_TRY(kmeanspp_dev(ctx, bit_rows(s_dev, n, g.q_ld), k, r, centers_dev));
        PGV_TRY(ctx->km_g.ensure(sizeof(int32_t) * (size_t)n));
        int32_t *closest = ctx->km_g.as<int32_t>();
        PGV_HIP(hipMemsetAsync(closest, 0xff, sizeof(int32_t) * (size_t)n, ctx->stream));  // -1: not assigned yet
        for (int it = 0; it < max_iterations; it++) {
            iters = it + 1;
            PGV_TRY(bit_lloyd_dev(ctx, nbits, g, s_dev, n, centers_dev, k, closest, r, &counts_dev, h_counts, &changes));
            // stop when an iteration other than the first moves nothing (src/ivfkmeans.c:482-483)
            if (changes == 0 && it != 0) break;
        }
        if (out_closest)
            PGV_HIP(hipMemcpyAsync(out_closest, closest, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, ctx->stream));
    }
    // (CheckCenters, src/ivfkmeans.c:539-547, has nothing to find in bit strings)
    PGV_TRY(unstage_rows(ctx, centers_dev, k, g.bytes, g.q_ld, out_centers));
    if (out_iters) *out_iters = iters;
    return pgv_ctx_sync(ctx);
}

// --------------------------------------------------------------------- k-means

// assignment + per-center sums/counts for staged samples; all outputs device
int lloyd_partial_dev(pgv_ctx *ctx, pgv_ops ops, pgv_dtype dtype, const RowGeom &g,
                             const void *samples_dev, int n, const void *centers_dev, int k,
                             int32_t *closest_io, float *sums /*[k x ld]*/, int32_t *counts,
                             unsigned long long *changes) {
    // km_d: closest_new[n] | offsets[k+1] | members[n]
    PGV_TRY(ctx->km_d.ensure(sizeof(int32_t) * (2 * (size_t)n + (size_t)k + 1)));
    int32_t *closest_new = ctx->km_d.as<int32_t>();
    int32_t *offsets = closest_new + n;
    int32_t *members = offsets + k + 1;
    PGV_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)k, ctx->stream));
    PGV_HIP(hipMemsetAsync(changes, 0, sizeof(unsigned long long), ctx->stream));
    if (n > 0) {
        PGV_TRY(launch_argmin_mode(ctx, spherical(ops) ? 3 : 0, dtype, g, samples_dev, n, centers_dev, k,
                                   closest_new, nullptr));
        PGV_TRY(launch_changes_hist(ctx, closest_new, closest_io, n, counts, changes));
    }
    PGV_TRY(launch_members(ctx, closest_io, n, k, counts, offsets, members));
    PGV_TRY(launch_center_sums(ctx, dtype, g, samples_dev, offsets, members, k, sums));
    return PGV_OK;
}

// centers from (all-reduced) sums/counts; counts_host tells which clusters are empty
int lloyd_finish_dev(pgv_ctx *ctx, pgv_ops ops, pgv_dtype dtype, const RowGeom &g, int dim, int k,
                            const float *sums_dev, const int32_t *counts_dev, const int32_t *counts_host,
                            Rng &rng, void *centers_dev) {
    // empty clusters take dim RandomDouble() draws each, in center order (src/ivfkmeans.c:222-227)
    int nempty = 0;
    PGV_TRY(refill_empty_clusters(ctx, counts_host, k, 0, sizeof(int32_t) * (size_t)k, sizeof(float) * (size_t)dim,
                                  [&](void *row) {
                                      for (int d = 0; d < dim; d++) static_cast<float *>(row)[d] = (float)rng.next_double();
                                  }, &nempty));
    int32_t *refill_row = ctx->km_e.as<int32_t>();
    float *refill = reinterpret_cast<float *>(refill_row + k);
    PGV_TRY(launch_finish_centers(ctx, dtype, g, k, dim, sums_dev, counts_dev, refill, refill_row, centers_dev));
    if (spherical(ops)) {
        PGV_TRY(ctx->km_f.ensure(64));
        int32_t *flag = ctx->km_f.as<int32_t>();
        PGV_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), ctx->stream));
        PGV_TRY(launch_normalize_rows(ctx, dtype, g, centers_dev, k, dim, flag));
    }
    return PGV_OK;
}

int check_centers_dev(pgv_ctx *ctx, pgv_ops ops, pgv_dtype dtype, const RowGeom &g, int dim, int k,
                             const void *centers_dev) {
    PGV_TRY(ctx->km_f.ensure(64));
    int32_t *flag = ctx->km_f.as<int32_t>();
    PGV_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), ctx->stream));
    PGV_TRY(launch_check_centers(ctx, dtype, g, centers_dev, k, dim, ops == PGV_OPS_COSINE ? 1 : 0, flag));
    int32_t h = 0;
    PGV_HIP(hipMemcpyAsync(&h, flag, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    // messages of src/ivfkmeans.c:507-510, :533
    if (h & 2) PGV_FAIL(PGV_ERR_DATA, "NaN detected. Please report a bug.");
    if (h & 4) PGV_FAIL(PGV_ERR_DATA, "Infinite value detected. Please report a bug.");
    if (h & 8) PGV_FAIL(PGV_ERR_DATA, "Zero norm detected. Please report a bug.");
    return PGV_OK;
}

int pgv_kmeanspp_init(pgv_ctx *ctx, pgv_ops ops, pgv_dtype dtype, int dim, const void *samples, int n,
                      int k, const pgv_rng *rng, void *out_centers) {
    if (!ctx || !out_centers) PGV_FAIL(PGV_ERR_ARG, "pgv_kmeanspp_init: ctx/out_centers is NULL");
    PGV_TRY(check_common(dtype, dim));
    PGV_TRY(check_ops(ops));
    if (k < 1 || n < 1 || !samples) PGV_FAIL(PGV_ERR_ARG, "need samples and k >= 1");
    PGV_HIP(hipSetDevice(ctx->device));
    const RowGeom g = row_geom(dim, dtype);
    const void *s_dev;
    PGV_TRY(stage_rows(ctx, samples, n, dim, dtype, g, ctx->rows_stage, &s_dev));
    PGV_TRY(ctx->centers_stage.ensure((size_t)k * g.ld * elem_size(dtype)));
    PGV_HIP(hipMemsetAsync(ctx->centers_stage.p, 0, (size_t)k * g.ld * elem_size(dtype), ctx->stream));
    Rng r(rng);
    PGV_TRY(kmeanspp_dev(ctx, kmeans_rows(ops, dtype, g, s_dev, n), k, r, ctx->centers_stage.p));
    PGV_TRY(unstage_rows(ctx, ctx->centers_stage.p, k, dim, dtype, g, out_centers));
    return pgv_ctx_sync(ctx);
}

int pgv_lloyd_partial(pgv_ctx *ctx, pgv_ops ops, pgv_dtype dtype, int dim, const void *samples, int n,
                      const void *centers, int k, int32_t *io_closest, float *out_sums,
                      int32_t *out_counts, int64_t *out_changes) {
    if (!ctx || !io_closest || !out_sums || !out_counts || !out_changes)
        PGV_FAIL(PGV_ERR_ARG, "pgv_lloyd_partial: NULL argument");
    PGV_TRY(check_common(dtype, dim));
    PGV_TRY(check_ops(ops));
    if (k < 1 || n < 0 || !centers || (n > 0 && !samples)) PGV_FAIL(PGV_ERR_ARG, "bad sizes");
    PGV_HIP(hipSetDevice(ctx->device));
    const RowGeom g = row_geom(dim, dtype);
    const void *s_dev, *c_dev;
    PGV_TRY(stage_rows(ctx, samples, n, dim, dtype, g, ctx->rows_stage, &s_dev));
    PGV_TRY(stage_rows(ctx, centers, k, dim, dtype, g, ctx->centers_stage, &c_dev));
    // closest is in/out
    int32_t *closest_dev = io_closest;
    const bool closest_is_dev = is_device_ptr(io_closest);
    if (!closest_is_dev) {
        PGV_TRY(ctx->idx_stage.ensure(sizeof(int32_t) * (size_t)(n > 0 ? n : 1)));
        closest_dev = ctx->idx_stage.as<int32_t>();
        if (n) PGV_HIP(hipMemcpyAsync(closest_dev, io_closest, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    }
    // sums are produced padded [k x ld]; hand back [k x dim]
    PGV_TRY(ctx->km_g.ensure(sizeof(float) * (size_t)k * g.ld + 64));
    float *sums_pad = ctx->km_g.as<float>();
    unsigned long long *changes_dev = reinterpret_cast<unsigned long long *>(sums_pad + (size_t)k * g.ld);
    OutArg oc;
    PGV_TRY(oc.init(out_counts, sizeof(int32_t) * (size_t)k, ctx->out_stage));
    PGV_TRY(lloyd_partial_dev(ctx, ops, dtype, g, s_dev, n, c_dev, k, closest_dev, sums_pad, oc.as<int32_t>(), changes_dev));
    const bool sums_dev = is_device_ptr(out_sums);
    PGV_HIP(hipMemcpy2DAsync(out_sums, sizeof(float) * (size_t)dim, sums_pad, sizeof(float) * (size_t)g.ld,
                             sizeof(float) * (size_t)dim, (size_t)k,
                             sums_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    const bool ch_dev = is_device_ptr(out_changes);
    PGV_HIP(hipMemcpyAsync(out_changes, changes_dev, sizeof(int64_t), ch_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    bool need = !sums_dev || !ch_dev;
    if (!closest_is_dev && n) {
        PGV_HIP(hipMemcpyAsync(io_closest, closest_dev, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        need = true;
    }
    PGV_TRY(oc.finish(ctx, &need));
    return sync_if(ctx, need);
}

int pgv_lloyd_finish(pgv_ctx *ctx, pgv_ops ops, pgv_dtype dtype, int dim, int k, const float *sums,
                     const int32_t *counts, const pgv_rng *rng, void *out_centers) {
    if (!ctx || !sums || !counts || !out_centers) PGV_FAIL(PGV_ERR_ARG, "pgv_lloyd_finish: NULL argument");
    PGV_TRY(check_common(dtype, dim));
    PGV_TRY(check_ops(ops));
    if (k < 1) PGV_FAIL(PGV_ERR_ARG, "k < 1");
    PGV_HIP(hipSetDevice(ctx->device));
    const RowGeom g = row_geom(dim, dtype);
    // sums arrive [k x dim] fp32; the kernel wants [k x ld]
    PGV_TRY(ctx->km_g.ensure(sizeof(float) * (size_t)k * g.ld + 64));
    float *sums_pad = ctx->km_g.as<float>();
    const bool sums_dev = is_device_ptr(sums);
    PGV_HIP(hipMemsetAsync(sums_pad, 0, sizeof(float) * (size_t)k * g.ld, ctx->stream));
    PGV_HIP(hipMemcpy2DAsync(sums_pad, sizeof(float) * (size_t)g.ld, sums, sizeof(float) * (size_t)dim,
                             sizeof(float) * (size_t)dim, (size_t)k,
                             sums_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    const void *counts_dev;
    std::vector<int32_t> h_counts((size_t)k);
    if (is_device_ptr(counts)) {
        counts_dev = counts;
        PGV_HIP(hipMemcpyAsync(h_counts.data(), counts, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
        PGV_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        memcpy(h_counts.data(), counts, sizeof(int32_t) * (size_t)k);
        PGV_TRY(stage_flat(ctx, counts, sizeof(int32_t) * (size_t)k, ctx->out_stage, &counts_dev));
    }
    PGV_TRY(ctx->centers_stage.ensure((size_t)k * g.ld * elem_size(dtype)));
    Rng r(rng);
    PGV_TRY(lloyd_finish_dev(ctx, ops, dtype, g, dim, k, sums_pad, static_cast<const int32_t *>(counts_dev),
                             h_counts.data(), r, ctx->centers_stage.p));
    PGV_TRY(unstage_rows(ctx, ctx->centers_stage.p, k, dim, dtype, g, out_centers));
    return pgv_ctx_sync(ctx);
}

int pgv_kmeans(pgv_ctx *ctx, pgv_ops ops, pgv_dtype dtype, int dim, const void *samples, int n, int k,
               int max_iterations, const pgv_rng *rng, void *out_centers, int32_t *out_closest,
               int *out_iters) {
    if (!ctx || !out_centers) PGV_FAIL(PGV_ERR_ARG, "pgv_kmeans: ctx/out_centers is NULL");
    PGV_TRY(check_common(dtype, dim));
    PGV_TRY(check_ops(ops));
    if (k < 1 || k > 32768) PGV_FAIL(PGV_ERR_ARG, "lists %d outside 1..32768", k);
    if (n < 0 || (n > 0 && !samples)) PGV_FAIL(PGV_ERR_ARG, "bad samples");
    // spherical opclasses need dim > 1 (src/ivfbuild.c:375-378)
    if (spherical(ops) && dim < 2) PGV_FAIL(PGV_ERR_DIMS, "dimensions must be greater than one for this opclass");
    if (max_iterations <= 0) max_iterations = 500;  // src/ivfkmeans.c:347
    PGV_HIP(hipSetDevice(ctx->device));
    const RowGeom g = row_geom(dim, dtype);
    const size_t row_bytes = (size_t)g.ld * elem_size(dtype);
    Rng r(rng);
    PGV_TRY(ctx->centers_stage.ensure((size_t)k * row_bytes));
    void *centers_dev = ctx->centers_stage.p;
    PGV_HIP(hipMemsetAsync(centers_dev, 0, (size_t)k * row_bytes, ctx->stream));
    int iters = 0;

    if (n == 0) {
        // RandomCenters (src/ivfkmeans.c:110-133): as if every cluster were empty
        std::vector<int32_t> zero((size_t)k, 0);
        PGV_TRY(ctx->km_g.ensure(sizeof(float) * (size_t)k * g.ld + sizeof(int32_t) * (size_t)k));
        float *sums = ctx->km_g.as<float>();
        int32_t *counts = reinterpret_cast<int32_t *>(sums + (size_t)k * g.ld);
        PGV_HIP(hipMemsetAsync(sums, 0, sizeof(float) * (size_t)k * g.ld + sizeof(int32_t) * (size_t)k, ctx->stream));
        PGV_TRY(lloyd_finish_dev(ctx, ops, dtype, g, dim, k, sums, counts, zero.data(), r, centers_dev));
    } else {
        const void *s_dev;
        PGV_TRY(stage_rows(ctx, samples, n, dim, dtype, g, ctx->rows_stage, &s_dev));
        PGV_TRY(kmeanspp_dev(ctx, kmeans_rows(ops, dtype, g, s_dev, n), k, r, centers_dev));

        // km_g: sums[k x ld] | counts[k] | changes | closest[n]
        PGV_TRY(ctx->km_g.ensure(sizeof(float) * (size_t)k * g.ld + sizeof(int32_t) * ((size_t)k + (size_t)n) + 64));
        float *sums = ctx->km_g.as<float>();
        int32_t *counts = reinterpret_cast<int32_t *>(sums + (size_t)k * g.ld);
        unsigned long long *changes = reinterpret_cast<unsigned long long *>(counts + k + (k & 1));
        int32_t *closest = reinterpret_cast<int32_t *>(changes + 1);
        PGV_HIP(hipMemsetAsync(closest, 0xff, sizeof(int32_t) * (size_t)n, ctx->stream));  // -1: everything "changes" first
        PGV_TRY(staging_acquire(ctx));
        PGV_TRY(ctx->h_a.ensure(sizeof(int32_t) * (size_t)k + 16));
        for (int it = 0; it < max_iterations; it++) {
            iters = it + 1;
            PGV_TRY(lloyd_partial_dev(ctx, ops, dtype, g, s_dev, n, centers_dev, k, closest, sums, counts, changes));
            // counts (which clusters are empty) and the change count steer the host
            int32_t *h_counts = ctx->h_a.as<int32_t>();
            unsigned long long *h_changes = reinterpret_cast<unsigned long long *>(h_counts + k + (k & 1));
            PGV_HIP(hipMemcpyAsync(h_counts, counts, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
            PGV_HIP(hipMemcpyAsync(h_changes, changes, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
            PGV_HIP(hipStreamSynchronize(ctx->stream));
            const unsigned long long nchanges = *h_changes;
            PGV_TRY(lloyd_finish_dev(ctx, ops, dtype, g, dim, k, sums, counts, h_counts, r, centers_dev));
            // stop when an iteration other than the first reassigns nothing (src/ivfkmeans.c:482-483)
            if (nchanges == 0 && it != 0) break;
        }
        if (out_closest) {
            const bool dev = is_device_ptr(out_closest);
            PGV_HIP(hipMemcpyAsync(out_closest, closest, sizeof(int32_t) * (size_t)n,
                                   dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    PGV_TRY(check_centers_dev(ctx, ops, dtype, g, dim, k, centers_dev));
    PGV_TRY(unstage_rows(ctx, centers_dev, k, dim, dtype, g, out_centers));
    if (out_iters) *out_iters = iters;
    return pgv_ctx_sync(ctx);
}

}  // extern "C"
