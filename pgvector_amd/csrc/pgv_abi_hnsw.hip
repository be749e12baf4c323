// pgv_abi_hnsw.hip -- extern "C" entry points of libpgv_hip (include/pgv_hip.h): the HNSW mirror, its graph, searches and the build's scoring.
// Split out of pgv_abi.hip in round 5 (one unit per area, so that an edit recompiles one of them).
#include "pgv_abi_common.h"

extern "C" {

// ======================================================================= HNSW

int pgv_hnsw_upload(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, int dim, const void *elements,
                    int64_t n, pgv_hnsw **out) {
    return pgv_hnsw_upload_payload(ctx, metric, dtype, dim, elements, n, nullptr, 0, out);
}

// where the per-element payload starts inside the elements' allocation
static size_t hnsw_payload_offset(int64_t n, size_t row_bytes) {
    return ((size_t)(n > 0 ? n : 1) * row_bytes + 255) & ~(size_t)255;
}

// a bit mirror (pgv_hnsw_upload_bits, pgv_hnsw_upload_jaccard): rows of whole bytes scored by popcounts; the build-side
// entries serve it only where it was uploaded for that (pgv_hnsw_upload_bits_buildable)
static bool hnsw_is_bits(const pgv_hnsw *h) { return h->nbits > 0; }

// ... and a sparse mirror (pgv_hnsw_upload_sparse): CSR rows scored by sparse_pair.h; searched and scored through the
// _sparse entries, and built on only where it was uploaded for that (pgv_hnsw_upload_sparse_buildable)
static bool hnsw_is_sparse(const pgv_hnsw *h) { return h->sparse; }

#define PGV_NO_BUILD(h, who)                                                                                      \
    do {                                                                                                         \
        if ((h) && hnsw_is_bits(h) && !(h)->buildable)                                                           \
            PGV_FAIL(PGV_ERR_ARG, "%s: a bit mirror (pgv_hnsw_upload_bits / _jaccard) is searched and scored, not built on", who); \
        if ((h) && hnsw_is_sparse(h) && !(h)->buildable)                                                         \
            PGV_FAIL(PGV_ERR_ARG, "%s: a sparse mirror (pgv_hnsw_upload_sparse) is searched and scored, not built on", who); \
    } while (0)

// the entries that take dense queries or rows, on a sparse mirror; the _sparse entries on any other mirror
#define PGV_NO_SPARSE(h, who, twin)                                                                              \
    do {                                                                                                         \
        if ((h) && hnsw_is_sparse(h))                                                                            \
            PGV_FAIL(PGV_ERR_ARG, "%s: a sparse mirror (pgv_hnsw_upload_sparse) takes sparse queries: use %s", who, twin); \
    } while (0)
#define PGV_ONLY_SPARSE(h, who)                                                                                  \
    do {                                                                                                         \
        if ((h) && !hnsw_is_sparse(h))                                                                           \
            PGV_FAIL(PGV_ERR_ARG, "%s: not a sparse mirror (pgv_hnsw_upload_sparse)", who);                      \
    } while (0)

// the geometry of a mirror's rows: dim elements of dtype, or nbits bits
static RowGeom hnsw_geom(int dim, pgv_dtype dtype, int nbits) { return nbits > 0 ? bit_row_geom(nbits) : row_geom(dim, dtype); }
// bytes of one row as the caller packs it, and as the mirror keeps it (whole 16-byte vectors)
static size_t hnsw_src_row_bytes(int dim, pgv_dtype dtype, int nbits) {
    return nbits > 0 ? (size_t)(nbits + 7) / 8 : (size_t)dim * elem_size(dtype);
}
static size_t hnsw_row_bytes(const RowGeom &g) { return (size_t)g.nvec * kVecBytes; }

// queries [nq x dim] of the mirror's element type -> device rows in the mirror's row layout
static int hnsw_stage_queries(pgv_hnsw *h, const void *queries, int nq, const void **q_dev) {
    return stage_rows(h->ctx, queries, nq, hnsw_src_row_bytes(h->dim, h->dtype, h->nbits), hnsw_row_bytes(h->geom),
                      h->ctx->q_stage, q_dev);
}

static int hnsw_upload_rows(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, int dim, int nbits, const void *elements,
                            int64_t n, const void *payload, int payload_bytes, pgv_hnsw **out);

int pgv_hnsw_upload_payload(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, int dim, const void *elements,
                            int64_t n, const void *payload, int payload_bytes, pgv_hnsw **out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_upload: ctx/out is NULL");
    *out = nullptr;
    PGV_TRY(check_common(dtype, dim));
    PGV_TRY(check_metric(metric));
    return hnsw_upload_rows(ctx, metric, dtype, dim, 0, elements, n, payload, payload_bytes, out);
}

// The element rows of an HNSW index over bit strings (`USING hnsw (... bit_hamming_ops)`, sql/vector.sql:901-905; type
// info hnsw_bit_support, src/hnswutils.c:1403-1416): what hnswgettuple's first batch (src/hnswscan.c:25-56) scores with
// hamming_distance (src/bitvec.c:45-56 over BitHammingDistanceDefault, src/bitutils.c:49-73) when it walks such an index.
int pgv_hnsw_upload_bits(pgv_ctx *ctx, pgv_bit_metric metric, int nbits, const void *elements, int64_t n,
                         const void *payload, int payload_bytes, pgv_hnsw **out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_upload_bits: ctx/out is NULL");
    *out = nullptr;
    if (metric == PGV_BIT_JACCARD)
        PGV_FAIL(PGV_ERR_ARG,
                 "pgv_hnsw_upload_bits: this entry uploads bit_hamming_ops mirrors, whose distances are the walk's fp32 keys; a "
                 "bit_jaccard_ops mirror ranks by an integer key of the jaccard ratio: use pgv_hnsw_upload_jaccard");
    if (metric != PGV_BIT_HAMMING) PGV_FAIL(PGV_ERR_ARG, "unknown bit metric %d", (int)metric);
    if (nbits < 1 || nbits > kHnswMaxBits)
        PGV_FAIL(PGV_ERR_DIMS, "bit dimensions %d outside 1..%d (HNSW_MAX_DIM * 32, src/hnswutils.c:1414)", nbits, kHnswMaxBits);
    return hnsw_upload_rows(ctx, bit_metric_slot(PGV_BIT_HAMMING), PGV_F32, nbits, nbits, elements, n, payload, payload_bytes, out);
}

// ... over bit strings under bit_jaccard_ops (sql/vector.sql:907-911, the same type info): the same rows, scored with
// jaccard_distance (src/bitvec.c:60-70 over BitJaccardDistanceDefault, src/bitutils.c:99-131).  The mirror's metric slot
// says so, and with it every view, every exported handle and every launch (RowsView::jaccard, dispatch_rows).
int pgv_hnsw_upload_jaccard(pgv_ctx *ctx, int nbits, const void *elements, int64_t n, const void *payload, int payload_bytes,
                            pgv_hnsw **out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_upload_jaccard: ctx/out is NULL");
    *out = nullptr;
    if (nbits < 1 || nbits > kHnswMaxBits)
        PGV_FAIL(PGV_ERR_DIMS, "bit dimensions %d outside 1..%d (HNSW_MAX_DIM * 32, src/hnswutils.c:1414)", nbits, kHnswMaxBits);
    return hnsw_upload_rows(ctx, bit_metric_slot(PGV_BIT_JACCARD), PGV_F32, nbits, nbits, elements, n, payload, payload_bytes, out);
}

// The same rows under either bit metric, uploaded to be BUILT on as well (`CREATE INDEX ... USING hnsw (... bit_hamming_ops /
// bit_jaccard_ops)`, HnswFindElementNeighbors and HnswUpdateNeighborsInMemory over bit elements): everything the two
// entries above give, and the build-side entries (pgv_hnsw_build_*, pgv_hnsw_link_*, pgv_hnsw_score_groups) serve the
// mirror and its views.  Their distances are floats, as HnswCandidate.distance is: Hamming counts, or the (float) of
// jaccard_distance's float8.
int pgv_hnsw_upload_bits_buildable(pgv_ctx *ctx, pgv_bit_metric metric, int nbits, const void *elements, int64_t n,
                                   const void *payload, int payload_bytes, pgv_hnsw **out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_upload_bits_buildable: ctx/out is NULL");
    *out = nullptr;
    if (metric != PGV_BIT_HAMMING && metric != PGV_BIT_JACCARD) PGV_FAIL(PGV_ERR_ARG, "unknown bit metric %d", (int)metric);
    if (nbits < 1 || nbits > kHnswMaxBits)
        PGV_FAIL(PGV_ERR_DIMS, "bit dimensions %d outside 1..%d (HNSW_MAX_DIM * 32, src/hnswutils.c:1414)", nbits, kHnswMaxBits);
    PGV_TRY(hnsw_upload_rows(ctx, bit_metric_slot(metric), PGV_F32, nbits, nbits, elements, n, payload, payload_bytes, out));
    (*out)->buildable = true;
    return PGV_OK;
}

int pgv_hnsw_buildable_bits(const pgv_hnsw *h) { return h && hnsw_is_bits(h) && h->buildable ? h->nbits : 0; }

static int hnsw_upload_rows(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, int dim, int nbits, const void *elements,
                            int64_t n, const void *payload, int payload_bytes, pgv_hnsw **out) {
    if (n < 0 || (n > 0 && !elements)) PGV_FAIL(PGV_ERR_ARG, "bad elements");
    if (payload_bytes < 0 || payload_bytes > 4096 || (payload_bytes & 3) || (payload_bytes > 0 && n > 0 && !payload))
        PGV_FAIL(PGV_ERR_ARG, "payload: 0..4096 bytes per element in whole words, got %d", payload_bytes);
    PGV_HIP(hipSetDevice(ctx->device));
    pgv_hnsw *h = new (std::nothrow) pgv_hnsw();
    if (!h) PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    h->ctx = ctx;
    h->metric = metric;
    h->dtype = dtype;
    h->dim = dim;
    h->nbits = nbits;
    h->n = n;
    h->geom = hnsw_geom(dim, dtype, nbits);
    const size_t row_bytes = hnsw_row_bytes(h->geom), src_bytes = hnsw_src_row_bytes(dim, dtype, nbits);
    const size_t bytes = (size_t)(n > 0 ? n : 1) * row_bytes;
    // the payload (what a scan needs to turn an element into heap TIDs) rides in the same allocation, so that the one
    // IPC handle of the elements carries it to importing processes
    const size_t pay_off = hnsw_payload_offset(n, row_bytes), pay_total = (size_t)payload_bytes * (size_t)(n > 0 ? n : 0);
    if (malloc_exportable(&h->elements, payload_bytes > 0 ? pay_off + (pay_total ? pay_total : 4) : bytes) != hipSuccess) {
        delete h;
        PGV_FAIL(PGV_ERR_NOMEM, "hipMalloc(%zu) for hnsw elements failed", bytes);
    }
    h->payload_bytes = payload_bytes;
    h->payload = payload_bytes > 0 ? static_cast<char *>(h->elements) + pay_off : nullptr;
    if (pay_total) {
        hipError_t e = hipMemcpyAsync(h->payload, payload, pay_total,
                                      is_device_ptr(payload) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            pgv_hnsw_free(h);
            PGV_FAIL(PGV_ERR_DEVICE, "hnsw payload upload failed: %s", hipGetErrorString(e));
        }
    }
    if (n > 0) {
        const bool dev = is_device_ptr(elements);
        hipError_t e;
        if (row_bytes == src_bytes) {
            e = hipMemcpyAsync(h->elements, elements, (size_t)n * row_bytes,
                               dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
        } else {
            e = hipMemsetAsync(h->elements, 0, bytes, ctx->stream);
            if (e == hipSuccess)
                e = hipMemcpy2DAsync(h->elements, row_bytes, elements, src_bytes, src_bytes,
                                     (size_t)n, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            pgv_hnsw_free(h);
            PGV_FAIL(PGV_ERR_DEVICE, "hnsw upload failed: %s", hipGetErrorString(e));
        }
    }
    *out = h;
    return PGV_OK;
}

// PGV_HNSW_PAIRS_GATHER=1: the build's pair distances by the older gathered kernel (one pair a lane group, both rows from
// L2) instead of score_groups_kernel's 4 x 4 tiles -- the same values bit for bit, for A/B runs
static bool hnsw_pairs_by_gather() {
    static int v = -1;
    if (v < 0) {
        const char *e = getenv("PGV_HNSW_PAIRS_GATHER");
        v = e && atoi(e) != 0 ? 1 : 0;
    }
    return v != 0;
}

// The gathered route's pair distances, pair i = (a[i], b[i]) of element slots.  Over sparse rows the pairs are oriented
// first -- the smaller slot is the row, the larger the query, sparse_groups_kernel's rule -- and scored as
// pgv_hnsw_score_pairs scores them, the mirror its own query array
static int hnsw_score_gathered(pgv_ctx *ctx, const RowsView &rows, int32_t *a, int32_t *b, int64_t npairs, float *out) {
    if (!rows.sparse()) return launch_score_gather(ctx, rows, rows.rows, a, b, npairs, out);
    PGV_TRY(launch_sparse_orient_pairs(ctx, a, b, npairs));
    return launch_sparse_pairs(ctx, rows, rows.ptr, rows.rows, a, b, npairs, out);
}

// Searches on this handle's stream see the mirror's last patch, whichever stream ran it (a device-side wait).
static int hnsw_graph_acquire(pgv_hnsw *h) {
    pgv_hnsw *o = h->view_of ? h->view_of : h;
    if (o->graph_ev_set) PGV_HIP(hipStreamWaitEvent(h->ctx->stream, o->graph_ev, 0));
    return PGV_OK;
}

// a view follows its owner: the graph may have been (re)set and the entry point moved since the view was made
static void hnsw_view_refresh(pgv_hnsw *h) {
    if (h->view_of) h->graph = h->view_of->graph;
}

// The arrays of a graph over n elements with g->nbr_total neighbor slots in its one allocation, levels | nbr_start |
// nbr, each rounded to 16 bytes: in g->mem where an importer has opened it, in a fresh exportable allocation otherwise.
// The process that sets a graph and the ones that import it both come here, so they agree on the layout
static int hnsw_graph_carve(HnswGraph *g, int64_t n) {
    const size_t lb = ((size_t)n * sizeof(int32_t) + 15) / 16 * 16;
    const size_t sb = ((size_t)(n + 1) * sizeof(int64_t) + 15) / 16 * 16;
    g->bytes = lb + sb + (size_t)(g->nbr_total > 0 ? g->nbr_total : 1) * sizeof(int32_t);
    if (!g->mem && malloc_exportable(&g->mem, g->bytes) != hipSuccess) {
        const size_t bytes = g->bytes;
        *g = HnswGraph();
        PGV_FAIL(PGV_ERR_NOMEM, "hipMalloc(%zu) for the hnsw graph failed", bytes);
    }
    char *base = static_cast<char *>(g->mem);
    g->levels = reinterpret_cast<const int32_t *>(base);
    g->nbr_start = reinterpret_cast<const int64_t *>(base + lb);
    g->nbr = reinterpret_cast<int32_t *>(base + lb + sb);
    return PGV_OK;
}

int pgv_hnsw_device(const pgv_hnsw *h) { return h && h->ctx ? h->ctx->device : -1; }

int pgv_hnsw_share(pgv_hnsw *h, pgv_ctx *ctx, pgv_hnsw **out) {
    if (!h || !ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_share: mirror/ctx/out is NULL");
    *out = nullptr;
    if (ctx->device != h->ctx->device) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_share: the mirror lives on another device");
    pgv_hnsw *v = new (std::nothrow) pgv_hnsw();
    if (!v) PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    static_cast<HnswElements &>(*v) = *h;
    v->ctx = ctx;
    v->view_of = h->view_of ? h->view_of : h;
    hnsw_view_refresh(v);
    *out = v;
    return PGV_OK;
}

static void hnsw_link_free(pgv_hnsw *o);

void pgv_hnsw_free(pgv_hnsw *h) {
    if (!h) return;
    if (h->ctx) (void)hipStreamSynchronize(h->ctx->stream);
    if (h->view_of) {  // the owner's allocations stay
        h->bitmaps.release();
        delete h;
        return;
    }
    hnsw_link_free(h);
    if (h->graph_ev) (void)hipEventDestroy(h->graph_ev);
    if (h->imported) {
        if (h->elements) (void)hipIpcCloseMemHandle(h->elements);
        if (h->graph.mem) (void)hipIpcCloseMemHandle(h->graph.mem);
    } else {
        if (h->elements) (void)hipFree(h->elements);
        if (h->graph.mem) (void)hipFree(h->graph.mem);
    }
    h->bitmaps.release();
    h->live.release();
    delete h;
}

struct HnswHandleWire {
    uint64_t magic;
    uint32_t abi, pid;
    int32_t device, metric, dtype, dim, m, entry;
    int64_t n, nbr_total;
    uint64_t graph_bytes;
    // nbits > 0: a bit mirror, and `metric` above is its pgv_bit_metric (0 Hamming -- what the word always held for a bit
    // mirror -- or 1 Jaccard: an importer walks with the exporter's keys); 0 otherwise, as the word always was
    int32_t payload_bytes, nbits;
    hipIpcMemHandle_t elements, graph;
};
static_assert(sizeof(HnswHandleWire) <= PGV_INDEX_HANDLE_BYTES, "pgv_index_handle too small for an HNSW mirror");
static constexpr uint64_t kHnswHandleMagic = 0x7067765f686e7731ull;  // "pgv_hnw1"

int pgv_hnsw_export(pgv_hnsw *h, pgv_index_handle *out) {
    if (!h || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_export: handle/out is NULL");
    if (hnsw_is_sparse(h))
        PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_export: a sparse mirror (pgv_hnsw_upload_sparse) is not exported: the handle carries one "
                              "allocation of fixed-width rows");
    if (h->imported || h->view_of) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_export: export from the process that uploaded the mirror");
    if (!h->elements || !h->graph.mem || h->graph.m == 0)
        PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_export: needs a non-empty mirror with its graph set (pgv_hnsw_set_graph)");
    PGV_HIP(hipSetDevice(h->ctx->device));
    PGV_HIP(hipStreamSynchronize(h->ctx->stream));
    HnswHandleWire w;
    memset(&w, 0, sizeof(w));
    w.magic = kHnswHandleMagic;
    w.abi = PGV_ABI_VERSION;
    w.pid = (uint32_t)getpid();
    w.device = h->ctx->device;
    w.metric = h->metric;
    w.dtype = h->dtype;
    w.dim = h->dim;
    w.m = h->graph.m;
    w.entry = h->graph.entry;
    w.n = h->n;
    w.nbr_total = h->graph.nbr_total;
    w.graph_bytes = h->graph.bytes;
    w.payload_bytes = h->payload_bytes;
    w.nbits = h->nbits;
    hipError_t e = hipIpcGetMemHandle(&w.elements, h->elements);
    if (e == hipSuccess) e = hipIpcGetMemHandle(&w.graph, h->graph.mem);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        PGV_FAIL(PGV_ERR_DEVICE, "hipIpcGetMemHandle failed: %s (HSA_ENABLE_IPC_MODE_LEGACY=0 must be set)", hipGetErrorString(e));
    }
    memset(out, 0, sizeof(*out));
    memcpy(out->bytes, &w, sizeof(w));
    return PGV_OK;
}

int pgv_hnsw_import(pgv_ctx *ctx, const pgv_index_handle *handle, pgv_hnsw **out) {
    if (!ctx || !handle || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_import: ctx/handle/out is NULL");
    *out = nullptr;
    HnswHandleWire w;
    memcpy(&w, handle->bytes, sizeof(w));
    if (w.magic != kHnswHandleMagic || w.abi != PGV_ABI_VERSION)
        PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_import: not an HNSW handle of this library version");
    if (w.pid == (uint32_t)getpid())
        PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_import: the handle was exported by this process");
    if (w.device != ctx->device)
        PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_import: the mirror lives on device %d, the context on %d", w.device, ctx->device);
    if (w.nbits != 0) {
        if (w.nbits < 1 || w.nbits > kHnswMaxBits || w.dim != w.nbits || (w.metric != PGV_BIT_HAMMING && w.metric != PGV_BIT_JACCARD))
            PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_import: corrupt handle");
    } else {
        PGV_TRY(check_common((pgv_dtype)w.dtype, w.dim));
        PGV_TRY(check_metric((pgv_metric)w.metric));
    }
    if (w.n < 1 || w.m < 2 || w.m > 100 || w.entry < -1 || w.entry >= w.n || w.nbr_total < 0 || w.payload_bytes < 0 ||
        w.payload_bytes > 4096)
        PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_import: corrupt handle");
    PGV_HIP(hipSetDevice(ctx->device));
    pgv_hnsw *h = new (std::nothrow) pgv_hnsw();
    if (!h) PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    h->ctx = ctx;
    h->metric = (pgv_metric)w.metric;
    h->dtype = (pgv_dtype)w.dtype;
    h->dim = w.dim;
    h->n = w.n;
    h->nbits = w.nbits;
    h->geom = hnsw_geom(w.dim, h->dtype, w.nbits);
    h->graph.m = w.m;
    h->graph.entry = w.entry;
    h->graph.nbr_total = w.nbr_total;
    h->imported = true;
    hipError_t e = hipIpcOpenMemHandle(&h->elements, w.elements, hipIpcMemLazyEnablePeerAccess);
    if (e == hipSuccess) e = hipIpcOpenMemHandle(&h->graph.mem, w.graph, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (h->elements && !h->graph.mem) { (void)hipIpcCloseMemHandle(h->elements); }
        delete h;
        PGV_FAIL(PGV_ERR_DEVICE, "hipIpcOpenMemHandle failed: %s", hipGetErrorString(e));
    }
    (void)hnsw_graph_carve(&h->graph, h->n);  // (in the opened allocation; its bytes are the exporter's w.graph_bytes)
    h->payload_bytes = w.payload_bytes;
    h->payload = w.payload_bytes > 0
                     ? static_cast<char *>(h->elements) + hnsw_payload_offset(h->n, hnsw_row_bytes(h->geom))
                     : nullptr;
    *out = h;
    return PGV_OK;
}

// the payload rows of the given element slots (a scan's results) -> host memory; slots < 0 give zero bytes
int pgv_hnsw_get_payload(pgv_hnsw *h, const int64_t *elements, int n, void *out) {
    if (!h || !out || (n > 0 && !elements)) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_get_payload: handle/elements/out is NULL");
    if (n < 0) PGV_FAIL(PGV_ERR_ARG, "n < 0");
    if (h->payload_bytes <= 0) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_get_payload: the mirror was uploaded without a payload");
    if (n == 0) return PGV_OK;
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    const void *e_dev;
    PGV_TRY(stage_flat(ctx, elements, sizeof(int64_t) * (size_t)n, ctx->idx_stage, &e_dev));
    OutArg oo;
    PGV_TRY(oo.init(out, (size_t)h->payload_bytes * (size_t)n, ctx->out_stage));
    PGV_TRY(launch_gather_words(ctx, h->payload, h->payload_bytes / 4, h->n, static_cast<const int64_t *>(e_dev), n,
                                oo.as<uint32_t>()));
    bool need = false;
    PGV_TRY(oo.finish(ctx, &need));
    return sync_if(ctx, need);
}

int pgv_hnsw_score(pgv_hnsw *h, const void *queries, int nq, const int32_t *slot, const int32_t *query_of,
                   int64_t npairs, float *out) {
    if (!h || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_score: handle/out is NULL");
    PGV_NO_SPARSE(h, "pgv_hnsw_score", "pgv_hnsw_score_sparse");
    if (npairs < 0 || nq < 1) PGV_FAIL(PGV_ERR_ARG, "bad sizes");
    if (npairs == 0) return PGV_OK;
    if (!queries || !slot) PGV_FAIL(PGV_ERR_ARG, "queries/slot is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    const void *q_dev, *s_dev, *qo_dev = nullptr;
    PGV_TRY(hnsw_stage_queries(h, queries, nq, &q_dev));
    PGV_TRY(stage_flat(ctx, slot, sizeof(int32_t) * (size_t)npairs, ctx->idx_stage, &s_dev));
    if (query_of) PGV_TRY(stage_flat(ctx, query_of, sizeof(int32_t) * (size_t)npairs, ctx->plan_d, &qo_dev));
    OutArg od;
    PGV_TRY(od.init(out, sizeof(float) * (size_t)npairs, ctx->out_stage));
    PGV_TRY(launch_score_gather(ctx, hnsw_rows(h), q_dev, static_cast<const int32_t *>(s_dev),
                                static_cast<const int32_t *>(qo_dev), npairs, od.as<float>()));
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    return sync_if(ctx, need);
}

int pgv_hnsw_set_graph(pgv_hnsw *h, int m, int32_t entry, const int32_t *levels, const int64_t *nbr_start,
                       const int32_t *nbr) {
    if (!h) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_set_graph: handle is NULL");
    if (h->imported || h->view_of) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_set_graph: an imported mirror / a view is read-only");
    if (m < 2 || m > 100) PGV_FAIL(PGV_ERR_ARG, "m must be 2..100 (src/hnsw.h:55-56), got %d", m);
    if (entry < -1 || entry >= h->n) PGV_FAIL(PGV_ERR_ARG, "entry point %d out of range", (int)entry);
    if (h->n > 0 && (!levels || !nbr_start || !nbr)) PGV_FAIL(PGV_ERR_ARG, "levels/nbr_start/nbr is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_HIP(hipStreamSynchronize(ctx->stream));  // no search may still be reading the old graph
    HnswGraph &g = h->graph;
    if (g.mem) PGV_HIP(hipFree(g.mem));
    g = HnswGraph();
    g.m = m;
    g.entry = entry;
    if (h->n == 0) return PGV_OK;
    // total neighbor slots: the last offset (it may live on either side)
    int64_t total = 0;
    PGV_HIP(hipMemcpy(&total, nbr_start + h->n, sizeof(int64_t), hipMemcpyDefault));
    if (total < 0) PGV_FAIL(PGV_ERR_ARG, "nbr_start is not an offset array");
    g.nbr_total = total;
    PGV_TRY(hnsw_graph_carve(&g, h->n));
    // (the one place that writes levels and nbr_start)
    PGV_HIP(hipMemcpyAsync(const_cast<int32_t *>(g.levels), levels, (size_t)h->n * sizeof(int32_t), hipMemcpyDefault, ctx->stream));
    PGV_HIP(hipMemcpyAsync(const_cast<int64_t *>(g.nbr_start), nbr_start, (size_t)(h->n + 1) * sizeof(int64_t), hipMemcpyDefault,
                           ctx->stream));
    if (total > 0) PGV_HIP(hipMemcpyAsync(g.nbr, nbr, (size_t)total * sizeof(int32_t), hipMemcpyDefault, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    return PGV_OK;
}

// one launch of the walk over the mirror as it stands, on its context's stream: the workgroups, their visited sets, the
// query counter
static int hnsw_run_search(pgv_hnsw *h, const HnswSearchArgs &a) {
    pgv_ctx *ctx = h->ctx;
    int words = 0;
    const int grid = hnsw_search_grid(ctx, a.nq, h->n, &words);
    PGV_TRY(h->bitmaps.ensure((size_t)grid * words * sizeof(uint32_t)));
    PGV_TRY(ctx->counters.ensure(256));
    return launch_hnsw_search(ctx, hnsw_rows(h), h->graph, a, h->bitmaps.as<uint32_t>(), words, grid, ctx->counters.as<int>());
}

// the searches of a batch of the build into lw_* (device arrays [nq x layer_cap x ef] / [nq x layer_cap]), on ctx's stream
static int hnsw_search_into(pgv_hnsw *h, const int32_t *e_dev, const int32_t *l_dev, int nq, int ef_construction, int layer_cap,
                            int32_t *lw_ids, float *lw_dist, int32_t *lw_cnt) {
    HnswSearchArgs a;
    a.qids = e_dev;
    a.qlevels = l_dev;
    a.nq = nq;
    a.ef = ef_construction;
    a.k = 0;
    a.lw_ids = lw_ids;
    a.lw_dist = lw_dist;
    a.lw_cnt = lw_cnt;
    a.lcap = layer_cap;
    if (hnsw_is_sparse(h)) a.max_q_nnz = h->sparse_max_nnz;  // (a query is an element: the LDS query region holds the longest)
    return hnsw_run_search(h, a);
}

int pgv_hnsw_search(pgv_hnsw *h, const void *queries, int nq, int ef_search, int k, int64_t *out_elem,
                    float *out_dist, int64_t *out_scored) {
    if (!h || !out_elem || !out_dist) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_search: handle/out is NULL");
    PGV_NO_SPARSE(h, "pgv_hnsw_search", "pgv_hnsw_search_sparse");
    hnsw_view_refresh(h);
    if (nq < 0) PGV_FAIL(PGV_ERR_ARG, "bad query count");
    if (ef_search < 1 || ef_search > 1000)
        PGV_FAIL(PGV_ERR_ARG, "hnsw.ef_search must be 1..1000 (src/hnsw.c:93-94), got %d", ef_search);
    if (k < 1 || k > ef_search) PGV_FAIL(PGV_ERR_ARG, "k must be 1..ef_search, got %d", k);
    if (h->graph.m == 0) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_search needs pgv_hnsw_set_graph first");
    if (nq == 0) return PGV_OK;
    if (!queries) PGV_FAIL(PGV_ERR_ARG, "queries is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_TRY(hnsw_graph_acquire(h));
    const void *q_dev;
    PGV_TRY(hnsw_stage_queries(h, queries, nq, &q_dev));
    OutArg oe, od, os;
    PGV_TRY(oe.init(out_elem, sizeof(int64_t) * (size_t)nq * k, ctx->out_stage2));
    PGV_TRY(od.init(out_dist, sizeof(float) * (size_t)nq * k, ctx->out_stage));
    PGV_TRY(os.init(out_scored, sizeof(int64_t) * (size_t)nq, ctx->sel_b));
    HnswSearchArgs a;
    a.queries = q_dev;
    a.nq = nq;
    a.ef = ef_search;
    a.k = k;
    a.out_elem = oe.as<int64_t>();
    a.out_dist = od.as<float>();
    a.out_scored = out_scored ? os.as<int64_t>() : nullptr;
    PGV_TRY(hnsw_run_search(h, a));
    bool need = false;
    PGV_TRY(oe.finish(ctx, &need));
    PGV_TRY(od.finish(ctx, &need));
    PGV_TRY(os.finish(ctx, &need));
    return sync_if(ctx, need);
}

// ------------------------------------------------------------------ HNSW over sparsevec elements
constexpr int kHnswMaxNnz = 1000;  // HNSW_MAX_NNZ (src/hnsw.h:34)

// The element rows of an HNSW index over sparsevec (`USING hnsw (... sparsevec_l2_ops / _ip_ops / _cosine_ops / _l1_ops)`,
// sql/vector.sql:1189-1212; type info hnsw_sparsevec_support, src/hnswutils.c:1361-1433).  One allocation: the rows'
// (index, value) pairs, row after row, plus one slack pair (a lane past an empty last row reads it) | ptr [n + 1] | payload
static int hnsw_upload_sparse_rows(const char *who, pgv_ctx *ctx, pgv_metric metric, int dim, const int64_t *row_ptr,
                                   const int32_t *row_idx, const float *row_val, int64_t n, const void *payload,
                                   int payload_bytes, pgv_hnsw **out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "%s: ctx/out is NULL", who);
    *out = nullptr;
    PGV_TRY(check_metric(metric));
    PGV_TRY(check_sparse_dim(who, dim));
    if (n < 0 || n > 0x7fffffff || (n > 0 && !row_ptr)) PGV_FAIL(PGV_ERR_ARG, "%s: bad n / row_ptr is NULL", who);
    if (payload_bytes < 0 || payload_bytes > 4096 || (payload_bytes & 3) || (payload_bytes > 0 && n > 0 && !payload))
        PGV_FAIL(PGV_ERR_ARG, "payload: 0..4096 bytes per element in whole words, got %d", payload_bytes);
    PGV_HIP(hipSetDevice(ctx->device));
    const int64_t none[1] = {0};
    StagedCsr r;
    // (the host copy of a device row_ptr is checked like a host one: the walk's register rows are sized from it)
    PGV_TRY(stage_csr(ctx, who, "elements", dim, n > 0 ? row_ptr : none, row_idx, row_val, n, true, ctx->plan_b, ctx->rows_stage,
                      ctx->idx_stage, &r));
    int max_nnz = 0;
    for (int64_t v = 0; v < n; v++) {
        if (r.host_ptr[v + 1] - r.host_ptr[v] > kHnswMaxNnz)
            PGV_FAIL(PGV_ERR_DIMS, "%s: element %lld has %lld stored elements: sparsevec cannot have more than %d "
                                   "non-zero elements for hnsw index (src/hnswutils.c:1371)",
                     who, (long long)v, (long long)(r.host_ptr[v + 1] - r.host_ptr[v]), kHnswMaxNnz);
        max_nnz = std::max(max_nnz, (int)(r.host_ptr[v + 1] - r.host_ptr[v]));
    }
    const int64_t total = r.host_ptr[n];
    pgv_hnsw *h = new (std::nothrow) pgv_hnsw();
    if (!h) PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    h->ctx = ctx;
    h->metric = metric;
    h->dtype = PGV_F32;
    h->dim = dim;
    h->sparse = true;
    h->sparse_max_nnz = max_nnz;
    h->n = n;
    const size_t elem_bytes = (((size_t)total + 1) * 8 + 255) & ~(size_t)255;
    const size_t ptr_bytes = (((size_t)n + 1) * sizeof(int64_t) + 255) & ~(size_t)255;
    const size_t pay_total = (size_t)payload_bytes * (size_t)n;
    const size_t bytes = elem_bytes + ptr_bytes + (pay_total ? pay_total : 4);
    if (malloc_exportable(&h->elements, bytes) != hipSuccess) {
        delete h;
        PGV_FAIL(PGV_ERR_NOMEM, "hipMalloc(%zu) for sparse hnsw elements failed", bytes);
    }
    char *base = static_cast<char *>(h->elements);
    h->sparse_ptr = reinterpret_cast<const int64_t *>(base + elem_bytes);
    h->payload_bytes = payload_bytes;
    h->payload = payload_bytes > 0 ? base + elem_bytes + ptr_bytes : nullptr;
    hipError_t e = hipMemsetAsync(base + (size_t)total * 8, 0, 8, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(base + elem_bytes, r.dev.ptr, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess && pay_total)
        e = hipMemcpyAsync(h->payload, payload, pay_total, is_device_ptr(payload) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                           ctx->stream);
    int rc = PGV_OK;
    if (e == hipSuccess) rc = launch_sparse_pack(ctx, r.dev.idx, r.dev.val, total, h->elements);
    if (e == hipSuccess && rc == PGV_OK) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess || rc != PGV_OK) {
        pgv_hnsw_free(h);
        if (rc != PGV_OK) return rc;
        PGV_FAIL(PGV_ERR_DEVICE, "sparse hnsw upload failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return PGV_OK;
}

int pgv_hnsw_upload_sparse(pgv_ctx *ctx, pgv_metric metric, int dim, const int64_t *row_ptr, const int32_t *row_idx,
                           const float *row_val, int64_t n, const void *payload, int payload_bytes, pgv_hnsw **out) {
    return hnsw_upload_sparse_rows("pgv_hnsw_upload_sparse", ctx, metric, dim, row_ptr, row_idx, row_val, n, payload, payload_bytes,
                                   out);
}

// The same rows uploaded to be BUILT on as well (`CREATE INDEX ... USING hnsw (... sparsevec_*_ops)`): everything the entry
// above gives, and the build-side entries (pgv_hnsw_build_*, pgv_hnsw_link_*, pgv_hnsw_score_groups) serve the mirror and
// its views.  The build-side value of the pair {a, b} of element slots is score_element(row = the smaller slot, query =
// the larger one) -- pgv_hnsw_score_pairs(min, max) -- wherever it is computed: score_element's last bit
// depends on which side is the query, and the build compares values of one pair that reach it by different routes.
int pgv_hnsw_upload_sparse_buildable(pgv_ctx *ctx, pgv_metric metric, int dim, const int64_t *row_ptr, const int32_t *row_idx,
                                     const float *row_val, int64_t n, const void *payload, int payload_bytes, pgv_hnsw **out) {
    PGV_TRY(hnsw_upload_sparse_rows("pgv_hnsw_upload_sparse_buildable", ctx, metric, dim, row_ptr, row_idx, row_val, n, payload,
                                    payload_bytes, out));
    (*out)->buildable = true;
    return PGV_OK;
}

int pgv_hnsw_buildable_sparse(const pgv_hnsw *h) { return h && hnsw_is_sparse(h) && h->buildable ? h->dim : 0; }

int64_t pgv_hnsw_elements(const pgv_hnsw *h) { return h ? h->n : -1; }

// queries in CSR -> the device, validated like pgv_sparse_topk's; *max_nnz: the longest one's stored elements
static int hnsw_stage_sparse_queries(pgv_hnsw *h, const char *who, const int64_t *q_ptr, const int32_t *q_idx, const float *q_val,
                                     int nq, StagedCsr *q, int *max_nnz) {
    pgv_ctx *ctx = h->ctx;
    PGV_TRY(stage_csr(ctx, who, "queries", h->dim, q_ptr, q_idx, q_val, nq, true, ctx->plan_c, ctx->q_stage, ctx->centers_stage, q));
    *max_nnz = 0;
    for (int i = 0; i < nq; i++) *max_nnz = std::max(*max_nnz, (int)(q->host_ptr[i + 1] - q->host_ptr[i]));
    return PGV_OK;
}

// HnswGetDistance over sparse elements for the caller's (element, query) pairs: pgv_hnsw_score with sparse queries
int pgv_hnsw_score_sparse(pgv_hnsw *h, const int64_t *q_ptr, const int32_t *q_idx, const float *q_val, int nq,
                          const int32_t *slot, const int32_t *query_of, int64_t npairs, float *out) {
    const char *who = "pgv_hnsw_score_sparse";
    if (!h || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_score_sparse: handle/out is NULL");
    PGV_ONLY_SPARSE(h, who);
    if (npairs < 0 || nq < 1) PGV_FAIL(PGV_ERR_ARG, "bad sizes");
    if (npairs == 0) return PGV_OK;
    if (!q_ptr || !slot) PGV_FAIL(PGV_ERR_ARG, "q_ptr/slot is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    StagedCsr q;
    int max_nnz = 0;
    PGV_TRY(hnsw_stage_sparse_queries(h, who, q_ptr, q_idx, q_val, nq, &q, &max_nnz));
    // the queries' pairs side by side, as the elements are kept
    const int64_t qtotal = q.host_ptr[nq];
    PGV_TRY(ctx->dist_mat.ensure((size_t)(qtotal > 0 ? qtotal : 1) * 8));
    PGV_TRY(launch_sparse_pack(ctx, q.dev.idx, q.dev.val, qtotal, ctx->dist_mat.p));
    const void *s_dev, *qo_dev = nullptr;
    PGV_TRY(stage_flat(ctx, slot, sizeof(int32_t) * (size_t)npairs, ctx->idx_stage, &s_dev));
    if (query_of) PGV_TRY(stage_flat(ctx, query_of, sizeof(int32_t) * (size_t)npairs, ctx->plan_d, &qo_dev));
    OutArg od;
    PGV_TRY(od.init(out, sizeof(float) * (size_t)npairs, ctx->out_stage));
    PGV_TRY(launch_sparse_pairs(ctx, hnsw_rows(h), q.dev.ptr, ctx->dist_mat.p, static_cast<const int32_t *>(s_dev),
                                static_cast<const int32_t *>(qo_dev), npairs, od.as<float>()));
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    return sync_if(ctx, need);
}

// pgv_hnsw_search over a sparse mirror: hnswgettuple's first batch (src/hnswscan.c:25-56) with sparsevec queries
int pgv_hnsw_search_sparse(pgv_hnsw *h, const int64_t *q_ptr, const int32_t *q_idx, const float *q_val, int nq, int ef_search,
                           int k, int64_t *out_elem, float *out_dist, int64_t *out_scored) {
    const char *who = "pgv_hnsw_search_sparse";
    if (!h || !out_elem || !out_dist) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_search_sparse: handle/out is NULL");
    PGV_ONLY_SPARSE(h, who);
    hnsw_view_refresh(h);
    if (nq < 0) PGV_FAIL(PGV_ERR_ARG, "bad query count");
    if (ef_search < 1 || ef_search > 1000)
        PGV_FAIL(PGV_ERR_ARG, "hnsw.ef_search must be 1..1000 (src/hnsw.c:93-94), got %d", ef_search);
    if (k < 1 || k > ef_search) PGV_FAIL(PGV_ERR_ARG, "k must be 1..ef_search, got %d", k);
    if (h->graph.m == 0) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_search_sparse needs pgv_hnsw_set_graph first");
    if (nq == 0) return PGV_OK;
    if (!q_ptr) PGV_FAIL(PGV_ERR_ARG, "q_ptr is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_TRY(hnsw_graph_acquire(h));
    StagedCsr q;
    HnswSearchArgs a;
    PGV_TRY(hnsw_stage_sparse_queries(h, who, q_ptr, q_idx, q_val, nq, &q, &a.max_q_nnz));
    OutArg oe, od, os;
    PGV_TRY(oe.init(out_elem, sizeof(int64_t) * (size_t)nq * k, ctx->out_stage2));
    PGV_TRY(od.init(out_dist, sizeof(float) * (size_t)nq * k, ctx->out_stage));
    PGV_TRY(os.init(out_scored, sizeof(int64_t) * (size_t)nq, ctx->sel_b));
    a.sparse_queries = q.dev;
    a.nq = nq;
    a.ef = ef_search;
    a.k = k;
    a.out_elem = oe.as<int64_t>();
    a.out_dist = od.as<float>();
    a.out_scored = out_scored ? os.as<int64_t>() : nullptr;
    PGV_TRY(hnsw_run_search(h, a));
    bool need = false;
    PGV_TRY(oe.finish(ctx, &need));
    PGV_TRY(od.finish(ctx, &need));
    PGV_TRY(os.finish(ctx, &need));
    return sync_if(ctx, need);
}

int pgv_hnsw_build_search(pgv_hnsw *h, const int32_t *elements, const int32_t *insert_levels, int nq,
                          int ef_construction, int layer_cap, int32_t *out_ids, float *out_dist, int32_t *out_count) {
    if (!h || !out_ids || !out_dist || !out_count) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_build_search: handle/out is NULL");
    PGV_NO_BUILD(h, "pgv_hnsw_build_search");
    hnsw_view_refresh(h);
    if (nq < 0 || layer_cap < 1) PGV_FAIL(PGV_ERR_ARG, "bad sizes");
    if (ef_construction < 4 || ef_construction > 1000)
        PGV_FAIL(PGV_ERR_ARG, "ef_construction must be 4..1000 (src/hnsw.h:58-59), got %d", ef_construction);
    if (h->graph.m == 0) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_build_search needs pgv_hnsw_set_graph first");
    if (nq == 0) return PGV_OK;
    if (!elements || !insert_levels) PGV_FAIL(PGV_ERR_ARG, "elements/insert_levels is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_TRY(hnsw_graph_acquire(h));
    const void *e_dev, *l_dev;
    PGV_TRY(stage_flat(ctx, elements, sizeof(int32_t) * (size_t)nq, ctx->idx_stage, &e_dev));
    PGV_TRY(stage_flat(ctx, insert_levels, sizeof(int32_t) * (size_t)nq, ctx->plan_d, &l_dev));
    const size_t per = (size_t)nq * layer_cap;
    OutArg oi, od, oc;
    PGV_TRY(oi.init(out_ids, sizeof(int32_t) * per * ef_construction, ctx->out_stage2));
    PGV_TRY(od.init(out_dist, sizeof(float) * per * ef_construction, ctx->out_stage));
    PGV_TRY(oc.init(out_count, sizeof(int32_t) * per, ctx->sel_b));
    PGV_TRY(hnsw_search_into(h, static_cast<const int32_t *>(e_dev), static_cast<const int32_t *>(l_dev), nq, ef_construction,
                             layer_cap, oi.as<int32_t>(), od.as<float>(), oc.as<int32_t>()));
    bool need = false;
    PGV_TRY(oi.finish(ctx, &need));
    PGV_TRY(od.finish(ctx, &need));
    PGV_TRY(oc.finish(ctx, &need));
    return sync_if(ctx, need);
}

// SelectNeighbors over the candidate lists lw_* of a batch (device arrays), on ctx's stream; outputs as pgv_hnsw_build_neighbors
static int hnsw_select_from(pgv_hnsw *h, const int32_t *lw_ids, const float *lw_dist, const int32_t *lw_cnt, const int32_t *l_dev,
                            int nq, int ef_construction, int layer_cap, int32_t *out_ids, float *out_dist, uint8_t *out_closer,
                            int32_t *out_count, int64_t *out_pairs) {
    pgv_ctx *ctx = h->ctx;
    const int m = h->graph.m, stride = 2 * m;
    const size_t per = (size_t)nq * layer_cap;
    const int ngroups = (int)per;
    const RowsView rows = hnsw_rows(h);
    PGV_TRY(ctx->km_e.ensure(sizeof(int64_t) * (per + 1)));
    int64_t *pair_start = ctx->km_e.as<int64_t>();
    // which lists SelectNeighbors has to thin, and where each one's pair triangle goes; the total comes back (8 bytes:
    // it sizes the next launches)
    PGV_TRY(launch_hnsw_select_plan(ctx, lw_cnt, ngroups, layer_cap, m, pair_start));
    int64_t npairs = 0;
    PGV_HIP(hipMemcpyAsync(&npairs, pair_start + ngroups, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    if (npairs < 0 || npairs > (int64_t)per * ef_construction * (ef_construction - 1) / 2)
        PGV_FAIL(PGV_ERR_STATE, "hnsw select: %lld pairs planned", (long long)npairs);
    if (npairs > 0) {
        PGV_TRY(ctx->dist_mat.ensure(sizeof(float) * (size_t)npairs));
        // CheckElementCloser's HnswGetDistance (src/hnswutils.c:1040-1059), a list's triangle in 4 x 4 tiles
        if (hnsw_pairs_by_gather()) {
            PGV_TRY(ctx->km_f.ensure(sizeof(int32_t) * (size_t)npairs));
            PGV_TRY(ctx->km_g.ensure(sizeof(int32_t) * (size_t)npairs));
            PGV_TRY(launch_expand_groups(ctx, lw_ids, nullptr, ef_construction, lw_cnt, nullptr, pair_start, ngroups,
                                         ctx->km_f.as<int32_t>(), ctx->km_g.as<int32_t>()));
            PGV_TRY(hnsw_score_gathered(ctx, rows, ctx->km_f.as<int32_t>(), ctx->km_g.as<int32_t>(), npairs,
                                        ctx->dist_mat.as<float>()));
        } else
            PGV_TRY(launch_score_groups(ctx, rows, lw_ids, nullptr, ef_construction, lw_cnt, nullptr, pair_start, ngroups,
                                        ctx->dist_mat.as<float>()));
    } else
        PGV_TRY(ctx->dist_mat.ensure(16));
    OutArg oi, od, oc, on;
    PGV_TRY(oi.init(out_ids, sizeof(int32_t) * per * stride, ctx->out_stage));
    PGV_TRY(od.init(out_dist, sizeof(float) * per * stride, ctx->out_stage2));
    PGV_TRY(oc.init(out_closer, per * stride, ctx->sel_a));
    PGV_TRY(on.init(out_count, sizeof(int32_t) * per, ctx->sel_b));
    PGV_TRY(launch_hnsw_select(ctx, lw_ids, lw_dist, lw_cnt, l_dev, pair_start, ctx->dist_mat.as<float>(), ngroups, layer_cap,
                               ef_construction, m, stride, oi.as<int32_t>(), od.as<float>(), oc.as<uint8_t>(), on.as<int32_t>()));
    if (out_pairs) *out_pairs = npairs;
    bool need = false;
    PGV_TRY(oi.finish(ctx, &need));
    PGV_TRY(od.finish(ctx, &need));
    PGV_TRY(oc.finish(ctx, &need));
    PGV_TRY(on.finish(ctx, &need));
    return sync_if(ctx, need);
}

static int hnsw_build_args(pgv_hnsw *h, const char *who, int nq, int ef_construction, int layer_cap) {
    if (nq < 0 || layer_cap < 1) PGV_FAIL(PGV_ERR_ARG, "%s: bad sizes", who);
    if (ef_construction < 4 || ef_construction > 1000)
        PGV_FAIL(PGV_ERR_ARG, "ef_construction must be 4..1000 (src/hnsw.h:58-59), got %d", ef_construction);
    if (h->graph.m == 0) PGV_FAIL(PGV_ERR_ARG, "%s needs pgv_hnsw_set_graph first", who);
    const int stride = 2 * h->graph.m;
    if ((size_t)nq * layer_cap > 0x7fffffff / (size_t)(ef_construction > stride ? ef_construction : stride))
        PGV_FAIL(PGV_ERR_ARG, "%s: batch too large", who);
    return PGV_OK;
}

int pgv_hnsw_build_neighbors(pgv_hnsw *h, const int32_t *elements, const int32_t *insert_levels, int nq,
                             int ef_construction, int layer_cap, int32_t *out_ids, float *out_dist, uint8_t *out_closer,
                             int32_t *out_count, int64_t *out_pairs) {
    if (!h || !out_ids || !out_dist || !out_closer || !out_count)
        PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_build_neighbors: handle/out is NULL");
    PGV_NO_BUILD(h, "pgv_hnsw_build_neighbors");
    hnsw_view_refresh(h);
    PGV_TRY(hnsw_build_args(h, "pgv_hnsw_build_neighbors", nq, ef_construction, layer_cap));
    if (out_pairs) *out_pairs = 0;
    if (nq == 0) return PGV_OK;
    if (!elements || !insert_levels) PGV_FAIL(PGV_ERR_ARG, "elements/insert_levels is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_TRY(hnsw_graph_acquire(h));
    const size_t per = (size_t)nq * layer_cap;
    const void *e_dev, *l_dev;
    PGV_TRY(stage_flat(ctx, elements, sizeof(int32_t) * (size_t)nq, ctx->idx_stage, &e_dev));
    PGV_TRY(stage_flat(ctx, insert_levels, sizeof(int32_t) * (size_t)nq, ctx->plan_c, &l_dev));
    // the candidate lists stay on the device: km_b ids | km_c distances | km_d counts
    PGV_TRY(ctx->km_b.ensure(sizeof(int32_t) * per * ef_construction));
    PGV_TRY(ctx->km_c.ensure(sizeof(float) * per * ef_construction));
    PGV_TRY(ctx->km_d.ensure(sizeof(int32_t) * per));
    PGV_TRY(hnsw_search_into(h, static_cast<const int32_t *>(e_dev), static_cast<const int32_t *>(l_dev), nq, ef_construction,
                             layer_cap, ctx->km_b.as<int32_t>(), ctx->km_c.as<float>(), ctx->km_d.as<int32_t>()));
    return hnsw_select_from(h, ctx->km_b.as<int32_t>(), ctx->km_c.as<float>(), ctx->km_d.as<int32_t>(),
                            static_cast<const int32_t *>(l_dev), nq, ef_construction, layer_cap, out_ids, out_dist, out_closer,
                            out_count, out_pairs);
}

// pgv_hnsw_build_neighbors in two halves, for a caller that overlaps them: the searches of a batch, whose candidate
// lists are KEPT on the device in one of two slots of the mirror's build state (pgv_hnsw_link_begin), and the selection
// over a kept slot -- from any view of the mirror, on that view's stream.  The searches of batch n + 2 (other slot, one
// view) then run beside the selection of batch n + 1 (another view).
int pgv_hnsw_build_search_keep(pgv_hnsw *h, const int32_t *elements, const int32_t *insert_levels, int nq, int ef_construction,
                               int layer_cap, int slot) {
    if (!h) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_build_search_keep: handle is NULL");
    PGV_NO_BUILD(h, "pgv_hnsw_build_search_keep");
    hnsw_view_refresh(h);
    pgv_hnsw *o = h->view_of ? h->view_of : h;
    if (!o->link) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_build_search_keep needs pgv_hnsw_link_begin");
    if (slot < 0 || slot > 1) PGV_FAIL(PGV_ERR_ARG, "slot must be 0 or 1");
    PGV_TRY(hnsw_build_args(h, "pgv_hnsw_build_search_keep", nq, ef_construction, layer_cap));
    HnswLinkState::Kept &K = o->link->kept[slot];
    K.nq = 0;
    if (nq == 0) return PGV_OK;
    if (!elements || !insert_levels) PGV_FAIL(PGV_ERR_ARG, "elements/insert_levels is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_TRY(hnsw_graph_acquire(h));
    const size_t per = (size_t)nq * layer_cap;
    PGV_TRY(K.ids.ensure(sizeof(int32_t) * per * ef_construction));
    PGV_TRY(K.dist.ensure(sizeof(float) * per * ef_construction));
    PGV_TRY(K.cnt.ensure(sizeof(int32_t) * per));
    PGV_TRY(K.elems.ensure(sizeof(int32_t) * 2 * (size_t)nq));
    int32_t *e_dev = K.elems.as<int32_t>(), *l_dev = e_dev + nq;
    PGV_HIP(hipMemcpyAsync(e_dev, elements, sizeof(int32_t) * (size_t)nq, hipMemcpyDefault, ctx->stream));
    PGV_HIP(hipMemcpyAsync(l_dev, insert_levels, sizeof(int32_t) * (size_t)nq, hipMemcpyDefault, ctx->stream));
    PGV_TRY(hnsw_search_into(h, e_dev, l_dev, nq, ef_construction, layer_cap, K.ids.as<int32_t>(), K.dist.as<float>(),
                             K.cnt.as<int32_t>()));
    PGV_HIP(hipStreamSynchronize(ctx->stream));  // the searches are over when this returns: the tuples may be rewritten
    K.nq = nq;
    K.ef = ef_construction;
    K.lcap = layer_cap;
    return PGV_OK;
}

int pgv_hnsw_build_select_kept(pgv_hnsw *h, int slot, int32_t *out_ids, float *out_dist, uint8_t *out_closer, int32_t *out_count,
                               int64_t *out_pairs) {
    if (!h || !out_ids || !out_dist || !out_closer || !out_count)
        PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_build_select_kept: handle/out is NULL");
    PGV_NO_BUILD(h, "pgv_hnsw_build_select_kept");
    // (no view refresh: the entry point may be moving under pgv_hnsw_link_apply on another thread, and nothing here looks
    // at the graph -- the kept lists, the element rows and m, which is fixed for the build)
    pgv_hnsw *o = h->view_of ? h->view_of : h;
    if (!o->link) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_build_select_kept needs pgv_hnsw_link_begin");
    if (slot < 0 || slot > 1) PGV_FAIL(PGV_ERR_ARG, "slot must be 0 or 1");
    if (out_pairs) *out_pairs = 0;
    const HnswLinkState::Kept &K = o->link->kept[slot];
    if (K.nq == 0) return PGV_OK;
    PGV_HIP(hipSetDevice(h->ctx->device));
    h->graph.m = o->graph.m;
    const int32_t *l_dev = K.elems.as<int32_t>() + K.nq;
    return hnsw_select_from(h, K.ids.as<int32_t>(), K.dist.as<float>(), K.cnt.as<int32_t>(), l_dev, K.nq, K.ef, K.lcap, out_ids,
                            out_dist, out_closer, out_count, out_pairs);
}

int pgv_hnsw_score_pairs(pgv_hnsw *h, const int32_t *a, const int32_t *b, int64_t npairs, float *out) {
    if (!h || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_score_pairs: handle/out is NULL");
    if (npairs < 0) PGV_FAIL(PGV_ERR_ARG, "bad sizes");
    if (npairs == 0) return PGV_OK;
    if (!a || !b) PGV_FAIL(PGV_ERR_ARG, "a/b is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    const void *a_dev, *b_dev;
    PGV_TRY(stage_flat(ctx, a, sizeof(int32_t) * (size_t)npairs, ctx->idx_stage, &a_dev));
    PGV_TRY(stage_flat(ctx, b, sizeof(int32_t) * (size_t)npairs, ctx->plan_d, &b_dev));
    OutArg od;
    PGV_TRY(od.init(out, sizeof(float) * (size_t)npairs, ctx->out_stage));
    // the element mirror is its own query array: pair i = (row a[i], "query" b[i])
    if (hnsw_is_sparse(h))
        PGV_TRY(launch_sparse_pairs(ctx, hnsw_rows(h), h->sparse_ptr, h->elements, static_cast<const int32_t *>(a_dev),
                                    static_cast<const int32_t *>(b_dev), npairs, od.as<float>()));
    else
        PGV_TRY(launch_score_gather(ctx, hnsw_rows(h), h->elements, static_cast<const int32_t *>(a_dev),
                                    static_cast<const int32_t *>(b_dev), npairs, od.as<float>()));
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    return sync_if(ctx, need);
}

int pgv_hnsw_score_groups(pgv_hnsw *h, const int32_t *ids, const int64_t *ids_start, const int32_t *from,
                          const int64_t *pair_start, int ngroups, int64_t nids, int64_t npairs, float *out) {
    if (!h || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_score_groups: handle/out is NULL");
    PGV_NO_BUILD(h, "pgv_hnsw_score_groups");
    if (ngroups < 0 || nids < 0 || npairs < 0) PGV_FAIL(PGV_ERR_ARG, "bad sizes");
    if (ngroups == 0 || npairs == 0) return PGV_OK;
    if (!ids || !ids_start || !from || !pair_start) PGV_FAIL(PGV_ERR_ARG, "ids/ids_start/from/pair_start is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    // the four small tables in one staging buffer, the expanded slot arrays in two scratch buffers
    const size_t b_ids = (sizeof(int32_t) * (size_t)nids + 15) & ~(size_t)15,
                 b_start = sizeof(int64_t) * ((size_t)ngroups + 1),
                 b_from = (sizeof(int32_t) * (size_t)ngroups + 15) & ~(size_t)15;
    PGV_TRY(ctx->km_a.ensure(b_ids + 2 * b_start + b_from));
    char *tab = ctx->km_a.as<char>();
    auto put = [&](void *dst, const void *src, size_t bytes) -> int {
        PGV_HIP(hipMemcpyAsync(dst, src, bytes, is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               ctx->stream));
        return PGV_OK;
    };
    PGV_TRY(put(tab, ids, sizeof(int32_t) * (size_t)nids));
    PGV_TRY(put(tab + b_ids, ids_start, b_start));
    PGV_TRY(put(tab + b_ids + b_start, pair_start, b_start));
    PGV_TRY(put(tab + b_ids + 2 * b_start, from, sizeof(int32_t) * (size_t)ngroups));
    const int32_t *g_ids = reinterpret_cast<const int32_t *>(tab), *g_from = reinterpret_cast<const int32_t *>(tab + b_ids + 2 * b_start);
    const int64_t *g_at = reinterpret_cast<const int64_t *>(tab + b_ids), *g_pair = reinterpret_cast<const int64_t *>(tab + b_ids + b_start);
    OutArg od;
    PGV_TRY(od.init(out, sizeof(float) * (size_t)npairs, ctx->out_stage));
    const RowsView rows = hnsw_rows(h);
    if (hnsw_pairs_by_gather()) {
        PGV_TRY(ctx->idx_stage.ensure(sizeof(int32_t) * (size_t)npairs));
        PGV_TRY(ctx->plan_d.ensure(sizeof(int32_t) * (size_t)npairs));
        int32_t *a_dev = ctx->idx_stage.as<int32_t>(), *b_dev = ctx->plan_d.as<int32_t>();
        PGV_TRY(launch_expand_groups(ctx, g_ids, g_at, 0, nullptr, g_from, g_pair, ngroups, a_dev, b_dev));
        PGV_TRY(hnsw_score_gathered(ctx, rows, a_dev, b_dev, npairs, od.as<float>()));
    } else
        PGV_TRY(launch_score_groups(ctx, rows, g_ids, g_at, 0, nullptr, g_from, g_pair, ngroups, od.as<float>()));
    bool need = true;  // the host tables above must have been read before the caller reuses them
    PGV_TRY(od.finish(ctx, &need));
    return sync_if(ctx, need);
}

// ------------------------------------------------------------------ the build's graph updates on the device
static void hnsw_link_free(pgv_hnsw *o) {
    HnswLinkState *L = o->link;
    if (!L) return;
    if (L->nb_dist) (void)hipFree(L->nb_dist);
    if (L->nb_flag) (void)hipFree(L->nb_flag);
    if (L->list_count) (void)hipFree(L->list_count);
    if (L->stats_dev) (void)hipFree(L->stats_dev);
    if (L->stats_host) (void)hipHostFree(L->stats_host);
    L->rec.release();
    L->links.release();
    L->ids.release();
    L->pa.release();
    L->pb.release();
    L->tri.release();
    L->mm.release();
    L->loc.release();
    L->sel.release();
    for (int i = 0; i < 2; i++) {
        L->kept[i].ids.release();
        L->kept[i].dist.release();
        L->kept[i].cnt.release();
        L->kept[i].elems.release();
    }
    delete L;
    o->link = nullptr;
}

int pgv_hnsw_link_begin(pgv_hnsw *h) {
    if (!h) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_link_begin: handle is NULL");
    PGV_NO_BUILD(h, "pgv_hnsw_link_begin");
    if (h->imported || h->view_of) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_link_begin: an imported mirror / a view is read-only");
    if (h->graph.m == 0) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_link_begin needs pgv_hnsw_set_graph first");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    hnsw_link_free(h);
    HnswLinkState *L = new (std::nothrow) HnswLinkState();
    if (!L) PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    const size_t total = (size_t)(h->graph.nbr_total > 0 ? h->graph.nbr_total : 1);
    L->nlists = total / (size_t)h->graph.m + 1;  // every list starts at a multiple of m
    if (hipMalloc(&L->nb_dist, total * sizeof(float)) != hipSuccess || hipMalloc(&L->nb_flag, total) != hipSuccess ||
        hipMalloc(&L->list_count, 2 * L->nlists * sizeof(int)) != hipSuccess) {
        if (L->nb_dist) (void)hipFree(L->nb_dist);
        if (L->nb_flag) (void)hipFree(L->nb_flag);
        delete L;
        PGV_FAIL(PGV_ERR_NOMEM, "hipMalloc(%zu) for the hnsw build state failed", total * 5 + 2 * L->nlists * sizeof(int));
    }
    L->list_rec = L->list_count + L->nlists;
    if (hipMalloc(&L->stats_dev, 4 * sizeof(int64_t)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&L->stats_host), 4 * sizeof(int64_t), hipHostMallocDefault) != hipSuccess) {
        h->link = L;
        hnsw_link_free(h);
        PGV_FAIL(PGV_ERR_NOMEM, "no room for the hnsw build's counters");
    }
    memset(L->stats_host, 0, 4 * sizeof(int64_t));
    PGV_HIP(hipMemsetAsync(L->stats_dev, 0, 4 * sizeof(int64_t), ctx->stream));
    h->link = L;
    PGV_HIP(hipMemsetAsync(L->nb_dist, 0, total * sizeof(float), ctx->stream));
    PGV_HIP(hipMemsetAsync(L->nb_flag, 0, total, ctx->stream));
    PGV_HIP(hipMemsetAsync(L->list_count, 0, 2 * L->nlists * sizeof(int), ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    return PGV_OK;
}

int pgv_hnsw_link_prepare(pgv_hnsw *h, const int32_t *elements, const uint8_t *linked, int nq, int layer_cap,
                          const int32_t *sel_ids, const float *sel_dist, const uint8_t *sel_closer, const int32_t *sel_count,
                          int64_t *out_pairs) {
    PGV_NO_BUILD(h, "pgv_hnsw_link_prepare");
    if (!h || !h->link) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_link_prepare needs pgv_hnsw_link_begin");
    if (nq < 0 || layer_cap < 1) PGV_FAIL(PGV_ERR_ARG, "bad sizes");
    HnswLinkState *L = h->link;
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    if (out_pairs) *out_pairs = 0;
    L->nrec = 0;
    L->npairs = 0;
    L->nq = nq;
    L->lcap = layer_cap;
    L->prepared = true;
    if (nq == 0) return PGV_OK;
    if (!elements || !linked || !sel_ids || !sel_dist || !sel_closer || !sel_count)
        PGV_FAIL(PGV_ERR_ARG, "the new elements' lists are NULL");
    const HnswGraph &G = h->graph;
    const RowsView rows = hnsw_rows(h);
    const size_t per = (size_t)nq * layer_cap, stride = 2 * (size_t)G.m;
    if (per * stride > 0x7fffffff) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_link_prepare: batch too large");
    // a searcher on another stream has left the tuples as the last patch / link made them
    PGV_TRY(hnsw_graph_acquire(h));
    // the batch's own lists (pgv_hnsw_build_neighbors' output), kept until _apply puts them in place
    {
        const size_t b_ids = sizeof(int32_t) * per * stride, b_dist = sizeof(float) * per * stride, b_cnt = sizeof(int32_t) * per,
                     b_el = sizeof(int32_t) * (size_t)nq, b_cl = (per * stride + 15) & ~(size_t)15, b_ln = ((size_t)nq + 15) & ~(size_t)15;
        PGV_TRY(L->sel.ensure(b_ids + b_dist + b_cnt + b_el + b_cl + b_ln));
        char *base = L->sel.as<char>();
        L->d_sel_ids = reinterpret_cast<int32_t *>(base);
        L->d_sel_dist = reinterpret_cast<float *>(base + b_ids);
        L->d_sel_cnt = reinterpret_cast<int32_t *>(base + b_ids + b_dist);
        L->d_elems = reinterpret_cast<int32_t *>(base + b_ids + b_dist + b_cnt);
        L->d_sel_closer = reinterpret_cast<uint8_t *>(base + b_ids + b_dist + b_cnt + b_el);
        L->d_linked = L->d_sel_closer + b_cl;
        PGV_HIP(hipMemcpyAsync(L->d_sel_ids, sel_ids, b_ids, hipMemcpyDefault, ctx->stream));
        PGV_HIP(hipMemcpyAsync(L->d_sel_dist, sel_dist, b_dist, hipMemcpyDefault, ctx->stream));
        PGV_HIP(hipMemcpyAsync(L->d_sel_cnt, sel_count, b_cnt, hipMemcpyDefault, ctx->stream));
        PGV_HIP(hipMemcpyAsync(L->d_elems, elements, b_el, hipMemcpyDefault, ctx->stream));
        PGV_HIP(hipMemcpyAsync(L->d_sel_closer, sel_closer, per * stride, hipMemcpyDefault, ctx->stream));
        PGV_HIP(hipMemcpyAsync(L->d_linked, linked, (size_t)nq, hipMemcpyDefault, ctx->stream));
    }
    // records: at most one per request
    const size_t cap = per * stride, n1 = cap + 1;
    const size_t b64 = sizeof(int64_t) * (5 * n1 + 4), b32 = sizeof(int32_t) * (7 * n1 + 8);
    PGV_TRY(L->rec.ensure(b64 + b32));
    char *base = L->rec.as<char>();
    L->rec_off = reinterpret_cast<int64_t *>(base);
    L->rec_pos = L->rec_off + n1;
    L->ids_start = L->rec_pos + n1;
    L->pair_start = L->ids_start + n1;
    L->mm_start = L->pair_start + n1;
    L->totals = L->mm_start + n1;
    L->rec_owner = reinterpret_cast<int32_t *>(base + b64);
    L->rec_lc = L->rec_owner + n1;
    L->rec_nstart = L->rec_lc + n1;
    L->rec_from = L->rec_nstart + n1;
    L->rec_wait = L->rec_from + n1;
    L->rec_list = L->rec_wait + n1;
    L->rec_fill = reinterpret_cast<int *>(L->rec_list + n1);
    L->blocked = L->rec_fill + n1;
    L->nrec_dev = L->blocked + 2;
    PGV_TRY(L->links.ensure((sizeof(int32_t) + sizeof(float)) * cap));
    L->d_link_elem = L->links.as<int32_t>();
    L->d_link_dist = reinterpret_cast<float *>(L->d_link_elem + cap);
    PGV_HIP(hipMemsetAsync(L->nrec_dev, 0, sizeof(int), ctx->stream));
    PGV_TRY(launch_hnsw_link_group(ctx, 0, G, L->d_elems, L->d_linked, nq, layer_cap, L->d_sel_ids, L->d_sel_dist, L->d_sel_cnt,
                                   L->list_count, L->list_rec, L->nrec_dev, L->rec_owner, L->rec_lc, L->rec_list, nullptr,
                                   nullptr, nullptr, nullptr));
    int nrec = 0;
    PGV_HIP(hipMemcpyAsync(&nrec, L->nrec_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));  // (also: the caller's arrays have been read)
    if (nrec < 0 || (size_t)nrec > cap) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_link_prepare: %d records", nrec);
    L->nrec = nrec;
    if (nrec == 0) return PGV_OK;
    PGV_TRY(launch_hnsw_link_size(ctx, G, L->nb_flag, L->rec_owner, L->rec_lc, L->rec_list, L->list_count, L->rec_off, nrec, 0,
                                  L->rec_pos, L->rec_nstart, L->rec_from, nullptr, L->ids_start, L->pair_start));
    PGV_TRY(launch_hnsw_link_scan(ctx, L->rec_off, L->ids_start, L->pair_start, nrec, L->totals));
    PGV_HIP(hipMemsetAsync(L->rec_fill, 0, sizeof(int) * (size_t)nrec, ctx->stream));
    PGV_TRY(launch_hnsw_link_group(ctx, 1, G, L->d_elems, L->d_linked, nq, layer_cap, L->d_sel_ids, L->d_sel_dist, L->d_sel_cnt,
                                   L->list_count, L->list_rec, L->nrec_dev, L->rec_owner, L->rec_lc, L->rec_list, L->rec_off,
                                   L->rec_fill, L->d_link_elem, L->d_link_dist));
    int64_t totals[3] = {0, 0, 0};
    PGV_HIP(hipMemcpyAsync(totals, L->totals, sizeof(totals), hipMemcpyDeviceToHost, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t nlinks = totals[0], nids = totals[1], npairs = totals[2];
    const int64_t lm0 = 2 * (int64_t)G.m;
    if (nlinks < nrec || (size_t)nlinks > cap || nids < nlinks || nids > nlinks + (int64_t)nrec * lm0 || npairs < 0)
        PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_link_prepare: %lld links / %lld ids / %lld pairs planned for %d records",
                 (long long)nlinks, (long long)nids, (long long)npairs, nrec);
    PGV_TRY(L->ids.ensure(sizeof(int32_t) * (size_t)(nids > 0 ? nids : 1)));
    PGV_TRY(L->tri.ensure(sizeof(float) * (size_t)(npairs > 0 ? npairs : 1)));
    const bool gather = hnsw_pairs_by_gather();
    if (gather) {
        PGV_TRY(L->pa.ensure(sizeof(int32_t) * (size_t)(npairs > 0 ? npairs : 1)));
        PGV_TRY(L->pb.ensure(sizeof(int32_t) * (size_t)(npairs > 0 ? npairs : 1)));
    }
    // the id lists (and, for the gathered form, the slot pairs)
    PGV_TRY(launch_hnsw_link_pairs(ctx, G.nbr, L->rec_pos, L->rec_nstart, L->rec_from, L->rec_off, L->d_link_elem, L->d_link_dist,
                                   L->rec_list, L->list_count, nrec, 0, L->ids_start, L->ids.as<int32_t>(), L->pair_start,
                                   gather ? L->pa.as<int32_t>() : nullptr, gather ? L->pb.as<int32_t>() : nullptr));
    if (npairs > 0) {
        if (gather)
            PGV_TRY(hnsw_score_gathered(ctx, rows, L->pa.as<int32_t>(), L->pb.as<int32_t>(), npairs, L->tri.as<float>()));
        else
            PGV_TRY(launch_score_groups(ctx, rows, L->ids.as<int32_t>(), L->ids_start, 0, nullptr, L->rec_from, L->pair_start, nrec,
                                        L->tri.as<float>()));
    }
    L->npairs = npairs;
    if (out_pairs) *out_pairs = npairs;
    return PGV_OK;  // the scoring runs on; pgv_hnsw_link_apply is ordered behind it on the same stream
}

int pgv_hnsw_link_apply(pgv_hnsw *h, int32_t entry) {
    PGV_NO_BUILD(h, "pgv_hnsw_link_apply");
    if (!h || !h->link || !h->link->prepared) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_link_apply needs pgv_hnsw_link_prepare");
    if (entry < -1 || entry >= h->n) PGV_FAIL(PGV_ERR_ARG, "entry point %d out of range", (int)entry);
    HnswLinkState *L = h->link;
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    L->prepared = false;
    const HnswGraph &G = h->graph;
    const RowsView rows = hnsw_rows(h);
    const int nrec = L->nrec, m = G.m;
    if (nrec > 0) {
        PGV_TRY(L->loc.ensure(sizeof(int16_t) * (size_t)nrec * (2 * (size_t)m + 1)));
        PGV_HIP(hipMemsetAsync(L->blocked, 0, 2 * sizeof(int), ctx->stream));  // [0] stopped in the first round, [1] in the second
        PGV_TRY(launch_hnsw_link_replay(ctx, G, L->nb_dist, L->nb_flag, nrec, 0, L->rec_lc, L->rec_off, L->d_link_dist,
                                        L->rec_pos, L->rec_nstart, L->rec_from, L->ids_start, L->ids.as<int32_t>(), L->pair_start,
                                        L->tri.as<float>(), nullptr, nullptr, L->rec_wait, L->loc.as<int16_t>(), L->blocked));
        // The replays that stepped outside the pairs fetched for them: their lists' member-member triangles, then the rest
        // of their newcomers.  Everything is enqueued without waiting for a count: the triangles' room is the bound (every
        // record, a full list), launches cover every record and the ones that did not stop leave at once -- the host is
        // back before the first kernel has run, and the searches of the next batch but one start on the device the
        // moment the last one is through (hnsw_graph_acquire on their stream).
        const size_t lm0 = 2 * (size_t)m, mm_bound = (size_t)nrec * (lm0 * (lm0 - 1) / 2);
        const bool async = !hnsw_pairs_by_gather() && mm_bound * sizeof(float) <= ((size_t)512 << 20);
        PGV_TRY(launch_hnsw_link_size(ctx, G, L->nb_flag, L->rec_owner, L->rec_lc, L->rec_list, L->list_count, L->rec_off, nrec, 1,
                                      L->rec_pos, L->rec_nstart, L->rec_from, L->rec_wait, nullptr, L->mm_start));
        PGV_TRY(launch_hnsw_link_scan(ctx, L->mm_start, nullptr, nullptr, nrec, L->totals));
        if (async) {
            PGV_TRY(L->mm.ensure(sizeof(float) * (mm_bound > 0 ? mm_bound : 1)));
            PGV_TRY(launch_score_groups(ctx, rows, L->ids.as<int32_t>(), L->ids_start, 0, L->rec_nstart, nullptr, L->mm_start, nrec,
                                        L->mm.as<float>()));
        } else {
            int64_t npairs2 = 0;
            PGV_HIP(hipMemcpyAsync(&npairs2, L->totals, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
            PGV_HIP(hipStreamSynchronize(ctx->stream));
            if (npairs2 < 0 || (size_t)npairs2 > mm_bound)
                PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_link_apply: %lld member pairs planned for %d records", (long long)npairs2, nrec);
            PGV_TRY(L->mm.ensure(sizeof(float) * (size_t)(npairs2 > 0 ? npairs2 : 1)));
            if (npairs2 > 0 && hnsw_pairs_by_gather()) {
                PGV_TRY(L->pa.ensure(sizeof(int32_t) * (size_t)npairs2));
                PGV_TRY(L->pb.ensure(sizeof(int32_t) * (size_t)npairs2));
                PGV_TRY(launch_hnsw_link_pairs(ctx, G.nbr, L->rec_pos, L->rec_nstart, L->rec_from, L->rec_off, L->d_link_elem,
                                               L->d_link_dist, L->rec_list, L->list_count, nrec, 1, L->ids_start,
                                               L->ids.as<int32_t>(), L->mm_start, L->pa.as<int32_t>(), L->pb.as<int32_t>()));
                PGV_TRY(hnsw_score_gathered(ctx, rows, L->pa.as<int32_t>(), L->pb.as<int32_t>(), npairs2, L->mm.as<float>()));
            } else if (npairs2 > 0)
                PGV_TRY(launch_score_groups(ctx, rows, L->ids.as<int32_t>(), L->ids_start, 0, L->rec_nstart, nullptr, L->mm_start,
                                            nrec, L->mm.as<float>()));
        }
        PGV_TRY(launch_hnsw_link_replay(ctx, G, L->nb_dist, L->nb_flag, nrec, 1, L->rec_lc, L->rec_off, L->d_link_dist,
                                        L->rec_pos, L->rec_nstart, L->rec_from, L->ids_start, L->ids.as<int32_t>(), L->pair_start,
                                        L->tri.as<float>(), L->mm_start, L->mm.as<float>(), L->rec_wait, L->loc.as<int16_t>(),
                                        L->blocked + 1));
        // the counts: added up on the device, copied to pinned memory behind the launches (read at the end)
        PGV_TRY(launch_hnsw_link_stats(ctx, L->blocked, L->totals, L->stats_dev));
        PGV_HIP(hipMemcpyAsync(L->stats_host, L->stats_dev, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    // the batch's own elements (their lists were selected with their searches)
    if (L->nq > 0)
        PGV_TRY(launch_hnsw_link_new(ctx, G, L->nb_dist, L->nb_flag, L->d_elems, L->d_linked, L->nq, L->lcap, L->d_sel_ids,
                                     L->d_sel_dist, L->d_sel_closer, L->d_sel_cnt));
    h->graph.entry = entry;
    // searches on other streams (the helper's view) wait for this on the device
    if (!h->graph_ev) PGV_HIP(hipEventCreateWithFlags(&h->graph_ev, hipEventDisableTiming));
    PGV_HIP(hipEventRecord(h->graph_ev, ctx->stream));
    h->graph_ev_set = true;
    return PGV_OK;
}

int pgv_hnsw_link_end(pgv_hnsw *h, int32_t *out_nbr, int64_t *out_pairs, int64_t *out_deferred) {
    if (!h) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_link_end: handle is NULL");
    PGV_NO_BUILD(h, "pgv_hnsw_link_end");
    if (out_pairs) *out_pairs = 0;
    if (out_deferred) *out_deferred = 0;
    if (!h->link) return PGV_OK;
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_TRY(hnsw_graph_acquire(h));
    if (out_nbr && h->graph.nbr_total > 0)
        PGV_HIP(hipMemcpyAsync(out_nbr, h->graph.nbr, sizeof(int32_t) * (size_t)h->graph.nbr_total, hipMemcpyDefault, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t deferred = h->link->stats_host[0], pairs2 = h->link->stats_host[1], still = h->link->stats_host[2];
    hnsw_link_free(h);
    if (still != 0) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_link_end: %lld list updates were left waiting for distances", (long long)still);
    if (out_pairs) *out_pairs = pairs2;
    if (out_deferred) *out_deferred = deferred;
    return PGV_OK;
}

int pgv_hnsw_update_graph(pgv_hnsw *h, int32_t entry, const int32_t *elements, int nupd,
                          const int64_t *tuple_offsets, const int32_t *tuples) {
    if (!h) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_update_graph: handle is NULL");
    if (h->imported) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_update_graph: an imported mirror is read-only");
    hnsw_view_refresh(h);
    // through a view (pgv_hnsw_share) the patch lands in the owner's arrays, on the view's stream
    pgv_hnsw *o = h->view_of ? h->view_of : h;
    if (o->imported) PGV_FAIL(PGV_ERR_STATE, "pgv_hnsw_update_graph: an imported mirror is read-only");
    if (h->graph.m == 0) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_update_graph needs pgv_hnsw_set_graph first");
    if (entry < -1 || entry >= h->n) PGV_FAIL(PGV_ERR_ARG, "entry point %d out of range", (int)entry);
    if (nupd < 0 || (nupd > 0 && (!elements || !tuple_offsets || !tuples))) PGV_FAIL(PGV_ERR_ARG, "bad update");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    h->graph.entry = entry;
    o->graph.entry = entry;
    if (nupd == 0) return PGV_OK;
    if (is_device_ptr(tuple_offsets)) PGV_FAIL(PGV_ERR_ARG, "tuple_offsets must be host memory");
    const int64_t total = tuple_offsets[nupd];
    for (int i = 0; i < nupd; i++)
        if (tuple_offsets[i] < 0 || tuple_offsets[i + 1] < tuple_offsets[i])
            PGV_FAIL(PGV_ERR_ARG, "tuple_offsets is not an offset array");
    // an earlier patch that ran on another stream comes first
    PGV_TRY(hnsw_graph_acquire(h));
    const void *id_dev, *tp_dev, *of_dev;
    PGV_TRY(stage_flat(ctx, elements, sizeof(int32_t) * (size_t)nupd, ctx->idx_stage, &id_dev));
    PGV_TRY(stage_flat(ctx, tuples, sizeof(int32_t) * (size_t)(total > 0 ? total : 1), ctx->plan_d, &tp_dev));
    PGV_TRY(stage_flat(ctx, tuple_offsets, sizeof(int64_t) * (size_t)(nupd + 1), ctx->plan_c, &of_dev));
    PGV_TRY(launch_hnsw_patch(ctx, h->graph, h->n, static_cast<const int32_t *>(id_dev),
                              static_cast<const int64_t *>(of_dev), static_cast<const int32_t *>(tp_dev), nupd));
    // later launches on this stream see the patched graph; searches on other streams (the owner's, other views') wait
    // for this event on the device.  The caller keeps searches that READ the old tuples away from the patch: they have
    // returned (every search ends with a stream synchronize) before it calls this.
    if (!o->graph_ev) PGV_HIP(hipEventCreateWithFlags(&o->graph_ev, hipEventDisableTiming));
    PGV_HIP(hipEventRecord(o->graph_ev, ctx->stream));
    o->graph_ev_set = true;
    return PGV_OK;
}

// ------------------------------------------------------------------ dead elements and hnswvacuum's repair search
// Which mirrors the repair entries serve: dense ones of this process (pgv_hnsw_upload / _upload_payload and their views).
static int hnsw_repair_mirror(const pgv_hnsw *h, const char *who) {
    if (hnsw_is_sparse(h))
        PGV_FAIL(PGV_ERR_ARG, "%s: a sparse mirror (pgv_hnsw_upload_sparse) has no dead elements and is not repaired: dense mirrors only", who);
    if (hnsw_is_bits(h) && (int)h->metric == (int)PGV_BIT_JACCARD)
        PGV_FAIL(PGV_ERR_ARG, "%s: a Jaccard bit mirror (pgv_hnsw_upload_jaccard) has no dead elements and is not repaired: dense mirrors only", who);
    if (hnsw_is_bits(h))
        PGV_FAIL(PGV_ERR_ARG, "%s: a bit mirror (pgv_hnsw_upload_bits) has no dead elements and is not repaired: dense mirrors only", who);
    const pgv_hnsw *o = h->view_of ? h->view_of : h;
    if (h->imported || o->imported)
        PGV_FAIL(PGV_ERR_ARG, "%s: an imported mirror (pgv_hnsw_import) is read-only: the process that uploaded it repairs it", who);
    return PGV_OK;
}

int pgv_hnsw_set_live(pgv_hnsw *h, const uint32_t *live, int64_t words) {
    if (!h) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_set_live: handle is NULL");
    PGV_TRY(hnsw_repair_mirror(h, "pgv_hnsw_set_live"));
    pgv_hnsw *o = h->view_of ? h->view_of : h;
    if (!live) {
        o->live_set = false;
        o->live_count = 0;
        return PGV_OK;
    }
    const int64_t want = (h->n + 31) / 32;
    if (words != want)
        PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_set_live: %lld words for %lld elements, expected %lld", (long long)words, (long long)h->n,
                 (long long)want);
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    // no repair search of THIS handle may still be reading the old bitmap; the ones other views of the mirror launched
    // are the caller's to have finished (they end synchronized, like every search: pgv_hip.h)
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    PGV_TRY(o->live.ensure(want > 0 ? (size_t)want * sizeof(uint32_t) : 16));
    std::vector<uint32_t> host((size_t)want);
    if (want > 0) {
        PGV_HIP(hipMemcpy(host.data(), live, (size_t)want * sizeof(uint32_t), hipMemcpyDefault));
        if (h->n & 31) host[(size_t)want - 1] &= (1u << (h->n & 31)) - 1u;  // bits past the last element say nothing
        PGV_HIP(hipMemcpyAsync(o->live.p, host.data(), (size_t)want * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        PGV_HIP(hipStreamSynchronize(ctx->stream));
    }
    int64_t count = 0;
    for (uint32_t w : host) count += __builtin_popcount(w);
    o->live_count = count;
    o->live_set = true;
    return PGV_OK;
}

int64_t pgv_hnsw_live_count(const pgv_hnsw *h) {
    if (!h) return -1;
    if (hnsw_repair_mirror(h, "pgv_hnsw_live_count") != PGV_OK) return -1;  // (the text names the mirror kind)
    const pgv_hnsw *o = h->view_of ? h->view_of : h;
    return o->live_set ? o->live_count : h->n;
}

int pgv_hnsw_repair_dead_cap_max(const pgv_hnsw *h, int ef_construction) {
    if (!h || h->sparse || h->nbits > 0) return -1;
    const pgv_hnsw *o = h->view_of ? h->view_of : h;
    if (o->graph.m == 0 || ef_construction < 4 || ef_construction > 1000) return -1;
    return hnsw_repair_dead_cap_max(h->geom, ef_construction, o->graph.m);
}

int pgv_hnsw_repair_neighbors(pgv_hnsw *h, const int32_t *elements, int nq, int ef_construction, int layer_cap, int dead_cap,
                              int32_t *out_ids, float *out_dist, uint8_t *out_closer, int32_t *out_count, int32_t *out_status,
                              int64_t *out_pairs) {
    if (!h || !out_ids || !out_dist || !out_closer || !out_count || !out_status)
        PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_repair_neighbors: handle/out is NULL");
    PGV_TRY(hnsw_repair_mirror(h, "pgv_hnsw_repair_neighbors"));
    hnsw_view_refresh(h);
    if (dead_cap < 0 || dead_cap > 0x3fffffff) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_repair_neighbors: dead_cap %d", dead_cap);
    PGV_TRY(hnsw_build_args(h, "pgv_hnsw_repair_neighbors", nq, ef_construction, layer_cap));
    // W's capacity: the stride of the candidate lists the selection reads
    PGV_TRY(hnsw_repair_lds_check("pgv_hnsw_repair_neighbors", h->geom, ef_construction, dead_cap, h->graph.m, nullptr));
    const int wcap = ef_construction + 1 + dead_cap;
    if ((size_t)nq * layer_cap > 0x7fffffff / (size_t)wcap) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_repair_neighbors: batch too large");
    if (out_pairs) *out_pairs = 0;
    if (nq == 0) return PGV_OK;
    if (!elements) PGV_FAIL(PGV_ERR_ARG, "elements is NULL");
    if (!is_device_ptr(elements))
        for (int i = 0; i < nq; i++)
            if (elements[i] < 0 || elements[i] >= h->n)
                PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_repair_neighbors: element %d (entry %d of the batch) is not a slot of the mirror",
                         (int)elements[i], i);
    pgv_ctx *ctx = h->ctx;
    pgv_hnsw *o = h->view_of ? h->view_of : h;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_TRY(hnsw_graph_acquire(h));
    const size_t per = (size_t)nq * layer_cap;
    const void *e_dev;
    PGV_TRY(stage_flat(ctx, elements, sizeof(int32_t) * (size_t)nq, ctx->idx_stage, &e_dev));
    // the candidate lists stay on the device, as the build's: km_b ids | km_c distances | km_d counts; plan_c the levels
    PGV_TRY(ctx->km_b.ensure(sizeof(int32_t) * per * wcap));
    PGV_TRY(ctx->km_c.ensure(sizeof(float) * per * wcap));
    PGV_TRY(ctx->km_d.ensure(sizeof(int32_t) * per));
    PGV_TRY(ctx->plan_c.ensure(sizeof(int32_t) * (size_t)nq));
    OutArg os;
    PGV_TRY(os.init(out_status, sizeof(int32_t) * (size_t)nq, ctx->plan_d));
    HnswRepairArgs a;
    a.qids = static_cast<const int32_t *>(e_dev);
    a.nq = nq;
    a.ef_construction = ef_construction;
    a.dead_cap = dead_cap;
    a.lcap = layer_cap;
    a.lw_ids = ctx->km_b.as<int32_t>();
    a.lw_dist = ctx->km_c.as<float>();
    a.lw_cnt = ctx->km_d.as<int32_t>();
    a.qlevels = ctx->plan_c.as<int32_t>();
    a.status = os.as<int32_t>();
    int words = 0;
    const int grid = hnsw_search_grid(ctx, nq, h->n, &words);
    PGV_TRY(h->bitmaps.ensure((size_t)grid * words * sizeof(uint32_t)));
    PGV_TRY(ctx->counters.ensure(256));
    PGV_TRY(launch_hnsw_repair(ctx, hnsw_rows(h), h->graph, o->live_set ? o->live.as<uint32_t>() : nullptr, a,
                               h->bitmaps.as<uint32_t>(), words, grid, ctx->counters.as<int>()));
    bool need = false;
    PGV_TRY(os.finish(ctx, &need));
    return hnsw_select_from(h, a.lw_ids, a.lw_dist, a.lw_cnt, a.qlevels, nq, wcap, layer_cap, out_ids, out_dist, out_closer,
                            out_count, out_pairs);
}

// ------------------------------------------------------------------ resumable scans: hnsw.iterative_scan on the device
// GetScanItems (src/hnswscan.c:25-56) for a query's first batch, ResumeScanItems (:61-87) for the later ones: what the
// reference keeps in so->v and so->discarded lives here, per query, between the launches.

struct pgv_hnsw_scan {
    pgv_hnsw *h = nullptr;
    int nq = 0, ef = 0, cap = 0, words = 0;
    void *queries = nullptr;  // [nq] rows in the mirror's layout (the scan's own copy: the caller's may go away), or over a
    void *q_ptr = nullptr;    // sparse mirror the queries in CSR, the scan's own copy as well: [nq + 1] offsets,
    void *q_idx = nullptr;    // ... the indices and
    void *q_val = nullptr;    // ... the values, as stage_query reads them
    int max_q_nnz = 0;        // the longest query's stored elements: every batch's LDS is sized by it
    void *bitmaps = nullptr;  // [nq x words] one visited set per query
    void *pool = nullptr;     // [nq x cap] (key, element)
    void *qstate = nullptr;   // [nq x kHnswScanQueryBytes], then the overflow word
    int failed_query = -1;    // a pool overflowed: every later call repeats the error
};

static int hnsw_scan_overflowed(const pgv_hnsw_scan *s) {
    PGV_FAIL(PGV_ERR_NOMEM,
             "pgv_hnsw_scan: the discarded candidates of query %d outgrew the scan's capacity of %d entries per query "
             "(discard_cap); the scan is over, the mirror is unaffected",
             s->failed_query, s->cap);
}

// what both begins check after their handle: the counts, and that there is a graph to walk
static int hnsw_scan_check(pgv_hnsw *h, const char *who, int nq, int ef_search, int64_t discard_cap) {
    if (nq < 0) PGV_FAIL(PGV_ERR_ARG, "bad query count");
    if (ef_search < 1 || ef_search > 1000)
        PGV_FAIL(PGV_ERR_ARG, "hnsw.ef_search must be 1..1000 (src/hnsw.c:93-94), got %d", ef_search);
    if (discard_cap < 0) PGV_FAIL(PGV_ERR_ARG, "discard_cap must be >= 0, got %lld", (long long)discard_cap);
    if (h->graph.m == 0) PGV_FAIL(PGV_ERR_ARG, "%s needs pgv_hnsw_set_graph first", who);
    return PGV_OK;
}

// A scan's state on the device, its query copy included: qbytes[i] bytes for *qbufs[i] (nqbufs of them, fields of the new
// scan), then the visited sets, the pools and the per-query state.  Nothing is written yet.  PGV_ERR_NOMEM frees it all.
static int hnsw_scan_alloc(pgv_hnsw *h, const char *who, int nq, int ef_search, int64_t discard_cap, const size_t *qbytes,
                           int nqbufs, void **(*qbuf)(pgv_hnsw_scan *, int), pgv_hnsw_scan **out, size_t *sbytes_out) {
    pgv_hnsw_scan *s = new (std::nothrow) pgv_hnsw_scan();
    if (!s) PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    s->h = h;
    s->nq = nq;
    s->ef = ef_search;
    if (discard_cap == 0) discard_cap = h->n < 65536 ? h->n : 65536;
    if (discard_cap < 1) discard_cap = 1;
    if (discard_cap > 0x7fffffff / 2) discard_cap = 0x7fffffff / 2;
    s->cap = (int)discard_cap;
    s->words = (int)((h->n + 31) / 32) + 1;
    const size_t rows = (size_t)(nq > 0 ? nq : 1);
    const size_t bbytes = rows * (size_t)s->words * sizeof(uint32_t), pbytes = rows * (size_t)s->cap * 8,
                 sbytes = rows * kHnswScanQueryBytes + 16;
    void **bufs[6];
    size_t sizes[6], total = 0;
    int nb = 0;
    for (int i = 0; i < nqbufs; i++, nb++) {
        bufs[nb] = qbuf(s, i);
        sizes[nb] = qbytes[i];
    }
    bufs[nb] = &s->bitmaps, sizes[nb++] = bbytes;
    bufs[nb] = &s->pool, sizes[nb++] = pbytes;
    bufs[nb] = &s->qstate, sizes[nb++] = sbytes;
    for (int i = 0; i < nb; i++) total += sizes[i];
    for (int i = 0; i < nb; i++)
        if (hipMalloc(bufs[i], sizes[i]) != hipSuccess) {
            (void)hipGetLastError();
            *bufs[i] = nullptr;
            const int cap = s->cap, words = s->words;
            pgv_hnsw_scan_end(s);
            PGV_FAIL(PGV_ERR_NOMEM, "%s: hipMalloc(%zu) failed; the state of %d queries takes %zu bytes "
                                    "(discard_cap %d, %d bitmap words per query)",
                     who, sizes[i], nq, total, cap, words);
        }
    *sbytes_out = sbytes;
    *out = s;
    return PGV_OK;
}

// the end of both begins: the query copy is on its way (rc, on the handle's stream); zero the per-query state and wait --
// the caller may reuse its query arrays right away
static int hnsw_scan_publish(pgv_hnsw_scan *s, const char *who, int rc, hipError_t e, size_t sbytes, pgv_hnsw_scan **out) {
    pgv_ctx *ctx = s->h->ctx;
    if (rc == PGV_OK && e == hipSuccess) e = hipMemsetAsync(s->qstate, 0, sbytes, ctx->stream);
    if (rc == PGV_OK && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (rc != PGV_OK || e != hipSuccess) {
        pgv_hnsw_scan_end(s);
        if (rc != PGV_OK) return rc;
        PGV_FAIL(PGV_ERR_DEVICE, "%s: staging failed: %s", who, hipGetErrorString(e));
    }
    *out = s;
    return PGV_OK;
}

int pgv_hnsw_scan_begin(pgv_hnsw *h, const void *queries, int nq, int ef_search, int64_t discard_cap, pgv_hnsw_scan **out) {
    const char *who = "pgv_hnsw_scan_begin";
    if (!h || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_scan_begin: handle/out is NULL");
    *out = nullptr;
    PGV_NO_SPARSE(h, who, "pgv_hnsw_scan_begin_sparse");
    hnsw_view_refresh(h);
    PGV_TRY(hnsw_scan_check(h, who, nq, ef_search, discard_cap));
    if (nq > 0 && !queries) PGV_FAIL(PGV_ERR_ARG, "queries is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    const size_t qbytes = (size_t)(nq > 0 ? nq : 1) * hnsw_row_bytes(h->geom);
    pgv_hnsw_scan *s = nullptr;
    size_t sbytes = 0;
    PGV_TRY(hnsw_scan_alloc(h, who, nq, ef_search, discard_cap, &qbytes, 1,
                            [](pgv_hnsw_scan *sc, int) -> void ** { return &sc->queries; }, &s, &sbytes));
    const int rc = put_padded_rows(ctx->stream, s->queries, hnsw_row_bytes(h->geom), queries,
                                   hnsw_src_row_bytes(h->dim, h->dtype, h->nbits), nq);
    return hnsw_scan_publish(s, who, rc, hipSuccess, sbytes, out);
}

// hnswbeginscan / hnswrescan on a sparse mirror: the queries in CSR, validated and staged as pgv_hnsw_search_sparse's, then
// copied into the scan's own three arrays (offsets, indices, values -- the layout stage_query reads; 8 bytes per stored
// element either way) so that the context's staging buffers and the caller's arrays are free again when this returns
int pgv_hnsw_scan_begin_sparse(pgv_hnsw *h, const int64_t *q_ptr, const int32_t *q_idx, const float *q_val, int nq, int ef_search,
                               int64_t discard_cap, pgv_hnsw_scan **out) {
    const char *who = "pgv_hnsw_scan_begin_sparse";
    if (!h || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_scan_begin_sparse: handle/out is NULL");
    *out = nullptr;
    PGV_ONLY_SPARSE(h, who);
    hnsw_view_refresh(h);
    PGV_TRY(hnsw_scan_check(h, who, nq, ef_search, discard_cap));
    if (!q_ptr) PGV_FAIL(PGV_ERR_ARG, "q_ptr is NULL");
    pgv_ctx *ctx = h->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    StagedCsr q;
    int max_nnz = 0;
    PGV_TRY(hnsw_stage_sparse_queries(h, who, q_ptr, q_idx, q_val, nq, &q, &max_nnz));
    // every batch carves the same LDS, sized by the scan's longest query: too much is refused here, not at the first next
    PGV_TRY(hnsw_sparse_scan_lds_check(who, h->metric, ef_search, h->graph.m, max_nnz));
    const int64_t total = q.host_ptr[nq];
    const size_t elems = (size_t)(total > 0 ? total : 1);
    const size_t qbytes[3] = {sizeof(int64_t) * ((size_t)nq + 1), sizeof(int32_t) * elems, sizeof(float) * elems};
    pgv_hnsw_scan *s = nullptr;
    size_t sbytes = 0;
    PGV_TRY(hnsw_scan_alloc(h, who, nq, ef_search, discard_cap, qbytes, 3,
                            [](pgv_hnsw_scan *sc, int i) -> void ** { return i == 0 ? &sc->q_ptr : i == 1 ? &sc->q_idx : &sc->q_val; },
                            &s, &sbytes));
    s->max_q_nnz = max_nnz;
    hipError_t e = hipMemcpyAsync(s->q_ptr, q.dev.ptr, qbytes[0], hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess && total > 0)
        e = hipMemcpyAsync(s->q_idx, q.dev.idx, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess && total > 0)
        e = hipMemcpyAsync(s->q_val, q.dev.val, sizeof(float) * (size_t)total, hipMemcpyDeviceToDevice, ctx->stream);
    return hnsw_scan_publish(s, who, PGV_OK, e, sbytes, out);
}

// what pgv_hnsw_scan_filtered hands a launch on top: hnswgettuple's loop runs inside it
struct HnswScanFilter {
    const uint32_t *keep;
    int64_t keep_stride;
    int k;
    int64_t max_scan_tuples;
    bool strict;
    int32_t *out_batches;
};

// one launch over the scan's state: a batch of every wanted query (ef = the scan's), the drain of their pools, or -- with
// `filter` -- every wanted query's whole filtered scan (out_elem / out_dist are then [nq x filter->k])
static int hnsw_scan_launch(pgv_hnsw_scan *s, const uint8_t *want, int ef, bool drain, int64_t *out_elem, float *out_dist,
                            int32_t *out_count, int64_t *out_scored, int64_t *out_left,
                            const HnswScanFilter *filter = nullptr) {
    pgv_hnsw *h = s->h;
    pgv_ctx *ctx = h->ctx;
    hnsw_view_refresh(h);
    if (s->nq == 0) return PGV_OK;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_TRY(hnsw_graph_acquire(h));
    const void *w_dev = nullptr;
    if (want) PGV_TRY(stage_flat(ctx, want, (size_t)s->nq, ctx->idx_stage, &w_dev));
    const int width = filter ? filter->k : ef;  // of an output row
    const void *keep_dev = nullptr;
    if (filter && filter->keep) {
        const size_t kwords = filter->keep_stride ? (size_t)s->nq * (size_t)filter->keep_stride : (size_t)(s->words - 1);
        PGV_TRY(stage_flat(ctx, filter->keep, sizeof(uint32_t) * kwords, ctx->rows_stage, &keep_dev));
    }
    OutArg oe, od, oc, os, ol, ob;
    PGV_TRY(oe.init(out_elem, sizeof(int64_t) * (size_t)s->nq * width, ctx->out_stage2));
    PGV_TRY(od.init(out_dist, sizeof(float) * (size_t)s->nq * width, ctx->out_stage));
    PGV_TRY(ob.init(filter ? filter->out_batches : nullptr, sizeof(int32_t) * (size_t)s->nq, ctx->plan_b));
    PGV_TRY(oc.init(out_count, sizeof(int32_t) * (size_t)s->nq, ctx->sel_a));
    PGV_TRY(os.init(out_scored, sizeof(int64_t) * (size_t)s->nq, ctx->sel_b));
    PGV_TRY(ol.init(out_left, sizeof(int64_t) * (size_t)s->nq, ctx->plan_a));
    PGV_TRY(ctx->counters.ensure(256));
    HnswSearchArgs a;
    a.queries = s->queries;
    if (hnsw_is_sparse(h)) {
        a.sparse_queries = {static_cast<const int64_t *>(s->q_ptr), static_cast<const int32_t *>(s->q_idx),
                            static_cast<const float *>(s->q_val), s->nq};
        a.max_q_nnz = drain ? 0 : s->max_q_nnz;  // (a drain stages no query: count up to 1000 fits whatever the queries store)
    }
    a.nq = s->nq;
    a.ef = ef;
    a.k = width;
    a.out_elem = oe.as<int64_t>();
    a.out_dist = od.as<float>();
    a.out_scored = out_scored ? os.as<int64_t>() : nullptr;
    HnswScanArgs sa;
    sa.pool = s->pool;
    sa.cap = s->cap;
    sa.qstate = s->qstate;
    sa.want = static_cast<const uint8_t *>(w_dev);
    sa.out_count = oc.as<int32_t>();
    sa.out_left = out_left ? ol.as<int64_t>() : nullptr;
    sa.overflow = reinterpret_cast<int *>(static_cast<char *>(s->qstate) + (size_t)s->nq * kHnswScanQueryBytes);
    sa.drain = drain;
    if (filter) {
        sa.filtered = true;
        sa.keep = static_cast<const uint32_t *>(keep_dev);
        sa.keep_stride = filter->keep_stride;
        sa.max_scan_tuples = filter->max_scan_tuples;
        sa.strict = filter->strict;
        sa.out_batches = ob.as<int32_t>();
    }
    // one workgroup per query (an unwanted or exhausted one's only writes its empty outputs): each has its own visited
    // set, so nothing caps the grid but the queries
    const int grid = s->nq < ctx->num_cus * 8 ? s->nq : ctx->num_cus * 8;
    PGV_TRY(launch_hnsw_search(ctx, hnsw_rows(h), h->graph, a, static_cast<uint32_t *>(s->bitmaps), s->words, grid,
                               ctx->counters.as<int>(), &sa));
    int over = 0;
    PGV_HIP(hipMemcpyAsync(&over, sa.overflow, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    bool need = false;
    PGV_TRY(oe.finish(ctx, &need));
    PGV_TRY(od.finish(ctx, &need));
    PGV_TRY(oc.finish(ctx, &need));
    PGV_TRY(os.finish(ctx, &need));
    PGV_TRY(ol.finish(ctx, &need));
    PGV_TRY(ob.finish(ctx, &need));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    if (over > 0) {
        s->failed_query = over - 1;
        return hnsw_scan_overflowed(s);
    }
    return PGV_OK;
}

int pgv_hnsw_scan_next(pgv_hnsw_scan *s, const uint8_t *want, int64_t *out_elem, float *out_dist, int32_t *out_count,
                       int64_t *out_scored, int64_t *out_left) {
    if (!s || !out_elem || !out_dist || !out_count) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_scan_next: scan/out is NULL");
    if (s->failed_query >= 0) return hnsw_scan_overflowed(s);
    return hnsw_scan_launch(s, want, s->ef, false, out_elem, out_dist, out_count, out_scored, out_left);
}

int pgv_hnsw_scan_drain(pgv_hnsw_scan *s, const uint8_t *want, int count, int64_t *out_elem, float *out_dist,
                        int32_t *out_count) {
    if (!s || !out_elem || !out_dist || !out_count) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_scan_drain: scan/out is NULL");
    if (count < 1 || count > 1000) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_scan_drain: count must be 1..1000, got %d", count);
    if (s->failed_query >= 0) return hnsw_scan_overflowed(s);
    return hnsw_scan_launch(s, want, count, true, out_elem, out_dist, out_count, nullptr, nullptr);
}

int pgv_hnsw_scan_filtered(pgv_hnsw_scan *s, const uint8_t *want, const uint32_t *keep, int64_t keep_stride, int k,
                           int64_t max_scan_tuples, int strict, int64_t *out_elem, float *out_dist, int32_t *out_count,
                           int64_t *out_scored, int32_t *out_batches, int64_t *out_left) {
    if (!s || !out_elem || !out_dist || !out_count) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_scan_filtered: scan/out is NULL");
    if (k < 1 || k > 4096) PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_scan_filtered: k must be 1..4096, got %d", k);
    if (max_scan_tuples < 1)
        PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_scan_filtered: max_scan_tuples must be >= 1, got %lld", (long long)max_scan_tuples);
    const int64_t kwords = s->words - 1;  // (n + 31) / 32 of the mirror the scan began on
    if (keep_stride != 0 && keep_stride < kwords)
        PGV_FAIL(PGV_ERR_ARG, "pgv_hnsw_scan_filtered: keep_stride %lld is below the %lld words of one bitmap over the mirror",
                 (long long)keep_stride, (long long)kwords);
    if (s->failed_query >= 0) return hnsw_scan_overflowed(s);
    const HnswScanFilter f{keep, keep ? keep_stride : 0, k, max_scan_tuples, strict != 0, out_batches};
    return hnsw_scan_launch(s, want, s->ef, false, out_elem, out_dist, out_count, out_scored, out_left, &f);
}

void pgv_hnsw_scan_end(pgv_hnsw_scan *s) {
    if (!s) return;
    if (s->h && s->h->ctx) {
        (void)hipSetDevice(s->h->ctx->device);
        (void)hipStreamSynchronize(s->h->ctx->stream);
    }
    if (s->queries) (void)hipFree(s->queries);
    if (s->q_ptr) (void)hipFree(s->q_ptr);
    if (s->q_idx) (void)hipFree(s->q_idx);
    if (s->q_val) (void)hipFree(s->q_val);
    if (s->bitmaps) (void)hipFree(s->bitmaps);
    if (s->pool) (void)hipFree(s->pool);
    if (s->qstate) (void)hipFree(s->qstate);
    delete s;
}

}  // extern "C"
