// pgv_abi_ivf.hip -- extern "C" entry points of libpgv_hip (include/pgv_hip.h): the IVFFlat mirror, the build's tuplesort on the device, list scans, one query at a time.
// Split out of pgv_abi.hip in round 5 (one unit per area, so that an edit recompiles one of them).
#include "pgv_abi_common.h"

extern "C" {

// ============================================================== IVFFlat index

namespace {
// where each device array of an IVFFlat mirror sits inside its one allocation
struct IndexLayout {
    size_t centers, vectors, offsets, tids, row_norms, center_norms, bytes;
    bool has_tids, has_norms;
};
IndexLayout index_layout(int nlists, int64_t n, size_t row_bytes, bool has_tids, bool l2) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    IndexLayout L{};
    size_t at = 0;
    L.centers = at; at = up(at + (size_t)nlists * row_bytes);
    L.vectors = at; at = up(at + (size_t)(n > 0 ? n : 1) * row_bytes);
    L.offsets = at; at = up(at + sizeof(int64_t) * ((size_t)nlists + 1));
    L.has_tids = has_tids;
    L.tids = at; if (has_tids) at = up(at + sizeof(uint64_t) * (size_t)n);
    L.has_norms = l2;
    L.row_norms = at; if (l2 && n > 0) at = up(at + sizeof(float) * ((size_t)n + 1));
    L.center_norms = at; if (l2) at = up(at + sizeof(float) * ((size_t)nlists + 1));
    L.bytes = at;
    return L;
}
void index_carve(pgv_index *ix, const IndexLayout &L) {
    char *b = static_cast<char *>(ix->arena);
    ix->centers = b + L.centers;
    ix->vectors = b + L.vectors;
    ix->list_offsets = reinterpret_cast<int64_t *>(b + L.offsets);
    ix->tids = L.has_tids ? reinterpret_cast<uint64_t *>(b + L.tids) : nullptr;
    ix->row_norms = L.has_norms && ix->nrows > 0 ? reinterpret_cast<float *>(b + L.row_norms) : nullptr;
    ix->center_norms = L.has_norms ? reinterpret_cast<float *>(b + L.center_norms) : nullptr;
}
// len_prefix / max_list_len from h_offsets
void index_host_tables(pgv_index *ix) {
    const int nlists = ix->nlists;
    std::vector<int64_t> lens((size_t)nlists);
    int64_t maxlen = 0;
    for (int l = 0; l < nlists; l++) {
        lens[l] = ix->h_offsets[l + 1] - ix->h_offsets[l];
        if (lens[l] > maxlen) maxlen = lens[l];
    }
    ix->max_list_len = maxlen;
    std::sort(lens.begin(), lens.end(), [](int64_t a, int64_t b) { return a > b; });
    ix->len_prefix.assign((size_t)nlists + 1, 0);
    for (int l = 0; l < nlists; l++) ix->len_prefix[l + 1] = ix->len_prefix[l] + lens[l];
}
}  // namespace

extern "C++" {
namespace {

// PGV_SCAN_SHADOW: 0 = never build or use the fp16 residual shadow, 1 = always (fp32 L2 indexes), unset = the default
// policy: fp32 L2 indexes whose rows stream past the caches (what the list scan reads from HBM; below that the shadow
// would only cost memory).  Read at every index creation and batch, so that one process can compare both forms
int shadow_env() {
    const char *e = getenv("PGV_SCAN_SHADOW");
    return e ? atoi(e) : -1;
}

// PGV_RANK_SHADOW: how a batch of an index with a center shadow is ranked and where its shadow scan's pair terms come from
//   0      the fp32 centers rank, shadow_pair_kernel computes t (the path before the center shadow)
//   1      (default) the fp16 center shadow ranks, the ranking's exact recheck hands t on
//   2      the fp16 center shadow ranks, shadow_pair_kernel computes t (tests: both routes of t on one ranking)
// Read at every batch: A/B runs on one build, and tests that compare the paths in one process tree
int rank_shadow_env() {
    const char *e = getenv("PGV_RANK_SHADOW");
    return e ? atoi(e) : 1;
}

// PGV_PROBE_PRUNE: 0 = every probed list is scanned, otherwise (default) a batch over the row shadow drops the probed
// lists that provably hold none of a query's k nearest rows (pgv_internal.h, beside ScanBound).  Read at every batch, like
// PGV_SCAN_SHADOW: one process compares both
bool probe_prune_on(const pgv_index *ix, int probes) {
    const char *e = getenv("PGV_PROBE_PRUNE");
    return (e ? atoi(e) != 0 : true) && ix->list_radius && probes <= probe_prune_max_probes();
}

// The fp16 residual shadow of an fp32 L2 index (kernels_shadow.hip; the bound: pgv_internal.h, ScanBound), built once
// with the index -- its rows never change afterwards.  Its own allocation (+50 % of the fp32 row bytes), outside the
// exportable arena; no device memory for it is no error: the list scan keeps the fp32 rows.  The same allocation holds
// the fp16 copy of the centers that the batch ranking multiplies: rows | 256 bytes of words | centers
int shadow_create(pgv_ctx *ctx, pgv_index *ix) {
    const int env = shadow_env();
    if (env == 0 || ix->metric != PGV_L2SQ || ix->dtype != PGV_F32 || ix->nrows <= 0 || !ix->row_norms || !ix->center_norms)
        return PGV_OK;
    if (env < 0 && !rows_stream_past_caches(ivf_rows(ix))) return PGV_OK;
    const RowGeom g16 = row_geom(ix->dim, PGV_F16);
    const size_t bytes = ((size_t)ix->nrows * g16.ld * sizeof(uint16_t) + 255) & ~(size_t)255;
    const size_t cbytes = ((size_t)ix->nlists * g16.ld * sizeof(uint16_t) + 255) & ~(size_t)255;
    // ... and behind them the lists' radii (probe pruning): the build's fp64 bits, then the fp32 values in their place
    const size_t rbytes = sizeof(unsigned long long) * (size_t)ix->nlists;
    void *sh = nullptr;
    if (hipMalloc(&sh, bytes + 256 + cbytes + rbytes) != hipSuccess) {
        (void)hipGetLastError();
        return PGV_OK;
    }
    // [0] max |x_i - c_i| | [8] E^2 | [16] P^2 of the rows; at byte 32 the same of the centers (max |c_i|, E_c^2, P_c^2)
    void *words = static_cast<char *>(sh) + bytes;
    void *csh = static_cast<char *>(sh) + bytes + 256;
    void *rad = static_cast<char *>(sh) + bytes + 256 + cbytes;
    int rc = launch_shadow_build(ctx, ix->geom, g16, ix->vectors, ix->centers, ix->list_offsets, ix->nlists, ix->nrows, sh,
                                 words, rad);
    if (rc == PGV_OK)
        rc = launch_shadow_build(ctx, ix->geom, g16, ix->centers, nullptr, nullptr, 0, ix->nlists, csh,
                                 static_cast<char *>(words) + 32);
    unsigned char h[56];
    if (rc == PGV_OK && (hipStreamSynchronize(ctx->stream) != hipSuccess ||
                         hipMemcpy(h, words, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)) {
        set_error("shadow build failed: %s", hipGetErrorString(hipGetLastError()));
        rc = PGV_ERR_DEVICE;
    }
    if (rc != PGV_OK) {
        (void)hipFree(sh);
        return rc;
    }
    float max_abs;
    double e2, p2;
    memcpy(&max_abs, h, 4);
    memcpy(&e2, h + 8, 8);
    memcpy(&p2, h + 16, 8);
    const double P = std::sqrt(p2), E = std::sqrt(e2);
    if (!std::isfinite(E) || !std::isfinite(P) || !std::isfinite(max_abs)) {  // NaN / inf rows: the fp32 scan
        (void)hipFree(sh);
        return PGV_OK;
    }
    // rounded up: the fp64 sums (relative 1e-9 covers them many times over) and rho itself in fp64 (x_i - c_i is
    // exact there unless the exponents lie ~30 apart: 1e-12 |rho| <= 1e-12 (P + E) covers that)
    ix->shadow = sh;
    ix->shadow_geom = g16;
    ix->shadow_s = shadow_scale_of(max_abs);
    ix->shadow_E = (E + 1e-12 * (P + E)) * (1.0 + 1e-9);
    ix->shadow_P = P * (1.0 + 1e-9);
    // the lists' radii: sqrt of the fp64 maxima, rounded up like E (x_i - c_i and the sum in fp64: 1e-9 covers them) and
    // once more into fp32; a non-finite one is +inf (its list is never dropped, and nothing behind it), an empty list 0.
    // A failed copy leaves the index without radii: nothing is pruned
    {
        std::vector<unsigned long long> rb((size_t)ix->nlists);
        std::vector<float> rf((size_t)ix->nlists);
        if (hipMemcpy(rb.data(), rad, rbytes, hipMemcpyDeviceToHost) == hipSuccess) {
            for (int l = 0; l < ix->nlists; l++) {
                double r2;
                memcpy(&r2, &rb[l], 8);
                const double R = std::sqrt(r2) * (1.0 + 1e-9);
                float f = (float)R;
                if (std::isfinite(f) && (double)f < R) f = std::nextafterf(f, INFINITY);
                rf[l] = std::isfinite(R) ? f : INFINITY;
            }
            if (hipMemcpy(rad, rf.data(), sizeof(float) * rf.size(), hipMemcpyHostToDevice) == hipSuccess)
                ix->list_radius = static_cast<float *>(rad);
        }
        (void)hipGetLastError();
    }
    // the centers' copy, rounded up the same way; a non-finite E_c or P_c (NaN / inf in a center) drops it alone: the
    // ranking stays on the fp32 centers
    float cmax_abs;
    double ce2, cp2;
    memcpy(&cmax_abs, h + 32, 4);
    memcpy(&ce2, h + 40, 8);
    memcpy(&cp2, h + 48, 8);
    const double Pc = std::sqrt(cp2), Ec = std::sqrt(ce2);
    if (std::isfinite(Ec) && std::isfinite(Pc) && std::isfinite(cmax_abs)) {
        ix->cshadow = csh;
        ix->cshadow_s = shadow_scale_of(cmax_abs);
        ix->cshadow_E = (Ec + 1e-12 * (Pc + Ec)) * (1.0 + 1e-9);
        ix->cshadow_P = Pc * (1.0 + 1e-9);
    }
    return PGV_OK;
}

// What the shadow paths of ONE batch share (ctx->sh_q): shadow_query_kernel runs once, ahead of the ranking, and serves
// the ranking over the center shadow and the list scan over the row shadow; the ranking's recheck leaves the probed
// pairs' t = -2 q.c_l for the scan's plan.  pgv_search_batch passes one through both halves; a half that gets none
// (pgv_rank_lists, pgv_scan_batch, the sharded search) prepares what it needs itself.
struct ShadowBatch {
    void *qcast = nullptr;                     // [nq x g16.ld] fp16 queries
    float *qscale = nullptr, *qeps = nullptr;  // the list scan's factors 2^(1 + s + s_q) and band terms
    float *cscale = nullptr, *ceps = nullptr;  // the ranking's 2^(1 + s_c + s_q) and band terms
    float *pair_t = nullptr;                   // [nq x probes]
    bool scan_follows = false;                 // set by the caller: the shadow scan will run on the ranking's lists
    int need = 0;                              // ... for heads of this many rows (the search's k: probe pruning)
    bool cast_for_scan = false;                // qscale / qeps are written
    // the ranking left pair_t, cleared the plan's counters and counted the lists it emitted into them (PlanEmit)
    bool pairs_done = false;
};

int shadow_batch_cast(pgv_index *ix, const void *q_dev, int nq, int probes, bool for_rank, bool for_scan, ShadowBatch *sb) {
    pgv_ctx *ctx = ix->ctx;
    const RowGeom &g16 = ix->shadow_geom;
    const size_t qb = ((size_t)nq * g16.ld * sizeof(uint16_t) + 255) & ~(size_t)255;
    PGV_TRY(ctx->sh_q.ensure(qb + sizeof(float) * (size_t)nq * (4 + (size_t)probes)));
    sb->qcast = ctx->sh_q.p;
    sb->qscale = reinterpret_cast<float *>(ctx->sh_q.as<char>() + qb);
    sb->qeps = sb->qscale + nq;
    sb->cscale = sb->qeps + nq;
    sb->ceps = sb->cscale + nq;
    sb->pair_t = sb->ceps + nq;
    constexpr double u = 5.9604644775390625e-8;  // 2^-24
    ShadowTerms st{};
    st.s = ix->shadow_s;
    st.E = ix->shadow_E;
    st.P = ix->shadow_P;
    st.g_dot = gamma_n(shadow_chain_length(g16) + 4.0, u);
    st.g_pair = gamma_n((double)pair_chain_length(ix->geom), u);
    st.g_cn = shadow_band(ix->geom.ld, 0.f, u).g_norm;
    RankShadowTerms rt{};
    rt.s = ix->cshadow_s;
    rt.E = ix->cshadow_E;
    rt.P = ix->cshadow_P;
    rt.g_dot = st.g_dot;  // (dense_scan's tasks take the 32-query and 16-wide forms: shadow_chain_length covers both)
    rt.g_cn = st.g_cn;
    PGV_TRY(launch_shadow_query(ctx, ix->geom, g16, q_dev, nq, st, rt, ix->center_norms + ix->nlists,
                                ix->row_norms + ix->nrows, sb->qcast, for_scan ? sb->qscale : nullptr,
                                for_scan ? sb->qeps : nullptr, for_rank ? sb->cscale : nullptr,
                                for_rank ? sb->ceps : nullptr));
    sb->cast_for_scan = for_scan;
    return PGV_OK;
}

// What a mirror's rows are made of, as the upload entries state it: dim elements of dtype under metric, or nbits bits
// (pgv_index_upload_bits; metric / dtype are unused there, and PGV_L1 keeps every L2-only structure away from it)
struct IndexElem {
    pgv_metric metric;
    pgv_dtype dtype;
    int dim, nbits;
    static IndexElem bits(int nbits) { return {PGV_L1, PGV_F32, nbits, nbits}; }
    size_t tight_bytes() const { return nbits > 0 ? (size_t)(nbits + 7) / 8 : (size_t)dim * elem_size(dtype); }  // VARBITBYTES
};

// The mirror of an index whose list offsets are known: one allocation, host tables, the norms the MFMA paths want.
// `fill` enqueues (on ctx->stream) whatever brings centers / vectors / tids into the carved arrays.
// A bit index has rows of bit_row_geom(nbits).ld bytes, no norms and no shadow
template <typename Fill>
int index_create(pgv_ctx *ctx, const IndexElem &el, int nlists, const std::vector<int64_t> &off, bool has_tids, Fill fill,
                 pgv_index **out) {
    const pgv_metric metric = el.metric;
    const int nbits = el.nbits;
    const int64_t n = off[nlists];
    pgv_index *ix = new (std::nothrow) pgv_index();
    if (!ix) PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    ix->ctx = ctx;
    ix->refs = new (std::nothrow) int(1);
    if (!ix->refs) {
        delete ix;
        PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    }
    ix->metric = metric;
    ix->dtype = el.dtype;
    ix->dim = el.dim;
    ix->nlists = nlists;
    ix->nrows = n;
    ix->nbits = nbits;
    ix->geom = nbits > 0 ? bit_row_geom(nbits) : row_geom(el.dim, el.dtype);
    ix->h_offsets = off;
    index_host_tables(ix);

    auto fail = [&](int rc) {
        pgv_index_free(ix);
        return rc;
    };
    // one allocation for the whole mirror (a single IPC handle exports it): centers | vectors | list_offsets |
    // tids | row_norms | center_norms, each part 256-byte aligned
    IndexLayout lay = index_layout(nlists, n, ivf_rows(ix).row_bytes(), has_tids && n > 0, metric == PGV_L2SQ && nbits == 0);
    if (malloc_exportable(&ix->arena, lay.bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("hipMalloc(%zu) for the index mirror failed", lay.bytes);
        return fail(PGV_ERR_NOMEM);
    }
    ix->arena_bytes = lay.bytes;
    index_carve(ix, lay);
    int rc;
    if ((rc = fill(ix)) != PGV_OK) return fail(rc);
    if (hipMemcpyAsync(ix->list_offsets, ix->h_offsets.data(), sizeof(int64_t) * off.size(),
                       hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return fail((set_error("copy of list_offsets failed"), PGV_ERR_DEVICE));
    if (ix->row_norms) {
        // |x|^2 per row and the largest of them: the MFMA scan's expansion of the L2 distance
        if (hipMemsetAsync(ix->row_norms + n, 0, sizeof(float), ctx->stream) != hipSuccess)
            return fail((set_error("memset of row_norms failed"), PGV_ERR_DEVICE));
        if ((rc = launch_row_norms(ctx, ivf_rows(ix), ix->row_norms, reinterpret_cast<unsigned *>(ix->row_norms + n))) != PGV_OK)
            return fail(rc);
    }
    if (ix->center_norms) {
        if (hipMemsetAsync(ix->center_norms + nlists, 0, sizeof(float), ctx->stream) != hipSuccess)
            return fail((set_error("memset of center_norms failed"), PGV_ERR_DEVICE));
        if ((rc = launch_row_norms(ctx, ivf_centers(ix), ix->center_norms,
                                   reinterpret_cast<unsigned *>(ix->center_norms + nlists))) != PGV_OK)
            return fail(rc);
    }
    if (nbits == 0 && (rc = shadow_create(ctx, ix)) != PGV_OK) return fail(rc);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess)
        return fail((set_error("index upload failed: %s", hipGetErrorString(hipGetLastError())), PGV_ERR_DEVICE));
    *out = ix;
    return PGV_OK;
}

// What pgv_index_upload and pgv_index_upload_bits share once their own arguments are checked: the offsets read and
// validated, then the mirror with centers, rows and tids copied in
int index_upload(pgv_ctx *ctx, const IndexElem &el, int nlists, const void *centers, const int64_t *list_offsets,
                 const void *rows, const char *rows_name, const uint64_t *tids, pgv_index **out) {
    // IVFFLAT_MAX_LISTS (src/ivfflat.h:56)
    if (nlists < 1 || nlists > 32768) PGV_FAIL(PGV_ERR_ARG, "lists %d outside 1..32768", nlists);
    if (!centers || !list_offsets) PGV_FAIL(PGV_ERR_ARG, "centers/list_offsets is NULL");
    PGV_HIP(hipSetDevice(ctx->device));
    std::vector<int64_t> off((size_t)nlists + 1);
    if (is_device_ptr(list_offsets)) {
        PGV_HIP(hipMemcpy(off.data(), list_offsets, sizeof(int64_t) * off.size(), hipMemcpyDeviceToHost));
    } else {
        memcpy(off.data(), list_offsets, sizeof(int64_t) * off.size());
    }
    if (off[0] != 0) PGV_FAIL(PGV_ERR_ARG, "list_offsets[0] must be 0");
    for (int l = 0; l < nlists; l++)
        if (off[l + 1] < off[l]) PGV_FAIL(PGV_ERR_ARG, "list_offsets not ascending at list %d", l);
    const int64_t n = off[nlists];
    if (n > 0 && !rows) PGV_FAIL(PGV_ERR_ARG, "%s is NULL", rows_name);
    return index_create(ctx, el, nlists, off, tids != nullptr, [&](pgv_index *ix) -> int {
        const size_t padded = ivf_rows(ix).row_bytes();
        PGV_TRY(put_padded_rows(ctx->stream, ix->centers, padded, centers, el.tight_bytes(), nlists));
        PGV_TRY(put_padded_rows(ctx->stream, ix->vectors, padded, rows, el.tight_bytes(), n));
        if (ix->tids)
            PGV_HIP(hipMemcpyAsync(ix->tids, tids, sizeof(uint64_t) * (size_t)n,
                                   is_device_ptr(tids) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
        return PGV_OK;
    }, out);
}

}  // namespace
}  // extern "C++"

int pgv_index_upload(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, int dim, int nlists,
                     const void *centers, const int64_t *list_offsets, const void *vectors,
                     const uint64_t *tids, pgv_index **out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_index_upload: ctx/out is NULL");
    *out = nullptr;
    PGV_TRY(check_common(dtype, dim));
    PGV_TRY(check_metric(metric));
    return index_upload(ctx, IndexElem{metric, dtype, dim, 0}, nlists, centers, list_offsets, vectors, "vectors", tids, out);
}

// `USING ivfflat (col bit_hamming_ops)` (sql/vector.sql:894-899; the bit type info of src/ivfutils.c:411-424): the mirror
// of pgv_index_upload with packed bit strings for centers and rows.  The element type is recorded as pgv_index::nbits
int pgv_index_upload_bits(pgv_ctx *ctx, int nbits, int nlists, const void *centers, const int64_t *list_offsets,
                          const void *rows, const uint64_t *tids, pgv_index **out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_index_upload_bits: ctx/out is NULL");
    *out = nullptr;
    // IVFFLAT_MAX_DIM * 32 (src/ivfutils.c:416)
    if (nbits < 1 || nbits > kIvfMaxBits) PGV_FAIL(PGV_ERR_DIMS, "bit length %d outside 1..%d", nbits, kIvfMaxBits);
    return index_upload(ctx, IndexElem::bits(nbits), nlists, centers, list_offsets, rows, "rows", tids, out);
}

int pgv_index_nbits(const pgv_index *ix) { return ix ? ix->nbits : -1; }

// the entries that do not serve a bit index (include/pgv_hip.h): refused before anything is launched
#define PGV_NO_BIT_INDEX(ix, who)                                                                                 \
    do {                                                                                                          \
        if ((ix)->nbits > 0) PGV_FAIL(PGV_ERR_ARG, "%s: not served on a bit index (pgv_index_upload_bits)", who); \
    } while (0)

// the queries of an index in its rows' layout; of a bit index: [nq x VARBITBYTES] bit strings into whole register slices
// of the Hamming kernels (bit_query_bytes)
static int stage_queries(pgv_index *ix, const void *queries, int nq, const void **q_dev) {
    if (ix->nbits > 0)
        return stage_rows(ix->ctx, queries, nq, (size_t)(ix->nbits + 7) / 8, (size_t)bit_query_bytes(ix->nbits), ix->ctx->q_stage,
                          q_dev);
    return stage_rows(ix->ctx, queries, nq, ix->dim, ix->dtype, ix->geom, ix->ctx->q_stage, q_dev);
}

// ------------------------------------------------------------ the build's tuplesort on the device
struct pgv_builder {
    pgv_ctx *ctx = nullptr;
    pgv_metric metric = PGV_L2SQ;
    pgv_dtype dtype = PGV_F32;
    int dim = 0, nlists = 0;
    RowGeom geom{};
    DBuf centers;  // [nlists x ld]
    DBuf rows;     // [cap x ld] heap order
    DBuf tids;     // [cap]
    DBuf lists;    // [cap] int32
    int64_t n = 0, cap = 0;
    int64_t assigned = 0;  // rows [0, assigned) have their list id
    bool has_tids = true;
    // centers not known yet (pgv_builder_begin with centers == NULL): rows are only copied, on a stream of the
    // builder's own, so that the k-means which is still computing the centers on the context's stream (from another
    // host thread) and the upload of the heap overlap; pgv_builder_set_centers ends this state
    bool deferred = false;
    hipStream_t copy_stream = nullptr;
    hipStream_t stream() const { return deferred ? copy_stream : ctx->stream; }
    // the heap-order rows as the kernels take them; centers and rows share its row_bytes()
    RowsView view() const { return {rows.p, n, geom, row_kind(dtype), metric}; }
    size_t row_bytes() const { return view().row_bytes(); }
    // tightly packed rows or centers (host or device) into padded ones at dst
    int put(hipStream_t to, void *dst, const void *src, int64_t cnt) const {
        return put_padded_rows(to, dst, row_bytes(), src, (size_t)dim * elem_size(dtype), cnt);
    }
};

static int builder_reserve(pgv_builder *b, int64_t want) {
    if (want <= b->cap) return PGV_OK;
    int64_t cap = b->cap ? b->cap + b->cap / 2 : want;
    if (cap < want) cap = want;
    const size_t row_bytes = b->row_bytes();
    DBuf rows, tids, lists;
    PGV_TRY(rows.ensure(row_bytes * (size_t)cap));
    int rc = tids.ensure(sizeof(uint64_t) * (size_t)cap);
    if (rc == PGV_OK) rc = lists.ensure(sizeof(int32_t) * (size_t)cap);
    if (rc == PGV_OK && b->n > 0) {
        hipError_t e = hipMemcpyAsync(rows.p, b->rows.p, row_bytes * (size_t)b->n, hipMemcpyDeviceToDevice, b->stream());
        if (e == hipSuccess) e = hipMemcpyAsync(tids.p, b->tids.p, sizeof(uint64_t) * (size_t)b->n, hipMemcpyDeviceToDevice, b->stream());
        if (e == hipSuccess) e = hipMemcpyAsync(lists.p, b->lists.p, sizeof(int32_t) * (size_t)b->n, hipMemcpyDeviceToDevice, b->stream());
        if (e == hipSuccess) e = hipStreamSynchronize(b->stream());
        if (e != hipSuccess) {
            set_error("growing the builder failed: %s", hipGetErrorString(e));
            rc = PGV_ERR_DEVICE;
        }
    }
    if (rc != PGV_OK) {
        rows.release();
        tids.release();
        lists.release();
        return rc;
    }
    b->rows.release();
    b->tids.release();
    b->lists.release();
    b->rows = rows;
    b->tids = tids;
    b->lists = lists;
    b->cap = cap;
    return PGV_OK;
}

// rows [assigned, n) to their nearest center
static int builder_assign_pending(pgv_builder *b) {
    if (b->assigned >= b->n) return PGV_OK;
    PGV_TRY(launch_argmin(b->ctx, b->metric, b->dtype, b->geom, b->rows.as<char>() + (size_t)b->assigned * b->row_bytes(),
                          b->n - b->assigned, b->centers.p, b->nlists, b->lists.as<int32_t>() + b->assigned, nullptr));
    b->assigned = b->n;
    return PGV_OK;
}

int pgv_builder_begin(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, int dim, int nlists, const void *centers,
                      int64_t expected_rows, pgv_builder **out) {
    if (!ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_builder_begin: ctx/out is NULL");
    *out = nullptr;
    PGV_TRY(check_common(dtype, dim));
    PGV_TRY(check_metric(metric));
    if (nlists < 1 || nlists > 32768) PGV_FAIL(PGV_ERR_ARG, "lists %d outside 1..32768", nlists);
    if (expected_rows < 0) PGV_FAIL(PGV_ERR_ARG, "expected_rows < 0");
    PGV_HIP(hipSetDevice(ctx->device));
    pgv_builder *b = new (std::nothrow) pgv_builder();
    if (!b) PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    b->ctx = ctx;
    b->metric = metric;
    b->dtype = dtype;
    b->dim = dim;
    b->nlists = nlists;
    b->geom = row_geom(dim, dtype);
    int rc = b->centers.ensure(b->row_bytes() * (size_t)nlists);
    if (rc == PGV_OK && centers) {
        rc = b->put(ctx->stream, b->centers.p, centers, nlists);
        if (rc == PGV_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = PGV_ERR_DEVICE;  // the caller may reuse centers
    } else if (rc == PGV_OK) {
        b->deferred = true;
        if (hipStreamCreateWithFlags(&b->copy_stream, hipStreamNonBlocking) != hipSuccess) {
            set_error("pgv_builder_begin: no stream for the upload");
            rc = PGV_ERR_DEVICE;
        }
    }
    if (rc == PGV_OK && expected_rows > 0) rc = builder_reserve(b, expected_rows);
    if (rc != PGV_OK) {
        pgv_builder_free(b);
        return rc;
    }
    *out = b;
    return PGV_OK;
}

void pgv_builder_free(pgv_builder *b) {
    if (!b) return;
    if (b->copy_stream) {
        (void)hipStreamSynchronize(b->copy_stream);
        (void)hipStreamDestroy(b->copy_stream);
    }
    if (b->ctx) (void)hipStreamSynchronize(b->ctx->stream);
    b->centers.release();
    b->rows.release();
    b->tids.release();
    b->lists.release();
    delete b;
}

int64_t pgv_builder_rows(const pgv_builder *b) { return b ? b->n : -1; }

int pgv_builder_add(pgv_builder *b, const void *rows, const uint64_t *tids, int64_t n) {
    if (!b) PGV_FAIL(PGV_ERR_ARG, "pgv_builder_add: builder is NULL");
    if (n < 0) PGV_FAIL(PGV_ERR_ARG, "n < 0");
    if (n == 0) return PGV_OK;
    if (!rows) PGV_FAIL(PGV_ERR_ARG, "rows is NULL");
    if (b->n + n > 0xffffffffll) PGV_FAIL(PGV_ERR_ARG, "pgv_builder_add: more than 2^32 rows");
    if (b->n > 0 && (tids != nullptr) != b->has_tids) PGV_FAIL(PGV_ERR_ARG, "pgv_builder_add: tids given for some batches only");
    pgv_ctx *ctx = b->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_TRY(builder_reserve(b, b->n + n));
    b->has_tids = tids != nullptr;
    hipStream_t stream = b->stream();
    PGV_TRY(b->put(stream, b->rows.as<char>() + (size_t)b->n * b->row_bytes(), rows, n));
    if (tids)
        PGV_HIP(hipMemcpyAsync(b->tids.as<uint64_t>() + b->n, tids, sizeof(uint64_t) * (size_t)n,
                               is_device_ptr(tids) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    b->n += n;
    // AddTupleToSort's argmin (src/ivfbuild.c:183-192) for this batch (and what an earlier centerless phase left),
    // where the rows now are
    if (!b->deferred) PGV_TRY(builder_assign_pending(b));
    // host buffers may be reused by the caller right away; device rows must have arrived before the caller's stream
    // moves on
    if (b->deferred || !is_device_ptr(rows) || (tids && !is_device_ptr(tids))) PGV_HIP(hipStreamSynchronize(stream));
    return PGV_OK;
}

int pgv_builder_set_centers(pgv_builder *b, const void *centers) {
    if (!b || !centers) PGV_FAIL(PGV_ERR_ARG, "pgv_builder_set_centers: builder/centers is NULL");
    if (!b->deferred) PGV_FAIL(PGV_ERR_STATE, "pgv_builder_set_centers: the builder has its centers");
    pgv_ctx *ctx = b->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_HIP(hipStreamSynchronize(b->copy_stream));  // every row has arrived; from here on the context's stream is used
    b->deferred = false;
    PGV_TRY(b->put(ctx->stream, b->centers.p, centers, b->nlists));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    return PGV_OK;
}

int pgv_builder_finish(pgv_builder *b, pgv_index **out_index, int64_t *out_offsets, int32_t *out_lists) {
    if (!b || !out_index) PGV_FAIL(PGV_ERR_ARG, "pgv_builder_finish: builder/out_index is NULL");
    *out_index = nullptr;
    pgv_ctx *ctx = b->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    if (b->deferred) PGV_FAIL(PGV_ERR_STATE, "pgv_builder_finish: no centers (pgv_builder_set_centers)");
    PGV_TRY(builder_assign_pending(b));
    const int64_t n = b->n;
    const int nlists = b->nlists;
    int list_bits = 1;
    while ((1 << list_bits) < nlists) list_bits++;
    const size_t sort_bytes = n > 0 ? build_sort_scratch_bytes(n, 32 + list_bits) : 0;
    // scratch: keys_tmp | keys_sorted | counts | offsets | bad | sort scratch
    const size_t kb = sizeof(unsigned long long) * (size_t)(n > 0 ? n : 1), cb = sizeof(unsigned long long) * (size_t)nlists,
                 ob = sizeof(int64_t) * ((size_t)nlists + 1);
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_sorted = up(kb), o_counts = o_sorted + up(kb), o_off = o_counts + up(cb), o_bad = o_off + up(ob),
                 o_sort = o_bad + 256;
    DBuf scratch;
    PGV_TRY(scratch.ensure(o_sort + sort_bytes + 256));
    char *sp = scratch.as<char>();
    auto *keys_tmp = reinterpret_cast<unsigned long long *>(sp);
    auto *keys_sorted = reinterpret_cast<unsigned long long *>(sp + o_sorted);
    auto *counts = reinterpret_cast<unsigned long long *>(sp + o_counts);
    auto *offsets_dev = reinterpret_cast<int64_t *>(sp + o_off);
    int *bad = reinterpret_cast<int *>(sp + o_bad);
    int rc = launch_build_order(ctx, b->lists.as<int32_t>(), n, nlists, keys_tmp, keys_sorted, counts, offsets_dev, bad,
                                sp + o_sort, sort_bytes);
    std::vector<int64_t> off((size_t)nlists + 1);
    int bad_h = 0;
    if (rc == PGV_OK) {
        hipError_t e = hipMemcpyAsync(off.data(), offsets_dev, ob, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && out_lists && n > 0)
            e = hipMemcpyAsync(out_lists, b->lists.p, sizeof(int32_t) * (size_t)n,
                               is_device_ptr(out_lists) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            set_error("pgv_builder_finish: %s", hipGetErrorString(e));
            rc = PGV_ERR_DEVICE;
        }
    }
    if (rc == PGV_OK && (bad_h || off[nlists] != n)) {
        set_error("pgv_builder_finish: assignment produced a list id outside 0..%d", nlists - 1);
        rc = PGV_ERR_STATE;
    }
    if (rc == PGV_OK)
        rc = index_create(ctx, IndexElem{b->metric, b->dtype, b->dim, 0}, nlists, off, true, [&](pgv_index *ix) -> int {
            PGV_HIP(hipMemcpyAsync(ix->centers, b->centers.p, b->row_bytes() * (size_t)nlists, hipMemcpyDeviceToDevice,
                                   ctx->stream));
            // rows and heap TIDs (heap positions when none were given) into list-major order, heap order inside a list
            return launch_build_gather(ctx, b->rows.p, keys_sorted, n, b->geom.nvec, ix->vectors,
                                       b->has_tids ? b->tids.as<uint64_t>() : nullptr, ix->tids);
        }, out_index);
    scratch.release();
    if (rc != PGV_OK) return rc;
    if (out_offsets) memcpy(out_offsets, off.data(), ob);
    // the heap-order copy has served
    b->rows.release();
    b->tids.release();
    b->lists.release();
    b->n = b->cap = b->assigned = 0;
    return PGV_OK;
}

// the mirror's rows, list-major, back to the host in pieces: double-buffered D2H into pinned memory, the sink called
// for piece i while piece i + 1 is on its way
int pgv_index_drain(pgv_index *ix, int64_t chunk_rows, pgv_rows_sink sink, void *arg) {
    if (!ix || !sink) PGV_FAIL(PGV_ERR_ARG, "pgv_index_drain: index/sink is NULL");
    PGV_NO_BIT_INDEX(ix, "pgv_index_drain");
    pgv_ctx *ctx = ix->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    const int64_t n = ix->nrows;
    if (n == 0) return PGV_OK;
    const size_t tight = (size_t)ix->dim * elem_size(ix->dtype), padded = ivf_rows(ix).row_bytes();
    // 64 MB pieces: long enough for the link's full rate, short enough that pinning the two bounce buffers (which
    // costs ~30 ms at 2 x 256 MB) does not show
    if (chunk_rows <= 0) chunk_rows = (int64_t)std::max<size_t>(1, ((size_t)64 << 20) / tight);
    if (chunk_rows > n) chunk_rows = n;
    void *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    const size_t piece = tight * (size_t)chunk_rows + sizeof(uint64_t) * (size_t)chunk_rows;
    int rc = PGV_OK;
    for (int i = 0; i < 2 && rc == PGV_OK; i++) {
        if (hipHostMalloc(&buf[i], piece, hipHostMallocDefault) != hipSuccess) rc = PGV_ERR_NOMEM;
        if (rc == PGV_OK && hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) rc = PGV_ERR_DEVICE;
    }
    auto issue = [&](int64_t c, int slot) -> int {
        const int64_t r0 = c * chunk_rows, cnt = std::min(chunk_rows, n - r0);
        char *dst = static_cast<char *>(buf[slot]);
        const char *src = static_cast<const char *>(ix->vectors) + (size_t)r0 * padded;
        if (padded == tight)
            PGV_HIP(hipMemcpyAsync(dst, src, tight * (size_t)cnt, hipMemcpyDeviceToHost, ctx->stream));
        else
            PGV_HIP(hipMemcpy2DAsync(dst, tight, src, padded, tight, (size_t)cnt, hipMemcpyDeviceToHost, ctx->stream));
        if (ix->tids)
            PGV_HIP(hipMemcpyAsync(dst + tight * (size_t)chunk_rows, ix->tids + r0, sizeof(uint64_t) * (size_t)cnt,
                                   hipMemcpyDeviceToHost, ctx->stream));
        PGV_HIP(hipEventRecord(ev[slot], ctx->stream));
        return PGV_OK;
    };
    const int64_t nchunks = (n + chunk_rows - 1) / chunk_rows;
    if (rc == PGV_OK) rc = issue(0, 0);
    for (int64_t c = 0; c < nchunks && rc == PGV_OK; c++) {
        const int slot = (int)(c & 1);
        if (c + 1 < nchunks) rc = issue(c + 1, slot ^ 1);
        if (rc != PGV_OK) break;
        if (hipEventSynchronize(ev[slot]) != hipSuccess) {
            set_error("pgv_index_drain: copy failed");
            rc = PGV_ERR_DEVICE;
            break;
        }
        const int64_t r0 = c * chunk_rows, cnt = std::min(chunk_rows, n - r0);
        const char *p = static_cast<const char *>(buf[slot]);
        const int src = sink(arg, r0, cnt, p, ix->tids ? reinterpret_cast<const uint64_t *>(p + tight * (size_t)chunk_rows) : nullptr);
        if (src != 0) {
            set_error("pgv_index_drain: the sink returned %d", src);
            rc = PGV_ERR_STATE;
        }
    }
    (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < 2; i++) {
        if (ev[i]) (void)hipEventDestroy(ev[i]);
        if (buf[i]) (void)hipHostFree(buf[i]);
    }
    if (rc == PGV_ERR_NOMEM) set_error("pgv_index_drain: pinned buffers (2 x %zu bytes) could not be allocated", piece);
    return rc;
}

static void index_drop_lanes(pgv_index *ix);

int pgv_index_set_overlap(pgv_index *ix, int lanes) {
    if (!ix) PGV_FAIL(PGV_ERR_ARG, "pgv_index_set_overlap: index is NULL");
    PGV_NO_BIT_INDEX(ix, "pgv_index_set_overlap");
    if (lanes < 1 || lanes > 4) PGV_FAIL(PGV_ERR_ARG, "pgv_index_set_overlap: lanes %d outside 1..4", lanes);
    PGV_HIP(hipSetDevice(ix->ctx->device));
    PGV_TRY(pgv_ctx_sync(ix->ctx));
    index_drop_lanes(ix);
    if (lanes == 1) return PGV_OK;
    PGV_HIP(hipEventCreateWithFlags(&ix->lane_event, hipEventDisableTiming));
    PGV_HIP(hipEventCreateWithFlags(&ix->lane_scan_done, hipEventDisableTiming));
    for (int i = 0; i < lanes; i++) {
        pgv_ctx *lc = nullptr;
        pgv_index *v = nullptr;
        int rc = pgv_ctx_create(ix->ctx->device, nullptr, &lc);
        if (rc == PGV_OK) rc = pgv_index_share(ix, lc, &v);
        if (rc != PGV_OK) {
            if (lc) pgv_ctx_destroy(lc);
            index_drop_lanes(ix);
            return rc;
        }
        lc->no_mfma_scan = ix->ctx->no_mfma_scan;
        lc->bound_mode = ix->ctx->bound_mode;
        lc->assign_bound_mode = ix->ctx->assign_bound_mode;
        if (ix->ctx->profiling) (void)pgv_ctx_set_profiling(lc, 1);
        lc->scan_gate = ix->lane_scan_done;
        ix->lanes.push_back(v);
        ix->ctx->children.push_back(lc);
    }
    return PGV_OK;
}

int pgv_index_share(pgv_index *ix, pgv_ctx *ctx, pgv_index **out) {
    if (!ix || !ctx || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_index_share: index/ctx/out is NULL");
    *out = nullptr;
    if (ctx->device != ix->ctx->device)
        PGV_FAIL(PGV_ERR_ARG, "pgv_index_share: the index lives on device %d, the context on %d", ix->ctx->device, ctx->device);
    pgv_index *v = new (std::nothrow) pgv_index(*ix);  // same device arrays, host tables copied
    if (!v) PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    v->ctx = ctx;
    v->lanes.clear();  // (the lanes of overlapping batches belong to the handle they were set on)
    v->lane_next = 0;
    v->lane_event = nullptr;
    v->lane_scan_done = nullptr;
    __atomic_add_fetch(ix->refs, 1, __ATOMIC_RELAXED);
    *out = v;
    return PGV_OK;
}

// What crosses the process boundary: the shape of the mirror and the IPC handle of its one allocation.
struct IndexHandleWire {
    uint64_t magic;
    uint32_t abi, pid;
    int32_t device, metric, dtype, dim, nlists, has_tids;
    int64_t nrows;
    uint64_t arena_bytes;
    hipIpcMemHandle_t mem;
};
static_assert(sizeof(IndexHandleWire) <= PGV_INDEX_HANDLE_BYTES, "pgv_index_handle too small");
static constexpr uint64_t kIndexHandleMagic = 0x7067765f69786831ull;  // "pgv_ixh1"

int pgv_index_export(pgv_index *ix, pgv_index_handle *out) {
    if (!ix || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_index_export: index/out is NULL");
    PGV_NO_BIT_INDEX(ix, "pgv_index_export");
    if (!ix->arena) PGV_FAIL(PGV_ERR_STATE, "pgv_index_export: the index has no device arrays");
    if (ix->imported) PGV_FAIL(PGV_ERR_STATE, "pgv_index_export: export from the process that uploaded the index");
    PGV_HIP(hipSetDevice(ix->ctx->device));
    IndexHandleWire w;
    memset(&w, 0, sizeof(w));
    w.magic = kIndexHandleMagic;
    w.abi = PGV_ABI_VERSION;
    w.pid = (uint32_t)getpid();
    w.device = ix->ctx->device;
    w.metric = ix->metric;
    w.dtype = ix->dtype;
    w.dim = ix->dim;
    w.nlists = ix->nlists;
    w.has_tids = ix->tids != nullptr;
    w.nrows = ix->nrows;
    w.arena_bytes = ix->arena_bytes;
    hipError_t e = hipIpcGetMemHandle(&w.mem, ix->arena);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        PGV_FAIL(PGV_ERR_DEVICE,
                 "hipIpcGetMemHandle failed: %s (the driver here shares memory by dmabuf: HSA_ENABLE_IPC_MODE_LEGACY=0 "
                 "must be in the environment of every process)", hipGetErrorString(e));
    }
    memset(out, 0, sizeof(*out));
    memcpy(out->bytes, &w, sizeof(w));
    return PGV_OK;
}

int pgv_index_import(pgv_ctx *ctx, const pgv_index_handle *handle, pgv_index **out) {
    if (!ctx || !handle || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_index_import: ctx/handle/out is NULL");
    *out = nullptr;
    IndexHandleWire w;
    memcpy(&w, handle->bytes, sizeof(w));
    if (w.magic != kIndexHandleMagic || w.abi != PGV_ABI_VERSION)
        PGV_FAIL(PGV_ERR_ARG, "pgv_index_import: not a handle of this library version");
    if (w.pid == (uint32_t)getpid())
        PGV_FAIL(PGV_ERR_STATE, "pgv_index_import: the handle was exported by this process (use pgv_index_share)");
    if (w.device != ctx->device)
        PGV_FAIL(PGV_ERR_ARG, "pgv_index_import: the index lives on device %d, the context on %d", w.device, ctx->device);
    PGV_TRY(check_common((pgv_dtype)w.dtype, w.dim));
    PGV_TRY(check_metric((pgv_metric)w.metric));
    if (w.nlists < 1 || w.nlists > 32768 || w.nrows < 0) PGV_FAIL(PGV_ERR_ARG, "pgv_index_import: corrupt handle");
    PGV_HIP(hipSetDevice(ctx->device));
    pgv_index *ix = new (std::nothrow) pgv_index();
    if (!ix) PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    ix->refs = new (std::nothrow) int(1);
    if (!ix->refs) {
        delete ix;
        PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    }
    ix->ctx = ctx;
    ix->metric = (pgv_metric)w.metric;
    ix->dtype = (pgv_dtype)w.dtype;
    ix->dim = w.dim;
    ix->nlists = w.nlists;
    ix->nrows = w.nrows;
    ix->geom = row_geom(w.dim, ix->dtype);
    ix->imported = true;
    IndexLayout lay = index_layout(w.nlists, w.nrows, ivf_rows(ix).row_bytes(), w.has_tids != 0, ix->metric == PGV_L2SQ);
    if (lay.bytes != w.arena_bytes) {
        pgv_index_free(ix);
        PGV_FAIL(PGV_ERR_ARG, "pgv_index_import: handle describes %llu bytes, this library lays the mirror out in %zu",
                 (unsigned long long)w.arena_bytes, lay.bytes);
    }
    hipError_t e = hipIpcOpenMemHandle(&ix->arena, w.mem, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ix->arena = nullptr;
        pgv_index_free(ix);
        PGV_FAIL(PGV_ERR_DEVICE, "hipIpcOpenMemHandle failed: %s (is the exporting process alive, and "
                 "HSA_ENABLE_IPC_MODE_LEGACY=0 set in both?)", hipGetErrorString(e));
    }
    ix->arena_bytes = lay.bytes;
    index_carve(ix, lay);
    // the host-side tables come from the mirror itself
    ix->h_offsets.assign((size_t)w.nlists + 1, 0);
    if (hipMemcpy(ix->h_offsets.data(), ix->list_offsets, sizeof(int64_t) * ix->h_offsets.size(),
                  hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("pgv_index_import: reading list_offsets failed: %s", hipGetErrorString(hipGetLastError()));
        pgv_index_free(ix);
        return PGV_ERR_DEVICE;
    }
    if (ix->h_offsets[0] != 0 || ix->h_offsets[w.nlists] != w.nrows) {
        pgv_index_free(ix);
        PGV_FAIL(PGV_ERR_DATA, "pgv_index_import: the shared mirror does not match its handle");
    }
    index_host_tables(ix);
    *out = ix;
    return PGV_OK;
}

// the device arrays go with the last handle on them (the uploaded index or a pgv_index_share view); an imported
// mirror is unmapped from this process, the exporter's allocation stays
static void index_drop_lanes(pgv_index *ix) {
    for (pgv_index *v : ix->lanes) {
        pgv_ctx *lc = v->ctx;
        if (ix->ctx) {
            auto &ch = ix->ctx->children;
            ch.erase(std::remove(ch.begin(), ch.end(), lc), ch.end());
        }
        pgv_index_free(v);  // (a view: gives its reference back)
        pgv_ctx_destroy(lc);
    }
    ix->lanes.clear();
    if (ix->lane_event) (void)hipEventDestroy(ix->lane_event);
    ix->lane_event = nullptr;
    if (ix->lane_scan_done) (void)hipEventDestroy(ix->lane_scan_done);
    ix->lane_scan_done = nullptr;
}

void pgv_index_free(pgv_index *ix) {
    if (!ix) return;
    if (!ix->lanes.empty()) index_drop_lanes(ix);
    if (ix->ctx) (void)hipStreamSynchronize(ix->ctx->stream);
    if (ix->refs && __atomic_sub_fetch(ix->refs, 1, __ATOMIC_ACQ_REL) > 0) {
        delete ix;
        return;
    }
    if (ix->arena) {
        if (ix->imported)
            (void)hipIpcCloseMemHandle(ix->arena);
        else
            (void)hipFree(ix->arena);
    }
    if (ix->shadow) (void)hipFree(ix->shadow);
    delete ix->refs;
    delete ix;
}

int pgv_index_tids(pgv_index *ix, const int64_t *slots, int64_t n, uint64_t *out) {
    if (!ix || !out || (n > 0 && !slots)) PGV_FAIL(PGV_ERR_ARG, "pgv_index_tids: index/slots/out is NULL");
    if (!ix->tids) PGV_FAIL(PGV_ERR_STATE, "pgv_index_tids: the index was uploaded without tids");
    if (is_device_ptr(slots) || is_device_ptr(out)) PGV_FAIL(PGV_ERR_ARG, "pgv_index_tids: host arrays only");
    PGV_HIP(hipSetDevice(ix->ctx->device));
    // a scan's slots come in runs (one per list): one copy per run of consecutive slots
    int64_t i = 0;
    while (i < n) {
        if (slots[i] < 0 || slots[i] >= ix->nrows) PGV_FAIL(PGV_ERR_ARG, "pgv_index_tids: slot %lld out of range", (long long)slots[i]);
        int64_t j = i + 1;
        while (j < n && slots[j] == slots[j - 1] + 1) j++;
        if (slots[j - 1] >= ix->nrows) PGV_FAIL(PGV_ERR_ARG, "pgv_index_tids: slot %lld out of range", (long long)slots[j - 1]);
        PGV_HIP(hipMemcpyAsync(out + i, ix->tids + slots[i], sizeof(uint64_t) * (size_t)(j - i), hipMemcpyDeviceToHost,
                               ix->ctx->stream));
        i = j;
    }
    PGV_HIP(hipStreamSynchronize(ix->ctx->stream));
    return PGV_OK;
}

int64_t pgv_index_rows(const pgv_index *ix) { return ix ? ix->nrows : -1; }
int pgv_index_lists(const pgv_index *ix) { return ix ? ix->nlists : -1; }

// device-side core of GetScanLists for nq staged queries
static int rank_lists_impl(pgv_index *ix, const void *q_dev, int nq, int maxprobes,
                           int32_t *out_lists_dev, float *out_dist_dev, ShadowBatch *sb) {
    pgv_ctx *ctx = ix->ctx;
    // distance matrix [nq x nlists], then the maxprobes smallest per row
    PGV_TRY(ctx->dist_mat.ensure(sizeof(float) * (size_t)nq * ix->nlists));
    float *mat = ctx->dist_mat.as<float>();
    PGV_TRY(ctx->sel_a.ensure(sizeof(int64_t) * (size_t)nq * maxprobes));
    float *dist = out_dist_dev;
    if (!dist) {
        PGV_TRY(ctx->sel_b.ensure(sizeof(float) * (size_t)nq * maxprobes));
        dist = ctx->sel_b.as<float>();
    }
    int64_t *pos = ctx->sel_a.as<int64_t>();
    if (ix->nbits > 0) {
        // GetScanLists (src/ivfscan.c:47-118) under hamming_distance: the dense tile kernel with the centers as rows, then
        // the maxprobes smallest per query with ties to the lower list id (the reference's strict `<` at :92)
        ScanTimer timer{ctx};
        PGV_TRY(timer.begin((double)ix->nlists * nq, (double)ix->nlists * ((nq + 31) / 32), true));
        PGV_TRY(launch_hamming_tiles(ctx, ivf_centers(ix), q_dev, bit_query_bytes(ix->nbits), nq, mat));
        PGV_TRY(timer.end());
        PGV_TRY(launch_topk_segments(ctx, mat, nullptr, nq, ix->nlists, maxprobes, dist, pos));
        return launch_cast_pos_to_i32(ctx, pos, (int64_t)nq * maxprobes, out_lists_dev);
    }
    // a batch against a few hundred centers or more: the matrix cores.  Inner product: the values are
    // the result.  L2: the expansion picks maxprobes + 16 candidates, their exact distances decide, and a
    // query whose candidates cannot be proven complete is redone exactly (same scheme as the list scan)
    // a handful of queries: one grid row per query over the centers, selection per query (two launches)
    // (measured on 1000 centers x 1536: ahead of the dense plan + top-k + position cast up to ~24 queries, level at 32)
    if (nq <= 24 && maxprobes <= query_head_cap()) {
        const int64_t cd_stride = query_row_stride(ix->nlists);
        PGV_TRY(ctx->dist_mat.ensure(sizeof(float) * (size_t)nq * cd_stride));
        return launch_query_rank(ctx, ix, q_dev, nq, ctx->dist_mat.as<float>(), cd_stride, maxprobes, out_lists_dev,
                                 out_dist_dev);
    }
    int cand = maxprobes + 16 < ix->nlists ? maxprobes + 16 : ix->nlists;
    // the fp16 center shadow (below) ranks with a band ~0.8 wide on the headline, where the bulk of the 1000 centers lies
    // a few dozen to the unit: with 16 spare candidates 2.5 queries of 1024 a step were flagged and widened (measured,
    // profiles/r09_step_overhead.md: their batch_fix_kernel pass cost ~25 us a step).  54 spare cost nothing -- the
    // selection pads 10 + 16 to 32 and 10 + 54 to 64 entries, the list scan's own shape, and the recheck reads only
    // the band's prefix
    const int rank_env = rank_shadow_env();
    const bool rank_sh = ix->metric == PGV_L2SQ && ix->cshadow && ix->dtype == PGV_F32 && rank_env != 0 && shadow_env() != 0;
    if (rank_sh && maxprobes + 54 <= 256) cand = maxprobes + 54 < ix->nlists ? maxprobes + 54 : ix->nlists;
    const bool mfma = nq >= 128 && ix->nlists >= 64 && !ctx->no_mfma_scan &&
                      (ix->metric == PGV_NEG_IP || (ix->metric == PGV_L2SQ && ix->center_norms && cand <= 256));
    if (mfma && ix->metric == PGV_L2SQ) {
        // fp32 centers with an fp16 copy: the expansion only picks the candidates, so it multiplies the
        // copy and the cast queries -- the three-stage fp16 form of the kernel, half the bytes -- and the band grows by
        // the per-query term ceps (pgv_internal.h).  The cast runs here, once for the batch: the list scan that follows
        // reads the same fp16 queries
        ShadowBatch own;
        if (!sb) sb = &own;
        const bool scan_follows = sb->scan_follows;
        if (rank_sh) {
            PGV_TRY(shadow_batch_cast(ix, q_dev, nq, maxprobes, true, scan_follows, sb));
            PGV_TRY(dense_scan(ctx, ivf_shadow_centers(ix), sb->qcast, nq, ix->nlists, mat, true, ix->center_norms, nullptr,
                               sb->cscale));
        } else {
            PGV_TRY(dense_scan(ctx, ivf_centers(ix), q_dev, nq, ix->nlists, mat, true, ix->center_norms, nullptr));
        }
        // the pair terms of the shadow scan that follows: q.c of the lists emitted, beside their exact distances
        ExactTail tail;
        tail.pair_t = (rank_sh && rank_env == 1 && scan_follows) ? sb->pair_t : nullptr;
        // ... and its plan's counting: the buffers are sized here, ahead of the kernels that write them;
        // the selection clears cnt | fill (every call: nothing is assumed of what an earlier call left), the recheck
        // counts the lists where it emits them and batch_fix_kernel moves the counts of the queries it redoes
        PlanBuffers pbuf;
        if (tail.pair_t) {
            PGV_TRY(plan_batch_reserve(ctx, ix->nlists, nq, maxprobes, &pbuf));
            tail.emit = {pbuf.cnt, pbuf.probe_off, pbuf.seg_len, ix->list_offsets};
            if (sb->need > 0 && probe_prune_on(ix, maxprobes)) {
                tail.emit.radius = ix->list_radius;
                tail.emit.need = sb->need;
            }
        }
        tail.rows = {ix->centers, nullptr, nullptr, ix->geom, ix->dtype,
                     reinterpret_cast<const unsigned *>(ix->center_norms + ix->nlists)};
        tail.queries = q_dev;
        tail.nq = nq;
        tail.kprime = cand;
        tail.k = maxprobes;
        tail.approx = mat;
        tail.fixed_len = ix->nlists;  // a center's position in the matrix row is its id
        // (dense_scan: the 32-query kernel, its 16-wide form for a last group of <= 16 queries)
        tail.bound = scan_bound_chain(ctx, ix->geom.ld, scan_chain_length(ix->geom, ix->dtype, false));
        if (rank_sh) tail.bound = shadow_band(ix->geom.ld, tail.bound.g_ref);
        tail.eps_add = rank_sh ? sb->ceps : nullptr;
        tail.out_dist = dist;
        tail.out_i32 = out_lists_dev;  // the center ids leave as the int32 list ids the callers want (no conversion pass)
        PGV_TRY(launch_exact_tail(ctx, tail, ctx->ms_b));
        sb->pairs_done = tail.pair_t != nullptr;
        return PGV_OK;
    } else {
        PGV_TRY(dense_scan(ctx, ivf_centers(ix), q_dev, nq, ix->nlists, mat, mfma, nullptr, nullptr));
        PGV_TRY(launch_topk_segments(ctx, mat, nullptr, nq, ix->nlists, maxprobes, dist, pos));
    }
    PGV_TRY(launch_cast_pos_to_i32(ctx, pos, (int64_t)nq * maxprobes, out_lists_dev));
    return PGV_OK;
}

int rank_lists_dev(pgv_index *ix, const void *q_dev, int nq, int maxprobes, int32_t *out_lists_dev, float *out_dist_dev) {
    return rank_lists_impl(ix, q_dev, nq, maxprobes, out_lists_dev, out_dist_dev, nullptr);
}

int pgv_rank_lists(pgv_index *ix, const void *queries, int nq, int maxprobes, int32_t *out_lists,
                   float *out_dist) {
    if (!ix || !out_lists) PGV_FAIL(PGV_ERR_ARG, "pgv_rank_lists: index/out_lists is NULL");
    if (nq < 0) PGV_FAIL(PGV_ERR_ARG, "nq < 0");
    if (maxprobes < 1 || maxprobes > ix->nlists)
        PGV_FAIL(PGV_ERR_ARG, "maxprobes %d outside 1..lists (%d)", maxprobes, ix->nlists);
    if (nq == 0) return PGV_OK;
    if (!queries) PGV_FAIL(PGV_ERR_ARG, "queries is NULL");
    pgv_ctx *ctx = ix->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    const void *q_dev;
    PGV_TRY(stage_queries(ix, queries, nq, &q_dev));
    OutArg ol, od;
    PGV_TRY(ol.init(out_lists, sizeof(int32_t) * (size_t)nq * maxprobes, ctx->out_stage));
    PGV_TRY(od.init(out_dist, sizeof(float) * (size_t)nq * maxprobes, ctx->out_stage2));
    PGV_TRY(rank_lists_dev(ix, q_dev, nq, maxprobes, ol.as<int32_t>(), od.as<float>()));
    bool need = false;
    PGV_TRY(ol.finish(ctx, &need));
    PGV_TRY(od.finish(ctx, &need));
    return sync_if(ctx, need);
}

// GetScanItems + head of the sorted stream for staged queries and device probe lists
// lanes of overlapping batches: this stream's list scan starts when the previous lane's has ended
static int scan_turn_begin(pgv_ctx *ctx) {
    if (ctx->scan_gate) PGV_HIP(hipStreamWaitEvent(ctx->stream, ctx->scan_gate, 0));
    return PGV_OK;
}
static int scan_turn_end(pgv_ctx *ctx) {
    if (ctx->scan_gate) PGV_HIP(hipEventRecord(ctx->scan_gate, ctx->stream));
    return PGV_OK;
}

// What the batched list scan does with nq queries x probes lists and heads of k, decided from the batch's shape before
// anything is launched: scan_batch_impl follows it, and pgv_search_batch tells the ranking of it ahead of time (`shadow`)
struct ScanPath {
    bool bits = false;       // a bit index: always the list-major plan into hamming_list_kernel, nothing else below applies
    bool per_query = false;  // every query scans its own lists: query_scan_kernel + mq_head_kernel, nothing below applies
    bool use_mfma = false;   // the matrix cores (32 queries per pass)
    bool use_tile = false;   // the tile kernel (16 queries per pass over the rows)
    bool wide = false;       // the 64-query form of the matrix-core kernel
    int qt = 0, rows_per_task = 0;  // queries | rows per task
    bool approx = false;     // MFMA L2: the values only pick candidates, the exact tail decides
    bool shadow = false;     // ... and come from the fp16 residual shadow (kernels_shadow.hip): half the bytes
};
static ScanPath scan_path(const pgv_index *ix, int nq, int probes, int k) {
    ScanPath p;
    // invert to list-major work.  Queries per list on average decides how wide a group is worth.  Lists probed by more
    // than 8 queries go to the tile kernel (16 queries per pass over the rows) when the row shape allows it.
    const double share = (double)nq * probes / (double)ix->nlists;
    if (ix->nbits > 0) {
        // integer distances: no per-query path, no matrix cores, no tile path, no shadow, no exact tail
        p.bits = true;
        p.qt = hamming_list_group_size(share);
        p.rows_per_task = hamming_list_rows_per_task();
        return p;
    }
    // Too few queries to share rows between them (every probed list belongs to one query): the list-major plan
    // gains nothing and costs a dozen launches.  Each query scans its own lists (query_scan_kernel, one grid row per
    // query) and selects its own head (mq_head_kernel): two launches.
    p.per_query = (share <= 0.4 || nq <= 4) && nq <= 1024 && probes <= query_max_batch_lists() && k <= query_head_cap();
    if (p.per_query) return p;
    // ... and to the matrix cores (32 queries per pass) for L2 / inner product heads of up to 192
    p.use_mfma = share > 3.0 && k <= 192 && !ix->ctx->no_mfma_scan &&
                 (ix->metric == PGV_NEG_IP || (ix->metric == PGV_L2SQ && ix->row_norms));
    p.use_tile = !p.use_mfma && tile_scan_supported(ix->geom) && share > 8.0;
    // lists probed by more than 32 queries of the batch are streamed once per group of `qt` queries: from ~12 queries per
    // list on average (configs[2] / [4]: 1024 x 64 probes over 4096 lists = 16) enough lists pass 32 for the 64-query
    // form of the kernel to pay (PGV_SCAN_WIDE = 0 / 1 forces it off / on: A/B)
    static const int wide_env = [] {
        const char *e = getenv("PGV_SCAN_WIDE");
        return e ? atoi(e) : -1;
    }();
    // measured (10 M rows, lists 4096, probes 64, 1024 queries): 3072-d fp16 88.5 k -> 93.3 k QPS (scan 10.81 -> 10.19 ms); 1536-d
    // fp32: HBM traffic -16 % (passes 1.26 -> 1.06) but the scan only 11.83 -> 11.43 ms, 81.7 k -> 84.4 k QPS (round 6; one GPU's
    // share 612 k -> 640 k) -- a task of two fp32 tiles per stage fill runs the matrix pipes at ~90 %, so the 64-query form
    // buys a few per cent there, not the traffic's 16; below ~12 queries per list it costs (headline, share 10: -3 %)
    p.wide = p.use_mfma && (wide_env < 0 ? share > 12.0 : wide_env != 0);
    p.qt = p.use_mfma ? (p.wide ? mfma_scan_queries_per_task_wide() : mfma_scan_queries_per_task())
                      : (p.use_tile ? tile_scan_queries_per_task()
                                    : scan_group_size(ix->geom, ix->dtype, (int)std::ceil(share)));
    constexpr int rpt_tiles = 20;  // tiles per task (measured best of 10 / 20 / 40 / 80 on the headline batch)
    p.rows_per_task = p.use_mfma ? mfma_scan_rows_per_task()
                                 : (p.use_tile ? rpt_tiles * tile_scan_tile_rows(ix->geom)
                                               : (p.qt >= 16 ? 256 : (p.qt >= 4 ? 128 : 64)));
    p.approx = p.use_mfma && ix->metric == PGV_L2SQ;
    // fp32 L2 with the fp16 residual shadow: the scan streams half the bytes
    p.shadow = p.approx && ix->shadow && shadow_env() != 0;
    return p;
}

// One list scan, by the kernel `path` names: its turn among the lanes, the timer, the launch.  out[pair.out_rel + row] of
// every task of `work`.  queries / qscale: the staged queries -- under path.shadow the shadow batch's cast ones, which
// go with the shadow rows, and their factors.  counted: (row, query) pairs = rows streamed, where the host knows them
static int list_scan_step(pgv_index *ix, const ScanPath &path, const ScanWork &work, const void *queries, const float *qscale,
                          double counted, float *out) {
    pgv_ctx *ctx = ix->ctx;
    const RowsView v = path.shadow ? ivf_shadow_rows(ix) : ivf_rows(ix);
    PGV_TRY(scan_turn_begin(ctx));
    ScanTimer timer{ctx};
    PGV_TRY(timer.begin(counted, counted));
    if (path.bits)
        PGV_TRY(launch_hamming_lists(ctx, v, queries, bit_query_bytes(ix->nbits), work, path.qt, out));
    else if (path.use_mfma)
        PGV_TRY(launch_mfma_scan(ctx, v, queries, work, ix->row_norms, nullptr, out, rows_stream_past_caches(v), path.qt,
                                 path.shadow ? qscale : nullptr));
    else if (path.use_tile)
        PGV_TRY(launch_tile_scan(ctx, v, queries, work, out));
    else
        PGV_TRY(launch_scan(ctx, v, queries, work, path.qt, out));
    PGV_TRY(timer.end());
    return scan_turn_end(ctx);
}

static int scan_batch_impl(pgv_index *ix, const void *q_dev, int nq, const int32_t *probe_lists, int probes,
                           int k, float *out_dist, int64_t *out_slot, uint64_t *out_tid, ShadowBatch *sb, bool prune) {
    pgv_ctx *ctx = ix->ctx;
    const ScanPath path = scan_path(ix, nq, probes, k);
    if (path.per_query) {
        const int64_t bound = ix->len_prefix[probes];  // rows of the `probes` longest lists
        const int64_t seg_stride = query_row_stride(bound);
        PGV_TRY(ctx->plan_d.ensure(sizeof(float) * (size_t)nq * seg_stride));
        OutArg od, os, ot;
        PGV_TRY(od.init(out_dist, sizeof(float) * (size_t)nq * k, ctx->out_stage));
        PGV_TRY(os.init(out_slot, sizeof(int64_t) * (size_t)nq * k, ctx->out_stage2));
        PGV_TRY(ot.init(out_tid, sizeof(uint64_t) * (size_t)nq * k, ctx->sel_b));
        PGV_TRY(scan_turn_begin(ctx));
        ScanTimer timer{ctx};
        PGV_TRY(timer.begin(0.0, 0.0));  // pairs / rows are added up on the device by mq_head_kernel
        float *seg = ctx->plan_d.as<float>();
        PGV_TRY(launch_query_scan(ctx, ix, q_dev, nq, probe_lists, probes, bound, seg, seg_stride));
        PGV_TRY(launch_multi_head(ctx, ix, nq, seg, seg_stride, probe_lists, probes, k, od.as<float>(), os.as<int64_t>(),
                                  ot.as<uint64_t>()));
        PGV_TRY(timer.end());
        PGV_TRY(scan_turn_end(ctx));
        bool need = false;
        PGV_TRY(od.finish(ctx, &need));
        PGV_TRY(os.finish(ctx, &need));
        PGV_TRY(ot.finish(ctx, &need));
        return sync_if(ctx, need);
    }
    // A batch that pgv_search_batch ranked over the center shadow brings the shadow scan's cast queries, their factors
    // 2^(1 + s + s_q) and band terms, and every probed pair's -2 q.c_l (ShadowBatch); otherwise they are made here
    ShadowBatch own;
    if (!sb) sb = &own;
    if (path.shadow && !sb->cast_for_scan) PGV_TRY(shadow_batch_cast(ix, q_dev, nq, probes, false, true, sb));
    const float *pair_t = (path.shadow && sb->pairs_done) ? sb->pair_t : nullptr;
    // lists that did not come from this batch's ranking over the center shadow: what that ranking's recheck would have
    // done to them is done here, in front of the plan -- the pairs' t, and the probes that cannot reach the head dropped
    // (-1 in a copy of the lists: the plan, the scan and the tail see the lists the fused route would have emitted)
    const bool counted = pair_t != nullptr;
    if (path.shadow && !pair_t && prune && probe_prune_on(ix, probes)) {
        PGV_TRY(ctx->plan_c.ensure(sizeof(int32_t) * (size_t)nq * probes));
        PGV_TRY(launch_probe_prune(ctx, ix, q_dev, nq, probe_lists, probes, k, ctx->plan_c.as<int32_t>(), sb->pair_t));
        probe_lists = ctx->plan_c.as<int32_t>();
        pair_t = sb->pair_t;
    }
    PlanResult plan;
    // (pair_t set: the ranking of this very batch also counted into the plan's buffers -- the plan is two launches)
    PGV_TRY(launch_plan_batch(ctx, ix, probe_lists, nq, probes, path.qt, path.rows_per_task, ctx->profiling, &plan, pair_t,
                              counted));
    if (path.shadow) {
        if (!pair_t)  // ... and every probe is kept (the sharded search, PGV_PROBE_PRUNE=0, an index without radii)
            PGV_TRY(launch_shadow_pairs(ctx, ix->geom, q_dev, ix->centers, plan.pair_start, ix->nlists, (int64_t)nq * probes,
                                        plan.pairs));
        ctx->scan_shadow_queries += nq;
    }

    // GetScanItems: one streaming pass
    PGV_TRY(ctx->plan_d.ensure(sizeof(float) * (size_t)(plan.out_bound > 0 ? plan.out_bound : 1)));
    float *seg_vals = ctx->plan_d.as<float>();
    // (pairs / rows of this launch are accumulated on the device)
    if (plan.ntasks_bound > 0)
        PGV_TRY(list_scan_step(ix, path, plan.work(), path.shadow ? sb->qcast : q_dev, sb->qscale, 0.0, seg_vals));

    // head of the sorted stream
    OutArg od, os, ot;
    PGV_TRY(od.init(out_dist, sizeof(float) * (size_t)nq * k, ctx->out_stage));
    PGV_TRY(os.init(out_slot, sizeof(int64_t) * (size_t)nq * k, ctx->out_stage2));
    PGV_TRY(ot.init(out_tid, sizeof(uint64_t) * (size_t)nq * k, ctx->sel_b));
    PGV_TRY(ctx->sel_a.ensure(sizeof(int64_t) * (size_t)nq * k));
    int64_t *pos = ctx->sel_a.as<int64_t>();
    if (path.approx) {
        // (the 64-query form of the scan keeps its four chains as consecutive quarters of the row: whole 128-byte slices;
        // the chain length covers every form that a task of this launch may take)
        ExactTail tail;
        tail.rows = {ix->vectors, ix->tids, ix->list_offsets, ix->geom, ix->dtype,
                     reinterpret_cast<const unsigned *>(ix->row_norms + ix->nrows)};
        tail.queries = q_dev;
        tail.nq = nq;
        tail.kprime = approx_candidates(k);
        tail.k = k;
        tail.approx = seg_vals;
        tail.probe_lists = probe_lists;  // (the candidates' positions become row slots inside the recheck)
        tail.probe_off = plan.probe_off;
        tail.probes = probes;
        tail.seg_start = plan.seg_start;
        tail.seg_bound = ix->len_prefix[probes];  // rows of the `probes` longest lists
        tail.bound = scan_bound_chain(ctx, ix->geom.ld, scan_chain_length(ix->geom, ix->dtype, path.wide));
        if (path.shadow) tail.bound = shadow_band(ix->geom.ld, tail.bound.g_ref);
        tail.eps_add = path.shadow ? sb->qeps : nullptr;
        tail.out_dist = od.as<float>();
        tail.out_slot = os.as<int64_t>();
        tail.out_tid = ot.as<uint64_t>();
        PGV_TRY(launch_exact_tail(ctx, tail, ctx->ms_a));
    } else {
        PGV_TRY(launch_topk_segments(ctx, seg_vals, plan.seg_start, nq, 0, k, od.as<float>(), pos, nullptr, nullptr, 0,
                                     ix->len_prefix[probes]));
        PGV_TRY(launch_positions_to_slots(ctx, ix, probe_lists, plan.probe_off, nq, probes, k, pos,
                                          os.as<int64_t>(), ot.as<uint64_t>()));
    }
    bool need = false;
    PGV_TRY(od.finish(ctx, &need));
    PGV_TRY(os.finish(ctx, &need));
    PGV_TRY(ot.finish(ctx, &need));
    return sync_if(ctx, need);
}

int scan_batch_dev(pgv_index *ix, const void *q_dev, int nq, const int32_t *probe_lists, int probes, int k, float *out_dist,
                   int64_t *out_slot, uint64_t *out_tid, bool prune) {
    return scan_batch_impl(ix, q_dev, nq, probe_lists, probes, k, out_dist, out_slot, out_tid, nullptr, prune);
}

int pgv_scan_lists(pgv_index *ix, const void *query, const int32_t *lists, int nlists,
                   float *out_dist, int64_t *out_slot, int64_t capacity, int64_t *out_count) {
    if (!ix || !out_count) PGV_FAIL(PGV_ERR_ARG, "pgv_scan_lists: index/out_count is NULL");
    if (nlists < 0 || (nlists > 0 && !lists)) PGV_FAIL(PGV_ERR_ARG, "bad list array");
    pgv_ctx *ctx = ix->ctx;
    PGV_HIP(hipSetDevice(ctx->device));

    std::vector<int32_t> hl((size_t)nlists);
    if (nlists) {
        if (is_device_ptr(lists))
            PGV_HIP(hipMemcpy(hl.data(), lists, sizeof(int32_t) * (size_t)nlists, hipMemcpyDeviceToHost));
        else
            memcpy(hl.data(), lists, sizeof(int32_t) * (size_t)nlists);
    }
    int64_t m = 0;
    for (int p = 0; p < nlists; p++) {
        if (hl[p] < 0 || hl[p] >= ix->nlists) PGV_FAIL(PGV_ERR_ARG, "list id %d out of range", hl[p]);
        m += ix->h_offsets[hl[p] + 1] - ix->h_offsets[hl[p]];
    }
    *out_count = m;
    if (m > capacity) PGV_FAIL(PGV_ERR_ARG, "output capacity %lld < %lld tuples", (long long)capacity, (long long)m);
    if (m == 0) return PGV_OK;
    if (!out_dist || !out_slot) PGV_FAIL(PGV_ERR_ARG, "out_dist/out_slot is NULL");

    OutArg od, os;
    PGV_TRY(od.init(out_dist, sizeof(float) * (size_t)m, ctx->out_stage));
    PGV_TRY(os.init(out_slot, sizeof(int64_t) * (size_t)m, ctx->out_stage2));

    // plan on the host: per probed list a run of chunks, all for the one query -- the batch's list kernels with one pair
    // per task
    ScanPath path;
    path.bits = ix->nbits > 0;
    path.qt = path.bits ? hamming_list_group_size(1.0) : 1;
    path.rows_per_task = path.bits ? hamming_list_rows_per_task() : rows_per_task_for(ctx, m, 1);
    const int ch = path.rows_per_task;
    int64_t ntasks = 0;
    for (int p = 0; p < nlists; p++) {
        int64_t len = ix->h_offsets[hl[p] + 1] - ix->h_offsets[hl[p]];
        ntasks += (len + ch - 1) / ch;
    }
    const size_t tb = sizeof(ScanTask) * (size_t)ntasks, pb = sizeof(ScanPair) * (size_t)nlists,
                 ob = sizeof(int64_t) * (size_t)nlists, lb = sizeof(int32_t) * (size_t)nlists;
    PGV_TRY(staging_acquire(ctx));
    PGV_TRY(ctx->h_a.ensure(tb + pb + ob + lb + 16));
    char *hb = ctx->h_a.as<char>();
    ScanTask *ht = reinterpret_cast<ScanTask *>(hb);
    ScanPair *hp = reinterpret_cast<ScanPair *>(hb + tb);
    int64_t *hoff = reinterpret_cast<int64_t *>(hb + tb + pb);
    int32_t *hlist = reinterpret_cast<int32_t *>(hb + tb + pb + ob);
    int *hn = reinterpret_cast<int *>(hb + tb + pb + ob + lb);
    int64_t t = 0, run = 0;
    for (int p = 0; p < nlists; p++) {
        const int64_t beg = ix->h_offsets[hl[p]], len = ix->h_offsets[hl[p] + 1] - beg;
        hp[p].out_rel = run - beg;
        hp[p].query = 0;
        hp[p].pad = 0;
        hoff[p] = run;
        hlist[p] = hl[p];
        for (int64_t c = 0; c * ch < len; c++) {
            ht[t].row0 = beg + c * ch;
            int64_t left = len - c * ch;
            ht[t].nrows = (int)(left < ch ? left : ch);
            ht[t].pair0 = p;
            ht[t].npairs = 1;
            ht[t].pad = 0;
            t++;
        }
        run += len;
    }
    *hn = (int)ntasks;
    const size_t total = tb + pb + ob + lb + 16;
    PGV_TRY(ctx->tasks.ensure(total));
    PGV_HIP(hipMemcpyAsync(ctx->tasks.p, hb, total, hipMemcpyHostToDevice, ctx->stream));
    char *db = ctx->tasks.as<char>();

    PGV_TRY(launch_iota_slots(ctx, ix, reinterpret_cast<int32_t *>(db + tb + pb + ob), nlists,
                              reinterpret_cast<int64_t *>(db + tb + pb), os.as<int64_t>()));
    if (query == nullptr) {
        // ZeroDistance (src/ivfscan.c:192-196): every tuple at distance 0
        PGV_HIP(hipMemsetAsync(od.dev, 0, sizeof(float) * (size_t)m, ctx->stream));
    } else {
        const void *q_dev;
        PGV_TRY(stage_queries(ix, query, 1, &q_dev));
        const ScanWork work{reinterpret_cast<ScanTask *>(db), reinterpret_cast<int *>(db + tb + pb + ob + lb), (int)ntasks,
                            reinterpret_cast<ScanPair *>(db + tb)};
        PGV_TRY(list_scan_step(ix, path, work, q_dev, nullptr, (double)m, od.as<float>()));
    }
    bool need = true;  // h_a must be consumed before the next call rewrites it
    PGV_TRY(od.finish(ctx, &need));
    PGV_TRY(os.finish(ctx, &need));
    return sync_if(ctx, need);
}

int check_batch_args(pgv_index *ix, const void *queries, int nq, int probes, int k, float *out_dist,
                            uint64_t *out_tid, const char *who) {
    if (!ix) PGV_FAIL(PGV_ERR_ARG, "%s: index is NULL", who);
    if (nq < 0 || k < 1) PGV_FAIL(PGV_ERR_ARG, "bad nq/k");
    if (probes < 1 || probes > ix->nlists)
        PGV_FAIL(PGV_ERR_ARG, "probes %d outside 1..lists (%d)", probes, ix->nlists);
    if (out_tid && !ix->tids) PGV_FAIL(PGV_ERR_STATE, "index was uploaded without tids");
    if (nq > 0 && (!queries || !out_dist)) PGV_FAIL(PGV_ERR_ARG, "queries/out_dist is NULL");
    return PGV_OK;
}

int pgv_search_batch(pgv_index *ix, const void *queries, int nq, int probes, int k, float *out_dist,
                     int64_t *out_slot, uint64_t *out_tid) {
    PGV_TRY(check_batch_args(ix, queries, nq, probes, k, out_dist, out_tid, "pgv_search_batch"));
    if (nq == 0) return PGV_OK;
    if (!ix->lanes.empty()) {
        // overlapping batches: this one runs on the next lane's stream, behind whatever the caller's stream holds now
        // (device-side queries may still be on their way) and beside the batch the previous call put on another lane
        pgv_index *lane = ix->lanes[ix->lane_next++ % ix->lanes.size()];
        PGV_HIP(hipSetDevice(ix->ctx->device));
        PGV_HIP(hipEventRecord(ix->lane_event, ix->ctx->stream));
        PGV_HIP(hipStreamWaitEvent(lane->ctx->stream, ix->lane_event, 0));
        return pgv_search_batch(lane, queries, nq, probes, k, out_dist, out_slot, out_tid);
    }
    pgv_ctx *ctx = ix->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    const void *q_dev;
    PGV_TRY(stage_queries(ix, queries, nq, &q_dev));
    // GetScanLists for the whole batch
    PGV_TRY(ctx->idx_stage.ensure(sizeof(int32_t) * (size_t)nq * probes));
    int32_t *probe_lists = ctx->idx_stage.as<int32_t>();
    // one query cast for the batch where both halves read fp16, and the ranking's q.c_l for the scan
    ShadowBatch sb;
    sb.scan_follows = scan_path(ix, nq, probes, k).shadow;
    sb.need = k;
    PGV_TRY(rank_lists_impl(ix, q_dev, nq, probes, probe_lists, nullptr, &sb));
    return scan_batch_impl(ix, q_dev, nq, probe_lists, probes, k, out_dist, out_slot, out_tid, &sb, true);
}

int pgv_scan_batch(pgv_index *ix, const void *queries, int nq, const int32_t *probe_lists, int probes, int k,
                   float *out_dist, int64_t *out_slot, uint64_t *out_tid) {
    PGV_TRY(check_batch_args(ix, queries, nq, probes, k, out_dist, out_tid, "pgv_scan_batch"));
    if (nq == 0) return PGV_OK;
    if (!probe_lists) PGV_FAIL(PGV_ERR_ARG, "probe_lists is NULL");
    pgv_ctx *ctx = ix->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    // the planner indexes list_offsets with these ids: host-side lists are checked here; lists that are
    // already on the device must come from pgv_rank_lists (ids in range, distinct per query)
    if (!is_device_ptr(probe_lists)) {
        for (size_t i = 0; i < (size_t)nq * probes; i++)
            if (probe_lists[i] < 0 || probe_lists[i] >= ix->nlists)
                PGV_FAIL(PGV_ERR_ARG, "probe list id %d out of range 0..%d", probe_lists[i], ix->nlists - 1);
    }
    const void *q_dev, *pl_dev;
    PGV_TRY(stage_queries(ix, queries, nq, &q_dev));
    PGV_TRY(stage_flat(ctx, probe_lists, sizeof(int32_t) * (size_t)nq * probes, ctx->idx_stage, &pl_dev));
    return scan_batch_dev(ix, q_dev, nq, static_cast<const int32_t *>(pl_dev), probes, k, out_dist, out_slot,
                          out_tid, true);
}

// the query cast of the shadow paths on its own (tests: shadow_query_kernel's outputs against a host model)
int pgv_index_shadow_cast(pgv_index *ix, const void *queries, int nq, void *out_qcast, float *out_qscale, float *out_qeps,
                          float *out_cscale, float *out_ceps) {
    if (!ix || !queries || nq < 1) PGV_FAIL(PGV_ERR_ARG, "pgv_index_shadow_cast: index/queries is NULL or nq < 1");
    PGV_NO_BIT_INDEX(ix, "pgv_index_shadow_cast");
    if (!ix->shadow || !ix->cshadow) PGV_FAIL(PGV_ERR_STATE, "pgv_index_shadow_cast: the index has no fp16 shadow");
    pgv_ctx *ctx = ix->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    const void *q_dev;
    PGV_TRY(stage_rows(ctx, queries, nq, ix->dim, ix->dtype, ix->geom, ctx->q_stage, &q_dev));
    ShadowBatch sb;
    PGV_TRY(shadow_batch_cast(ix, q_dev, nq, 1, true, true, &sb));
    const struct {
        void *dst;
        const void *src;
        size_t bytes;
    } parts[] = {{out_qcast, sb.qcast, (size_t)nq * ix->shadow_geom.ld * sizeof(uint16_t)},
                 {out_qscale, sb.qscale, sizeof(float) * (size_t)nq},
                 {out_qeps, sb.qeps, sizeof(float) * (size_t)nq},
                 {out_cscale, sb.cscale, sizeof(float) * (size_t)nq},
                 {out_ceps, sb.ceps, sizeof(float) * (size_t)nq}};
    for (const auto &p : parts)
        if (p.dst) PGV_HIP(hipMemcpyAsync(p.dst, p.src, p.bytes, hipMemcpyDefault, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    return PGV_OK;
}

// ------------------------------------------------------- one query at a time
namespace {

// Admission of single-query scans (threads of ONE process; a Postgres backend is a process of its own and has one
// scan in flight at most).  Measured on MI355X (profiles/r03_single_query_concurrency.md): the device runs ~2.5
// kernels of different streams at a time (4 hardware queues), 16 backends reach 48 k QPS and every backend beyond
// that LOWERS the total (32: 32 k, 64: 16 k -- co-running kernels slow each other down and the runtime interleaves
// barrier packets for every stream switch on a queue).  So at most g_scan_gate_width scan+head pairs are in flight
// per process; the others sleep on a futex.  PGV_MAX_INFLIGHT_SCANS overrides the width (0 = no gate).
static int g_scan_gate_width = -1;
static PgvGate g_scan_gate;  // pgv_gate.h (round 3's version lost wake-ups: the hang of BENCH_r03)
static void scan_gate_enter() {
    if (g_scan_gate_width < 0) {
        const char *e = getenv("PGV_MAX_INFLIGHT_SCANS");
        __atomic_store_n(&g_scan_gate_width, e ? atoi(e) : 16, __ATOMIC_RELAXED);
    }
    g_scan_gate.enter(g_scan_gate_width);
}
static void scan_gate_leave() { g_scan_gate.leave(g_scan_gate_width); }
struct ScanGate {
    ScanGate() { scan_gate_enter(); }
    ~ScanGate() { scan_gate_leave(); }
};

// the head record lands in pinned host memory; its seq word is written last.  Spin on it for a
// while (the kernel's own stores are the fastest completion signal there is), then fall back to
// a stream synchronise.
int wait_head(pgv_ctx *ctx, pgv_query *q, unsigned seq) {
    volatile QueryHead *h = static_cast<volatile QueryHead *>(q->head_pinned);
    for (int spin = 0; spin < 200000; spin++) {
        if (__atomic_load_n(&h->seq, __ATOMIC_ACQUIRE) == seq) return PGV_OK;
        __builtin_ia32_pause();
    }
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    if (__atomic_load_n(&h->seq, __ATOMIC_ACQUIRE) != seq) PGV_FAIL(PGV_ERR_DEVICE, "query kernel did not report");
    return PGV_OK;
}

void copy_head(pgv_query *q, int stride, int n, float *out_dist, int64_t *out_slot, uint64_t *out_tid) {
    if (out_slot) memcpy(out_slot, query_head_slots(q->head_pinned), sizeof(int64_t) * (size_t)n);
    if (out_tid) memcpy(out_tid, query_head_tids(q->head_pinned, stride), sizeof(uint64_t) * (size_t)n);
    if (out_dist) memcpy(out_dist, query_head_dists(q->head_pinned, stride), sizeof(float) * (size_t)n);
}

}  // namespace

// PGV_QUERY_DIRECT=0 keeps the staging kernel (A/B switch)
static bool query_direct_enabled() {
    static const bool on = [] {
        const char *e = getenv("PGV_QUERY_DIRECT");
        return !(e && e[0] == '0');
    }();
    return on;
}

int pgv_query_begin(pgv_index *ix, pgv_query **out) {
    if (!ix || !out) PGV_FAIL(PGV_ERR_ARG, "pgv_query_begin: index/out is NULL");
    *out = nullptr;
    PGV_NO_BIT_INDEX(ix, "pgv_query_begin");
    pgv_ctx *ctx = ix->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    pgv_query *q = new (std::nothrow) pgv_query();
    if (!q) PGV_FAIL(PGV_ERR_NOMEM, "out of host memory");
    q->ix = ix;
    const int cap = query_head_cap();
    const size_t state_bytes = sizeof(int32_t) * (size_t)cap + sizeof(float) * ((size_t)ix->nlists + 4);  // + one float4 of slack
    const size_t row_bytes = ivf_rows(ix).row_bytes();
    q->head_bytes = query_head_bytes(cap);
    int rc = q->state.ensure(state_bytes);
    if (rc == PGV_OK) rc = q->q_dev.ensure(row_bytes);
    if (rc == PGV_OK && hipHostMalloc(&q->q_pinned, row_bytes, hipHostMallocDefault) != hipSuccess) rc = PGV_ERR_NOMEM;
    if (rc == PGV_OK && hipHostMalloc(&q->head_pinned, q->head_bytes, hipHostMallocDefault) != hipSuccess)
        rc = PGV_ERR_NOMEM;
    if (rc == PGV_OK && hipMemsetAsync(q->state.p, 0, state_bytes, ctx->stream) != hipSuccess) rc = PGV_ERR_DEVICE;
    int large_bar = 0;
    if (rc == PGV_OK && query_direct_enabled() &&
        hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, ctx->device) == hipSuccess && large_bar) {
        // a device row the host can store into (the whole of HBM is behind the PCIe BAR): the query then needs no
        // staging kernel.  Optional: without it the pinned row + query_stage_kernel carry the query
        if (hipExtMallocWithFlags(&q->q_direct, row_bytes, hipDeviceMallocFinegrained) != hipSuccess) {
            (void)hipGetLastError();
            q->q_direct = nullptr;
        }
    }
    if (rc != PGV_OK) {
        set_error("pgv_query_begin: allocation failed");
        pgv_query_end(q);
        return rc;
    }
    memset(q->head_pinned, 0, q->head_bytes);
    q->lists = q->state.as<int32_t>();
    q->cdist = reinterpret_cast<float *>(q->lists + cap);
    *out = q;
    return PGV_OK;
}

void pgv_query_end(pgv_query *q) {
    if (!q) return;
    if (q->ix && q->ix->ctx) (void)hipStreamSynchronize(q->ix->ctx->stream);
    q->state.release();
    q->seg.release();
    q->q_dev.release();
    if (q->q_pinned) (void)hipHostFree(q->q_pinned);
    if (q->q_direct) (void)hipFree(q->q_direct);
    if (q->head_pinned) (void)hipHostFree(q->head_pinned);
    delete q;
}

int pgv_query_rank(pgv_query *q, const void *query, int max_probes) {
    if (!q) PGV_FAIL(PGV_ERR_ARG, "pgv_query_rank: q is NULL");
    pgv_index *ix = q->ix;
    pgv_ctx *ctx = ix->ctx;
    if (max_probes < 1 || max_probes > ix->nlists)
        PGV_FAIL(PGV_ERR_ARG, "maxprobes %d outside 1..lists (%d)", max_probes, ix->nlists);
    if (max_probes > query_head_cap())
        PGV_FAIL(PGV_ERR_ARG, "pgv_query_rank handles up to %d probes; use pgv_rank_lists", query_head_cap());
    PGV_HIP(hipSetDevice(ctx->device));
    q->max_probes = max_probes;
    q->is_null = query == nullptr;
    q->cur_n = 0;
    if (q->is_null) return launch_query_iota(ctx, q->lists, max_probes);
    const size_t tight = (size_t)ix->dim * elem_size(ix->dtype), row_bytes = ivf_rows(ix).row_bytes();
    if (is_device_ptr(query)) {
        PGV_HIP(hipMemsetAsync(q->q_dev.p, 0, row_bytes, ctx->stream));
        PGV_HIP(hipMemcpyAsync(q->q_dev.p, query, tight, hipMemcpyDeviceToDevice, ctx->stream));
        q->q_row = q->q_dev.p;
    } else {
        // the previous query's kernels have finished reading q_pinned: every pgv_query_scan waits for its head
        // (a rank that no scan followed is waited for here)
        if (q->rank_pending) PGV_HIP(hipStreamSynchronize(ctx->stream));
        void *dst = q->q_direct ? q->q_direct : q->q_pinned;
        memcpy(dst, query, tight);
        if (row_bytes > tight) memset(static_cast<char *>(dst) + tight, 0, row_bytes - tight);
        if (q->q_direct) {
            // the stores drain to the device ahead of the doorbell write of the launch below (posted writes, in order)
            __builtin_ia32_sfence();
            q->q_row = q->q_direct;
        } else {
            PGV_TRY(launch_query_stage(ctx, q->q_pinned, q->q_dev.p, ix->geom.nvec));
            q->q_row = q->q_dev.p;
        }
    }
    q->rank_pending = true;
    return launch_query_rank(ctx, ix, q->q_row, 1, q->cdist, 0, max_probes, q->lists, nullptr);
}

int pgv_query_scan(pgv_query *q, int first, int nprobes, int head, float *out_dist, int64_t *out_slot,
                   uint64_t *out_tid, int *out_count, int64_t *out_total) {
    if (!q || !out_count) PGV_FAIL(PGV_ERR_ARG, "pgv_query_scan: q/out_count is NULL");
    pgv_index *ix = q->ix;
    pgv_ctx *ctx = ix->ctx;
    if (q->max_probes <= 0) PGV_FAIL(PGV_ERR_STATE, "pgv_query_scan before pgv_query_rank");
    if (first < 0 || nprobes < 1 || first + nprobes > q->max_probes)
        PGV_FAIL(PGV_ERR_ARG, "lists [%d, %d) outside the %d ranked", first, first + nprobes, q->max_probes);
    if (nprobes > query_max_batch_lists())
        PGV_FAIL(PGV_ERR_ARG, "pgv_query_scan handles up to %d lists per batch; use pgv_scan_lists", query_max_batch_lists());
    if (head < 1 || head > query_head_cap()) PGV_FAIL(PGV_ERR_ARG, "head %d outside 1..%d", head, query_head_cap());
    if (out_tid && !ix->tids) PGV_FAIL(PGV_ERR_STATE, "index was uploaded without tids");
    PGV_HIP(hipSetDevice(ctx->device));
    const int64_t bound = ix->len_prefix[nprobes];  // rows of the nprobes longest lists
    PGV_TRY(q->seg.ensure(sizeof(float) * (size_t)query_row_stride(bound)));
    const unsigned seq = ++q->seq ? q->seq : ++q->seq;  // never 0: the cleared record's value
    ScanGate gate;  // held until the head is back (every return below)
    PGV_TRY(launch_query_scan(ctx, ix, q->is_null ? nullptr : q->q_row, 1, q->lists + first, nprobes, bound,
                              q->seg.as<float>(), 0));
    PGV_TRY(launch_query_head(ctx, ix, q->seg.as<float>(), q->lists + first, nprobes, 0, head, q->head_pinned, seq));
    q->cur_first = first;
    q->cur_n = nprobes;
    PGV_TRY(wait_head(ctx, q, seq));
    q->rank_pending = false;
    const QueryHead *h = static_cast<const QueryHead *>(q->head_pinned);
    *out_count = h->count;
    if (out_total) *out_total = h->total;
    copy_head(q, head, h->count, out_dist, out_slot, out_tid);
    return PGV_OK;
}

int pgv_query_more(pgv_query *q, int skip, int count, float *out_dist, int64_t *out_slot, uint64_t *out_tid,
                   int *out_count) {
    if (!q || !out_count) PGV_FAIL(PGV_ERR_ARG, "pgv_query_more: q/out_count is NULL");
    pgv_index *ix = q->ix;
    pgv_ctx *ctx = ix->ctx;
    if (q->cur_n <= 0) PGV_FAIL(PGV_ERR_STATE, "pgv_query_more before pgv_query_scan");
    if (skip < 0 || count < 1 || skip + count > query_head_cap())
        PGV_FAIL(PGV_ERR_ARG, "skip + count = %d exceeds %d; fetch the batch with pgv_scan_lists", skip + count,
                 query_head_cap());
    if (out_tid && !ix->tids) PGV_FAIL(PGV_ERR_STATE, "index was uploaded without tids");
    PGV_HIP(hipSetDevice(ctx->device));
    const unsigned seq = ++q->seq ? q->seq : ++q->seq;
    PGV_TRY(launch_query_head(ctx, ix, q->seg.as<float>(), q->lists + q->cur_first, q->cur_n, skip, count,
                              q->head_pinned, seq));
    PGV_TRY(wait_head(ctx, q, seq));
    const QueryHead *h = static_cast<const QueryHead *>(q->head_pinned);
    *out_count = h->count;
    copy_head(q, count, h->count, out_dist, out_slot, out_tid);
    return PGV_OK;
}

int pgv_query_lists(pgv_query *q, int32_t *out_lists, int n) {
    if (!q || !out_lists) PGV_FAIL(PGV_ERR_ARG, "pgv_query_lists: NULL argument");
    if (n < 0 || n > q->max_probes) PGV_FAIL(PGV_ERR_ARG, "%d lists asked, %d ranked", n, q->max_probes);
    pgv_ctx *ctx = q->ix->ctx;
    PGV_HIP(hipSetDevice(ctx->device));
    PGV_HIP(hipMemcpyAsync(out_lists, q->lists, sizeof(int32_t) * (size_t)n,
                           is_device_ptr(out_lists) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    q->rank_pending = false;
    return PGV_OK;
}

}  // extern "C"
