// pgv_internal.h -- shared declarations of libpgv_hip (host side + launchers).
// gfx950 only; no other backend is supported or compiled.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>

#include "../../include/pgv_hip.h"

namespace pgv {

// ------------------------------------------------------------------ errors
void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

#define PGV_FAIL(code, ...)            \
    do {                               \
        ::pgv::set_error(__VA_ARGS__); \
        return (code);                 \
    } while (0)

#define PGV_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e__ = (call);                                                       \
        if (e__ != hipSuccess) {                                                       \
            ::pgv::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__),   \
                             __FILE__, __LINE__);                                      \
            return e__ == hipErrorOutOfMemory ? PGV_ERR_NOMEM : PGV_ERR_DEVICE;        \
        }                                                                              \
    } while (0)

#define PGV_TRY(call)          \
    do {                       \
        int rc__ = (call);     \
        if (rc__ != PGV_OK)    \
            return rc__;       \
    } while (0)

// ------------------------------------------------------------- device memory
struct DBuf {  // growable device allocation, reused across calls
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);
    void release();
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct HBuf {  // growable pinned host allocation
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);
    void release();
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

bool is_device_ptr(const void *p);

constexpr int kVecBytes = 16;  // every row is padded to whole 16-byte vectors in HBM

constexpr int kHnswMaxBits = 64000;  // bit rows of an HNSW mirror: HNSW_MAX_DIM * 32 (src/hnswutils.c:1414)
constexpr int kIvfMaxBits = 64000;   // ... of an IVFFlat mirror: IVFFLAT_MAX_DIM * 32 (src/ivfutils.c:416)

inline int elem_size(pgv_dtype t) { return t == PGV_F32 ? 4 : 2; }
// padded row length in elements
inline int padded_dim(int dim, pgv_dtype t) {
    int per = kVecBytes / elem_size(t);
    return (dim + per - 1) / per * per;
}

// geometry of the streaming kernels for one row length (see kernels_scan.hip)
struct RowGeom {
    int ld;         // padded elements per row
    int nvec;       // 16-byte vectors per row
    int lpr_log2;   // lanes cooperating on one row = 1 << lpr_log2
    int nchunks;    // loop trips over the row
};
RowGeom row_geom(int dim, pgv_dtype t);
// ... of a packed bit row of nbits (kernels_hnsw.hip): the lane split of the walk and the pair scorer over a bit
// mirror (pgv_hnsw::nbits); ld is the padded row length in BYTES
RowGeom bit_row_geom(int nbits);

// Rows as the scoring and scan kernels and the HNSW walk take them: where they are, how many, how a row is laid out,
// what an element is and which distance goes with it.  Built where it is needed (hnsw_rows / ivf_rows and its kin for a
// mirror, in place for a caller's staged rows), never stored
// Bits: packed bit strings scored by xor + popcount; the metric is unused.  Sparse: sparsevec elements in CSR, a row's
// (index, value) pairs side by side (sparse_pair.h's QElem) from rows[ptr[r]] on; geom is unused
enum class RowKind { F32, F16, Bits, Sparse };
struct RowsView {
    const void *rows;  // [n x geom.nvec] 16-byte vectors; Sparse: [ptr[n] + 1] 8-byte (index, value) pairs
    int64_t n;
    RowGeom geom;
    RowKind kind;
    pgv_metric metric;
    const int64_t *ptr = nullptr;  // Sparse: [n + 1] where each row's pairs start
    bool bits() const { return kind == RowKind::Bits; }
    // bit rows ranked by jaccard_distance (an HNSW mirror of pgv_hnsw_upload_jaccard): their metric slot holds
    // bit_metric_slot(PGV_BIT_JACCARD) = 1; a Hamming mirror's holds 0 and a bit IVFFlat index's PGV_L1, the placeholders
    // they always held, so no view of an index can say Jaccard
    bool jaccard() const { return bits() && (int)metric == (int)PGV_BIT_JACCARD; }
    bool sparse() const { return kind == RowKind::Sparse; }
    pgv_dtype dtype() const { return kind == RowKind::F16 ? PGV_F16 : PGV_F32; }
    size_t row_bytes() const { return bits() ? (size_t)geom.ld : (size_t)geom.ld * elem_size(dtype()); }
};
inline pgv_metric bit_metric_slot(pgv_bit_metric m) { return static_cast<pgv_metric>((int)m); }
inline RowKind row_kind(pgv_dtype t) { return t == PGV_F16 ? RowKind::F16 : RowKind::F32; }

// The graph of an HNSW mirror (pgv_hnsw_set_graph): ONE allocation holding levels | nbr_start | nbr, so that one
// hipIpcMemHandle carries it; a view (pgv_hnsw_share) copies the whole struct from its owner
struct HnswGraph {
    void *mem = nullptr;
    size_t bytes = 0;
    const int32_t *levels = nullptr;     // [n]
    const int64_t *nbr_start = nullptr;  // [n + 1]
    int32_t *nbr = nullptr;              // [nbr_total] neighbour tuples, HnswNeighborTupleData layout
    int64_t nbr_total = 0;
    int m = 0;
    int32_t entry = -1;
};

// one unit of streaming work: rows [row0, row0 + nrows) scored against
// pairs [pair0, pair0 + npairs)
struct ScanTask {
    int64_t row0;
    int32_t nrows;
    int32_t pair0;
    int32_t npairs;
    int32_t pad;
};
// one (query, destination) of a task: distance of row r goes to out[out_rel + r]
struct ScanPair {
    int64_t out_rel;
    int32_t query;
    int32_t pad;
};
constexpr int kStatsWords = 9;  // pgv_ctx::stats_dev: the device-side accumulators of pgv_stats ([8]: scan_pruned_probes)
// the work of one planned launch (a PlanResult's, the dense plan's, pgv_scan_lists's host plan); all device arrays
struct ScanWork {
    const ScanTask *tasks;
    const int *ntasks_dev;  // how many of them there are
    int ntasks_bound;       // ... at most, known on the host
    const ScanPair *pairs;
};

}  // namespace pgv

// --------------------------------------------------------------- the context
struct pgv_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // scratch (device)
    pgv::DBuf q_stage, rows_stage, centers_stage, out_stage, out_stage2, idx_stage;
    pgv::DBuf tasks, pairs, counters, plan_a, plan_b, plan_c, plan_d, dist_mat, sel_a, sel_b;
    pgv::DBuf km_a, km_b, km_c, km_d, km_e, km_f, km_g;
    pgv::DBuf ms_b;  // MFMA center ranking: the same scratch as ms_a
    pgv::DBuf dense_plan;  // the last dense (every row x every query) MFMA task list, reused while its shape repeats
    int64_t dense_plan_rows = -1, dense_plan_stride = -1;
    int dense_plan_nq = -1, dense_plan_kind = -1;
    bool counters_clean = false;  // ctx->counters starts zeroed; mfma_scan_kernel leaves its words zero again
    pgv::DBuf ms_a;  // MFMA list scan: query norms | candidate values, positions, slots | flags
    // the shadow paths of a batch (kernels_shadow.hip): cast queries | list-scan factors, band terms | ranking factors,
    // band terms | the probed pairs' t = -2 q.c_l in probe order (written by the ranking's exact recheck)
    pgv::DBuf sh_q;
    pgv::DBuf mf_d;  // MFMA assignment split over center parts: the parts' candidates per row
    pgv::DBuf mf_a, mf_b, mf_c, zeros;  // MFMA assignment: norms, pre-filter candidates, redo list; 16 zero bytes
    pgv::DBuf stats_dev;  // profiling: pgv::kStatsWords doubles ({pairs, rows streamed} of the batched list scans, ...)
    // scratch (pinned host); h_a_busy marks the last async copy out of h_a (waited before reuse)
    pgv::HBuf h_a, h_b, h_c;
    hipEvent_t h_a_busy = nullptr;
    bool h_a_pending = false;
    // per-kernel profiling (pgv_ctx_set_profiling): HIP event pairs around the
    // streaming kernel, resolved lazily in pgv_ctx_get_stats
    bool profiling = false;
    bool no_mfma_scan = false;  // pgv_ctx_set_exact_scan
    bool no_widen = false;      // PGV_NO_WIDEN=1: flagged queries go straight to the exact pass (experiments)
    int bound_mode = 1;         // the scans' bound: PGV_BOUND_WORST_CASE unless pgv_ctx_set_bound says otherwise
    int assign_bound_mode = 1;  // the assignment pre-filter's: PGV_BOUND_WORST_CASE too since round 6 (pgv_ctx_set_bound)
    pgv::DBuf xt_norms;         // pgv_exact_topk: |row|^2 of the caller's rows
    std::vector<hipEvent_t> ev_pool;  // start/stop pairs
    size_t ev_used = 0;
    double scan_ms = 0.0;
    int64_t scan_launches = 0;
    double scan_pairs = 0.0;  // (row, query) pairs scored by timed launches
    double scan_rows = 0.0;   // rows streamed by timed launches
    std::vector<char> ev_is_aux;  // per event pair: counts towards aux_* instead of scan_*
    double aux_ms = 0.0;
    int64_t aux_launches = 0;
    double aux_pairs = 0.0;
    double scan_shadow_queries = 0.0;  // queries of batched list scans that read the fp16 residual shadow
    // lanes of indexes whose batches overlap (pgv_index_set_overlap): contexts with streams of their own that belong to
    // an index of this context; pgv_ctx_sync waits for them, the settings and the statistics include them
    std::vector<pgv_ctx *> children;
    // a lane's list scans take turns with the other lanes': two HBM-bound scans side by side only share the bandwidth,
    // while everything else of a batch (ranking, planning, top-k, recheck) fits under another batch's scan.  The event
    // belongs to the index (pgv_index::lane_scan_done); null outside lanes.
    hipEvent_t scan_gate = nullptr;
};

struct pgv_index {
    pgv_ctx *ctx = nullptr;
    pgv_metric metric = PGV_L2SQ;
    pgv_dtype dtype = PGV_F32;
    int dim = 0;
    // > 0: a mirror of `USING ivfflat (col bit_hamming_ops)` (pgv_index_upload_bits).  Its element type is not a pgv_dtype:
    // centers and rows are nbits bits in geom.nvec 16-byte vectors (geom.ld BYTES), scored by xor + popcount; metric and
    // dtype are placeholders (dim = nbits) that stop mattering in ivf_rows: the kernels get RowKind::Bits from there.
    // There are no norms and no shadow
    int nbits = 0;
    int nlists = 0;
    int64_t nrows = 0;
    pgv::RowGeom geom{};
    void *centers = nullptr;          // [nlists x ld]
    void *vectors = nullptr;          // [nrows x ld]
    int64_t *list_offsets = nullptr;  // device [nlists + 1]
    uint64_t *tids = nullptr;         // device [nrows] or null
    float *row_norms = nullptr;       // device [nrows] |x|^2 then one word: bits of the largest (L2 indexes; the MFMA scan)
    float *center_norms = nullptr;    // the same for the centers [nlists + 1]
    int *refs = nullptr;              // handles (the uploaded index + its pgv_index_share views) on the device arrays
    // every device array above lives in ONE allocation, so that one hipIpcMemHandle carries the whole mirror to
    // another process (pgv_index_export / pgv_index_import)
    void *arena = nullptr;
    size_t arena_bytes = 0;
    bool imported = false;            // arena was opened with hipIpcOpenMemHandle: closed, not freed
    // fp32 L2 indexes: the fp16 residual shadow the batched MFMA list scan streams instead of `vectors`
    // (kernels_shadow.hip): [nrows x shadow_geom.ld] fp16((x - c_l) 2^-shadow_s).  Its own allocation (the IPC
    // handle carries the arena only); shared by pgv_index_share views and freed with the arena; null when not built
    void *shadow = nullptr;
    pgv::RowGeom shadow_geom{};
    int shadow_s = 0;
    double shadow_E = 0.0;            // max over rows |(x - c_l) - 2^s shadow|, rounded up
    double shadow_P = 0.0;            // max over rows |2^s shadow|, rounded up
    // [nlists] R_l >= max |x - c_l| over the list's rows (probe pruning, the rule beside ScanBound): measured by the
    // shadow's build, inside its allocation, shared like it; null without a row shadow: nothing is pruned
    float *list_radius = nullptr;
    // ... and the fp16 copy of its centers that the batch ranking multiplies instead of `centers`:
    // [nlists x shadow_geom.ld] fp16(c 2^-cshadow_s), inside the shadow's allocation; null when not built
    void *cshadow = nullptr;
    int cshadow_s = 0;
    double cshadow_E = 0.0;           // max over centers |c - 2^s_c cshadow|, rounded up
    double cshadow_P = 0.0;           // max over centers |2^s_c cshadow|, rounded up
    std::vector<int64_t> h_offsets;   // host copy
    std::vector<int64_t> len_prefix;  // len_prefix[p] = rows in the p longest lists (output size bound)
    int64_t max_list_len = 0;
    // pgv_index_set_overlap: views of this index on contexts (streams, scratch) of their own; consecutive
    // pgv_search_batch calls take them in turn
    std::vector<pgv_index *> lanes;
    unsigned lane_next = 0;
    hipEvent_t lane_event = nullptr;  // orders a lane's start after what the caller's stream holds at the call
    hipEvent_t lane_scan_done = nullptr;  // the lanes' list scans run one after the other (pgv_ctx::scan_gate)
};

// one backend's index scan (pgv_query_*): everything between amrescan and amendscan that lives on the device
struct pgv_query {
    pgv_index *ix = nullptr;
    pgv::DBuf state;      // lists[head cap] | cdist[nlists]
    pgv::DBuf seg;        // distances of the current GetScanItems batch, tuplesort input order
    pgv::DBuf q_dev;      // the query row, padded
    void *q_pinned = nullptr;     // pinned host staging of the query payload
    const void *q_row = nullptr;  // where the kernels read the current query: q_direct or q_dev
    void *q_direct = nullptr;     // fine-grained device row the host writes through the BAR (no staging kernel), or null
    void *head_pinned = nullptr;  // pinned, device-written: QueryHead + head arrays
    size_t head_bytes = 0;
    int32_t *lists = nullptr;
    float *cdist = nullptr;
    int max_probes = 0;   // lists ranked by the last pgv_query_rank
    bool is_null = false;
    bool rank_pending = false;     // kernels that read q_pinned may still be in flight
    int cur_first = 0, cur_n = 0;  // the batch whose distances are in seg
    unsigned seq = 0;
};

// the element rows of a mirror: what a view (pgv_hnsw_share) has in common with its owner, copied as one struct
struct HnswElements {
    pgv_metric metric = PGV_L2SQ;
    pgv_dtype dtype = PGV_F32;
    int dim = 0;
    // > 0: a mirror of packed bit strings (pgv_hnsw_upload_bits / _jaccard).  Its element type is not a pgv_dtype: rows are
    // nbits bits in geom.nvec 16-byte vectors, scored by popcounts; dtype and dim are unused (dim = nbits), and metric is
    // bit_metric_slot() of the mirror's pgv_bit_metric: 0 (what it always held) bit_hamming_ops, 1 bit_jaccard_ops
    int nbits = 0;
    // a bit mirror uploaded by pgv_hnsw_upload_bits_buildable, or a sparse one uploaded by pgv_hnsw_upload_sparse_buildable:
    // the build-side entries serve it.  A view has it from its owner; an importer does not (the exported handle has no
    // field for it, and importers do not build)
    bool buildable = false;
    // a mirror of sparsevec elements (pgv_hnsw_upload_sparse): `elements` holds the rows' (index, value) pairs one row
    // after the other (and one slack pair), sparse_ptr [n + 1] where each row starts -- in the same allocation, like the
    // payload; dtype and geom are unused, dim is the vectors' dimension
    bool sparse = false;
    const int64_t *sparse_ptr = nullptr;
    int sparse_max_nnz = 0;  // the longest element's stored elements (<= HNSW_MAX_NNZ): sizes the LDS query of a build's walk
    int64_t n = 0;
    pgv::RowGeom geom{};
    void *elements = nullptr;  // [n x ld]
    char *payload = nullptr;  // [n x payload_bytes] behind the elements, same allocation (pgv_hnsw_upload_payload)
    int payload_bytes = 0;
};

struct pgv_hnsw : HnswElements {
    pgv_ctx *ctx = nullptr;
    pgv::HnswGraph graph;
    pgv::DBuf bitmaps;  // visited sets of the search workgroups
    bool imported = false;  // elements / graph were opened with hipIpcOpenMemHandle (a read-only view)
    pgv_hnsw *view_of = nullptr;  // pgv_hnsw_share: a view of that mirror in the same process (own context / stream)
    // the last pgv_hnsw_update_graph of the mirror (through it or through a view), recorded on the stream that ran it:
    // searches on any other stream wait for it on the device (owner's field; views look at view_of's)
    hipEvent_t graph_ev = nullptr;
    bool graph_ev_set = false;
    struct HnswLinkState *link = nullptr;  // pgv_hnsw_link_begin .. _end: the in-memory build's graph state (owner only)
    // pgv_hnsw_set_live: bit e = element e has heap TIDs ((n + 31) / 32 words on the device; owner's fields, views look at
    // view_of's).  Not set: every element is live.  Only pgv_hnsw_repair_neighbors reads it
    pgv::DBuf live;
    bool live_set = false;
    int64_t live_count = 0;
};

namespace pgv {
// a mirror's rows as its kernels take them
inline RowsView hnsw_rows(const pgv_hnsw *h) {
    if (h->sparse) return {h->elements, h->n, h->geom, RowKind::Sparse, h->metric, h->sparse_ptr};
    return {h->elements, h->n, h->geom, h->nbits > 0 ? RowKind::Bits : row_kind(h->dtype), h->metric};
}
// ... an IVFFlat mirror's: the only place that turns pgv_index::nbits into a row kind
inline RowsView ivf_rows(const pgv_index *ix) {
    return {ix->vectors, ix->nrows, ix->geom, ix->nbits > 0 ? RowKind::Bits : row_kind(ix->dtype), ix->metric};
}
inline RowsView ivf_centers(const pgv_index *ix) {
    RowsView v = ivf_rows(ix);
    v.rows = ix->centers;
    v.n = ix->nlists;
    return v;
}
// ... and the fp16 residual shadow of its rows and the fp16 copy of its centers (null rows when not built)
inline RowsView ivf_shadow_rows(const pgv_index *ix) { return {ix->shadow, ix->nrows, ix->shadow_geom, RowKind::F16, ix->metric}; }
inline RowsView ivf_shadow_centers(const pgv_index *ix) {
    return {ix->cshadow, ix->nlists, ix->shadow_geom, RowKind::F16, ix->metric};
}
}  // namespace pgv

// the state of a build whose graph updates run on the device (kernels_hnsw_link.hip): per tuple slot the neighbor's
// distance and closer flag, and the scratch of the batch in flight
struct HnswLinkState {
    float *nb_dist = nullptr;     // [nbr_total]
    uint8_t *nb_flag = nullptr;   // [nbr_total] bit 0 closer; bit 1 of a list's first slot: closerSet
    int *list_count = nullptr;    // [nlists] link requests of the batch in flight per list (slot position / m); zero between batches
    int *list_rec = nullptr;      // [nlists] the list's record in that batch
    size_t nlists = 0;
    int64_t *stats_dev = nullptr, *stats_host = nullptr;  // [3] lists deferred | member pairs scored | updates left waiting (sums)
    pgv::DBuf rec, links, ids, pa, pb, tri, mm, loc, sel;
    int nrec = 0, nq = 0, lcap = 0;
    int64_t npairs = 0;   // of the batch prepared last
    bool prepared = false;
    // where the pieces of `rec` / `links` / `sel` are (set by prepare)
    int32_t *rec_owner = nullptr, *rec_lc = nullptr, *rec_nstart = nullptr, *rec_from = nullptr, *rec_wait = nullptr,
            *rec_list = nullptr;
    int64_t *rec_off = nullptr, *rec_pos = nullptr, *ids_start = nullptr, *pair_start = nullptr, *mm_start = nullptr,
            *totals = nullptr;
    int *rec_fill = nullptr, *blocked = nullptr, *nrec_dev = nullptr;
    int32_t *d_link_elem = nullptr;
    float *d_link_dist = nullptr;
    int32_t *d_sel_ids = nullptr, *d_sel_cnt = nullptr, *d_elems = nullptr;
    float *d_sel_dist = nullptr;
    uint8_t *d_sel_closer = nullptr, *d_linked = nullptr;
    // pgv_hnsw_build_search_keep: the candidate lists of two batches (ids | distances | counts; elements | insert levels)
    struct Kept {
        pgv::DBuf ids, dist, cnt, elems;
        int nq = 0, ef = 0, lcap = 0;
    } kept[2];
};

namespace pgv {

// How far an MFMA L2 value a = |x|^2 - 2 q.x can be from the true s = |x|^2 - 2 q.x of the same pair (the distance
// less |q|^2, which shifts all values of a query alike), and what the candidate selection must allow for.
//
// ScanBound -- the list scan / center ranking / exact top-k (mfma_scan_kernel + batch_recheck_kernel):
//     eps(q, x) = g_sq (|q| + |x|)^2  +  g_dot 2 |q||x|  +  g_norm |x|^2 ,      band = a_k + 2 eps + g_ref |a_k + 2 eps + |q|^2|
//   statistical    g_sq = 8 sqrt(dim + 4) u, the rest 0: the probabilistic bound of a length-dim fp32 summation (Higham &
//                  Mary 2019: lambda sqrt(n) u fails with probability ~ exp(-lambda^2 / 2) per sum, lambda = 8), u = 2^-24
//   worst case     deterministic (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1 / eq. 3.5: a sum of n
//                  rounded products in ANY order errs by at most gamma_n sum |a_i b_i|, gamma_n = n u / (1 - n u)), with
//                  u = 2^-24 per operation: the matrix pipeline rounds products and accumulator additions to nearest,
//                  which tests/test_gpu_round4.py pins on the hardware (half-way cases through both MFMA shapes);
//                  which element joins which chain in what order, in every form, is restated by tests/chain_model.py
//                  and pinned bit for bit (fp32) by tests/test_gpu_scan_band.py and tests/mp_scan_band_worker.py, which
//                  also attack the band with rows whose error reaches ~0.9 of the g_dot term in either direction:
//                    g_dot   gamma_(chain + 4): the kernel keeps FOUR independent accumulators per output, each adds at
//                            most `chain` products (Cauchy-Schwarz: sum |q_i x_i| <= |q||x|), at most three more
//                            additions join them and the final fma(-2, dot, |x|^2) rounds once.  `chain` is
//                            scan_chain_length() / dense_chain_length(): dim / 4 for fp32 rows in the four-chain forms;
//                            for fp16 rows a chain takes whole instructions of 16 (32-query form) or 32 (16-wide form:
//                            chain c + 2 x slice parity) products, so with S = ceil(dim / 64) slices it holds up to
//                            max(16 S, 32 ceil(S / 2)) of them -- 32 at 64-d, where dim / 4 would say 16; the 64-query
//                            form and mfma_dense_kernel keep quarters of whole slices (32 or 64 products each)
//                    g_norm  gamma_(dim/64 + 10): row_norms_kernel's per-lane chains of dim / 64 fmas + 6 shuffle
//                            additions, + the final fma
//                    g_ref   2 gamma_(dim + 2): the exact form sum((q - x)^2) that decides among the candidates (here
//                            and in the reference) is itself rounded -- all terms positive, so RELATIVE to the distance;
//                            a row outside the band must stay outside when both its and the k-th row's exact values move
//                  |x| is the largest row norm of the index (one word, kept with the norms).
// ArgminBound -- the build's L2 pre-filter (mfma_argmin_kernel, ONE accumulator chain per output: 128 accumulators a
//   lane leave no room for four): gamma (|c|^2 + 2 |a||c|) + gamma_x d, DETERMINISTIC by default since round 6:
//   gamma = gamma_(dim+1), 5-10 x wider than the statistical 8 sqrt(dim + 4) u.  What made that affordable is not a
//   tighter band but cheaper ambiguity: a row's merged list carries kWide = 8 candidates and `dropped`, the smallest value
//   no list kept (keep_best), so the exact recheck evaluates whatever lies inside the band and only a row whose band holds
//   MORE than the lists do (its 8th value or `dropped` inside it) goes to the all-centers exact kernel -- round 5 sent
//   every row whose 4th value was inside (10 % of 3072-d rows: 32 -> 123 ms).  Measured (profiles/r06/assign_bounds.md):
//   worst case over statistical +4 % (1 M x 1000 x 1536 fp32), +10 % (1.25 M x 4096 x 3072 fp16), redo 0 - 0.06 %.
//   One unit roundoff per product of the chain is what the bound charges; tools/mfma_numerics.py shows the fp32 matrix
//   instructions to BE an fmaf chain bit for bit and the fp16 ones to lose at most 3.2 u per 16 products on random
//   inputs; swamping inputs (every product half an ulp of the accumulator) reach about 5 u per 16 on an MI355X
//   (profiles/r08_scan_band.md) -- charged: 16 u.
//
// The fp16 residual shadow (kernels_shadow.hip) -- the list scan of an fp32 L2 index over a shadow row
// rho~ = fp16((x - c_l) 2^-s) and a cast query q^ = 2^s_q fp16(q 2^-s_q) computes
//     a = fl(|x|^2 + t) - 2^(1 + s + s_q) acc,   t = fl(-2 q.c_l),   acc = fl(q^' . rho~)
// for the same s = |x|^2 - 2 q.c_l - 2 q.rho (x = c_l + rho).  The band of such a scan is ScanBound {0, 0, g_norm, g_ref}
// (worst-case g_norm: |x|^2 is the fp32 rows' own) plus a PER-QUERY term, computed in fp64 by shadow_query_kernel and
// rounded up into fp32, that covers every other difference between a and s:
//     representation   2 (|q| E + |q - q^| P):  q.rho - q^.(2^s rho~) = q.(rho - 2^s rho~) + (q - q^).(2^s rho~)
//                      (E = max |rho - 2^s rho~|, P = max |2^s rho~|, measured over the index's rows in fp64)
//     matrix cores     g_dot 2 |q^| P, g_dot = gamma_(chain + 4): fp16 products are exact in fp32, each of the four
//                      accumulator chains adds at most `chain` of them (shadow_chain_length; the instructions lose
//                      about 5 u per 16 products at worst, see above, charged u per product), two additions join them
//     pair term        gamma_(pair_chain_length) 2 |q| max|c|; max|c| from center_norms[nlists] (itself within
//                      gamma_(ld / 64 + 10)).  t reaches the scan by one of two routes, and the term covers the longer:
//                        shadow_pair_kernel (pgv_scan_batch; batch_fix_kernel's fill for a flagged ranking query): one
//                          fmaf chain of ceil(ld / 64) elements per lane + 6 shuffle additions: ceil(ld / 64) + 6
//                        batch_recheck_kernel of the ranking (pgv_search_batch; group_distance_dot): 2^lg lanes per row
//                          (RowGeom::lpr_log2), each lane two fmaf chains that take its 16-byte vectors in turn: at most
//                          4 ceil(ceil(nvec / 2^lg) / 2) products, one addition joins the two, lg DPP additions join the
//                          lanes: 4 ceil(ceil(nvec / 2^lg) / 2) + 1 + lg.  The final -2 * (q.c) is exact.
//                      1536-d: 30 by the first route, 19 by the second -- the term does not grow there.  The second is
//                      longer where row_geom puts few lanes on a row (a vector count that does not divide among many
//                      lanes; at most 64 vectors per lane, so never more than 4 * 32 + 1 + 6 = 135): 249-d has 63
//                      vectors on one lane, 129 roundings against 10, and its term grows by 119 u 2 |q| max|c|
//     epilogue         4 u (|x|^2 + |t| + 2 |q^| P): the addition |x|^2 + t and the final fmaf round once each
// and 4 FLT_MIN for whatever underflowed on the way; the 1.001 factor of the scans' eps applies on top.  A query whose
// scale 2^(1 + s + s_q) leaves the normal fp32 range, or whose terms are not finite, gets an infinite term: its band
// holds everything and batch_fix_kernel scores it exactly.
//
// The center shadow -- the batch ranking of such an index multiplies c~ = fp16(c 2^-s_c) and the same cast
// query: a = fl(|c|^2 - 2^(1 + s_c + s_q) acc) for s = |c|^2 - 2 q.c (the dense plan's pairs carry t = 0, so |c|^2 + t is
// exact).  The band is ScanBound {0, 0, g_norm, g_ref} (the fp32 center_norms are the index's own) plus a per-query term
// from the same kernel (RankShadowTerms), derived like the scan's with E_c = max |c - 2^s_c c~|, P_c = max |2^s_c c~|:
//     representation   2 (|q| E_c + |q - q^| P_c)
//     matrix cores     g_dot 2 |q^| P_c, g_dot = gamma_(shadow_chain_length + 4)
//     epilogue         4 u (max |c|^2 + 2 |q^| P_c): the final fmaf rounds once
// There is no pair term.  Nothing in it depends on the data being benign: E_c and P_c are measured, and a query whose
// band swallows all its candidates (maxprobes + 54 under this ranking, rank_lists_impl) goes through batch_fix_kernel as
// under the fp32 ranking.
struct ScanBound {
    float g_sq, g_dot, g_norm, g_ref;
};
struct ShadowTerms {  // shadow_query_kernel's inputs
    int s;
    double E, P;
    double g_dot, g_pair, g_cn;  // g_cn: relative error of the stored largest |x|^2 / |c|^2
};
struct RankShadowTerms {  // ... for the center ranking over the centers' shadow
    int s;
    double E, P;
    double g_dot, g_cn;
};
inline float gamma_n(double n, double v) { return (float)(n * v / (1.0 - n * v)); }
// roundings on the way to a pair term t = -2 q.c_l, whichever route computes it (the paragraph above)
inline int pair_chain_length(const RowGeom &g32) {
    const int by_pair_kernel = (g32.ld + 63) / 64 + 6;
    const int per_lane = (g32.nvec + (1 << g32.lpr_log2) - 1) >> g32.lpr_log2;
    const int by_recheck = 4 * ((per_lane + 1) / 2) + 1 + g32.lpr_log2;
    return by_pair_kernel > by_recheck ? by_pair_kernel : by_recheck;
}
// (the callers go through scan_bound_chain: this is the part that does not depend on the kernel form, and the g_dot of
// fp32 rows in the four-chain forms)
inline ScanBound scan_bound(const pgv_ctx *ctx, int dim) {
    if (ctx->bound_mode == 0) return {8.f * std::sqrt((float)dim + 4.f) * 5.9604645e-8f, 0.f, 0.f, 0.f};
    constexpr double v = 5.9604645e-8;  // 2^-24: round to nearest (tests/test_gpu_round4.py)
    return {0.f, gamma_n(dim / 4.0 + 4.0, v), gamma_n(dim / 64.0 + 10.0, v), 2.f * gamma_n(dim + 2.0, v)};
}
// the same with the products per accumulator chain given (mfma_dense_kernel: quarters of whole 128-byte slices)
inline ScanBound scan_bound_chain(const pgv_ctx *ctx, int dim, int chain) {
    ScanBound b = scan_bound(ctx, dim);
    if (ctx->bound_mode != 0) b.g_dot = gamma_n(chain + 4.0, 5.9604645e-8);
    return b;
}
// the band of the shadow paths (ranking over the center shadow, scan over the row shadow): the stored |x|^2's rounding,
// worst case whatever the bound mode, and the exact form's g_ref; the rest is the per-query term (ceps / qeps).  u: 2^-24
// as the caller writes it (shadow_query_kernel's terms: the exact 5.9604644775390625e-8, another float at some lengths)
inline ScanBound shadow_band(int ld, float g_ref, double u = 5.9604645e-8) {
    return {0.f, 0.f, gamma_n(ld / 64.0 + 10.0, u), g_ref};
}
// Probe pruning (PGV_PROBE_PRUNE) -- a probed list whose every row is provably farther than k rows of the
// lists in front of it is not scanned.  Per list l the index keeps R_l >= max |x - c_l| over its rows (list_radius:
// measured in fp64 where the row shadow is built, rounded up; 0 for an empty list, +inf where not finite).  For one query
// the probed lists come in probe order with d_j, the fp32 sum((q - c_j)^2) in the reference's arithmetic.
//     m     the smallest count such that lists 0 .. m-1 hold >= k rows together (none: nothing is dropped)
//     tau   max over i < m of sqrt(d_i) + R_i
//     probe j >= m is dropped iff sqrt(d_j) - R_j > tau
// Proof.  Write D_j = |q - c_j| (exact).  A row x of list i < m has |q - x| <= D_i + R_i, a row y of list j has
// |q - y| >= D_j - R_j (triangle inequality).  The distances the search orders by are fp32 sums of n = ld squares of
// rounded differences, all terms non-negative: fl = T^2 (1 + e) + e_a with |e| <= g = gamma_(ld + 4) in any order of
// summation (Higham 3.5; the subtraction's and the product's roundings are three of the n + 3), |e_a| <= a = (ld + 4)
// 2^-149 for products that underflowed.  The same holds between d_j and D_j^2.  Hence
//     every row of lists i < m:  fl <= H^2 (1 + g) + a,   H = max_i sqrt((d_i + a) / (1 - g)) + R_i          (probe_near)
//     every row of list j:       fl >= L^2 (1 - g) - a,   L = sqrt(max(d_j - a, 0) / (1 + g)) - R_j, if L > 0 (probe_far)
// and j is dropped only if L^2 (1 - g) - a > (H^2 (1 + g) + a)(1 + 2^-40) in fp64 (the factor covers the fp64 roundings of
// both sides many times over) with the right side below FLT_MAX (no kept row's distance has overflowed into a tie with
// the dropped ones).  Then >= k kept rows have a STRICTLY smaller distance than any row of list j: none of its rows is in
// the head, whatever the order among ties.  With g = a = 0 this is the rule above; the margins only keep more.  Equality
// keeps.  Anything non-finite (a NaN / inf query, an overflowed d, an infinite radius) among the first m lists drops
// nothing for the query; a non-finite far side keeps its list.  tests/prune_model.py is the host model.
#if defined(__HIPCC__)
#define PGV_HD __host__ __device__
#else
#define PGV_HD
#endif
struct ProbeMargins {
    double g = 0.0, a = 0.0;
};
PGV_HD inline ProbeMargins probe_margins(int ld) {  // ld: the fp32 row length
    const double n = (ld + 4.0) * 5.9604644775390625e-8;
    return {n / (1.0 - n), (ld + 4.0) * 1.401298464324817e-45};
}
PGV_HD inline double probe_near(float d, float R, ProbeMargins pm) { return sqrt(((double)d + pm.a) / (1.0 - pm.g)) + (double)R; }
PGV_HD inline double probe_far(float d, float R, ProbeMargins pm) {
    const double e = (double)d - pm.a;
    return sqrt((e > 0.0 ? e : 0.0) / (1.0 + pm.g)) - (double)R;
}
// lens / near [n]: the probed lists' rows and probe_near in probe order (a fill entry: 0 rows, near 0); far: probe_far of
// probe j
PGV_HD inline bool probe_dropped(const int64_t *lens, const double *near, int n, int j, int need, double far, ProbeMargins pm) {
    int64_t rows = 0;
    double tau = 0.0;
    bool finite = true;
    int m = 0;
    while (m < n && rows < need) {
        rows += lens[m];
        const double h = near[m];
        finite = finite && h < (double)INFINITY;  // (false for NaN)
        tau = h > tau ? h : tau;
        m++;
    }
    if (rows < need || j < m || !finite) return false;
    if (!(far > 0.0) || !(far < (double)INFINITY)) return false;
    const double lo2 = far * far * (1.0 - pm.g) - pm.a, hi2 = tau * tau * (1.0 + pm.g) + pm.a;
    return hi2 < 3.0e38 && lo2 > hi2 * (1.0 + 9.094947017729282e-13);
}

struct ExpansionBound {
    float gamma;        // of |x|^2 + 2 |q||x| (expansion terms)
    float gamma_exact;  // of (|q| + |x|)^2 (the exact value's own rounding; 0 in the statistical model)
};
inline ExpansionBound argmin_bound(const pgv_ctx *ctx, int dim) {
    constexpr float u = 5.9604645e-8f;
    if (ctx->assign_bound_mode == 0) return {8.f * std::sqrt((float)dim + 4.f) * u, 0.f};
    const float n1 = (float)(dim + 1) * u, n2 = (float)(dim + 2) * u;
    return {n1 / (1.f - n1), n2 / (1.f - n2)};
}

// ---------------------------------------------------------------- launchers
// kernels_scan.hip: stream rows, score them against small groups of queries
int launch_scan(pgv_ctx *ctx, const RowsView &v, const void *queries, const ScanWork &w, int qt, float *out);
int scan_group_size(const RowGeom &g, pgv_dtype dtype, int wanted);
// gathered variant (HNSW candidate scoring): pair i = (slot[i], query_of[i])
int launch_score_gather(pgv_ctx *ctx, const RowsView &v, const void *queries, const int32_t *slot, const int32_t *query_of,
                        int64_t npairs, float *out);
// the pairs (u, v < u), u >= from, inside groups of rows, in 4 x 4 tiles (bit for bit score_gather's values; fp32 / fp16
// rows only).  Group g is ids[ids_at[g] ..) (ids_at NULL: g * ids_stride), n_arr[g] rows (NULL: ids_at[g + 1] - ids_at[g]),
// from_arr[g] (NULL: 1); its pairs go to out[pair_at[g] ..), u ascending then v; pair_at[g + 1] == pair_at[g]: nothing wanted
int launch_score_groups(pgv_ctx *ctx, const RowsView &v, const int32_t *ids, const int64_t *ids_at, int64_t ids_stride,
                        const int32_t *n_arr, const int32_t *from_arr, const int64_t *pair_at, int ngroups, float *out);
// kernels_hnsw.hip: the same groups' pairs written out as the (slot, query_of) arrays of launch_score_gather, in the
// order launch_score_groups writes their values: a[] = slot of u, b[] = slot of v
int launch_expand_groups(pgv_ctx *ctx, const int32_t *ids, const int64_t *ids_at, int64_t ids_stride, const int32_t *n_arr,
                         const int32_t *from_arr, const int64_t *pair_at, int ngroups, int32_t *a, int32_t *b);

// kernels_misc.hip: operator-path cosine distance and bit-vector distances, one query x n rows
int launch_cosine(pgv_ctx *ctx, pgv_dtype dtype, const RowGeom &g, const void *rows, const void *query, int64_t n,
                  double *out);
int launch_bit_distance(pgv_ctx *ctx, int mode, const RowGeom &g, const void *rows, const void *query, int64_t n,
                        double *out);

// kernels_bit.hip: binary quantization.  The Hamming distances of every query x every row in 256-row x 32-query tiles
// (pgv_bit_topk): bit rows, queries [nq x qbytes] with qbytes a multiple of bit_topk_slice_bytes() (bit_query_bytes of
// the rows' length, or more), both zero padded; out[q * n + row]
int bit_topk_slice_bytes();
inline int bit_query_bytes(int nbits) {
    const int slice = bit_topk_slice_bytes();
    return ((nbits + 7) / 8 + slice - 1) / slice * slice;
}
int launch_hamming_tiles(pgv_ctx *ctx, const RowsView &v, const void *queries, int qbytes, int nq, float *out);
// the list scan of a bit index (pgv_index::nbits): the plan of launch_plan_batch with 256 rows per task and qt queries per
// group (hamming_list_group_size), the same rows and queries as launch_hamming_tiles; out[pair.out_rel + row]
int hamming_list_group_size(double queries_per_list);
int hamming_list_rows_per_task();
int launch_hamming_lists(pgv_ctx *ctx, const RowsView &v, const void *queries, int qbytes, const ScanWork &w, int qt,
                         float *out);
// the bit k-means' build side.  launch_bit_closest: row j of a chunk's distance matrix mat[j * k + c] (launch_hamming_tiles
// with the samples as queries) and its first minimum (best_val / best_pos, launch_topk_segments with k = 1) -> closest_io[j]:
// sticky and closest_io[j] >= 0: the current center unless best_val is strictly smaller; else best_pos.  counts[new] += 1,
// *changes += (new != old), out_dist[j] = the distance to the result (each may be null)
int launch_bit_closest(pgv_ctx *ctx, const float *mat, int k, const float *best_val, const int64_t *best_pos, int n,
                       bool sticky, int32_t *closest_io, float *out_dist, int32_t *counts, unsigned long long *changes);
// sums[c * nbits + i] += 1 per sample of center c with bit i set (BitSumCenter, src/ivfutils.c:363-370); sums start zero
int launch_bit_sums(pgv_ctx *ctx, const void *samples, int ld, int nbits, int n, const int32_t *closest, int32_t *sums);
// BitUpdateCenter (src/ivfutils.c:325-339) over sums / counts; a cluster with refill_row[c] >= 0 takes that packed row of
// `refill` [.. x (nbits + 7) / 8] instead.  centers: [k x ld] bytes, zero padded
int launch_bit_centers(pgv_ctx *ctx, const int32_t *sums, const int32_t *counts, int k, int nbits, int ld,
                       const int32_t *refill_row, const uint8_t *refill, void *centers);
// rows [n x dim] tightly packed -> out_bits [n x (dim + 7) / 8], bit i = x[i] > 0, first element in the top bit
int launch_binary_quantize(pgv_ctx *ctx, pgv_dtype dtype, int dim, const void *rows, int64_t n, void *out_bits);
// pgv_rerank around launch_score_gather and launch_topk_segments: cand [nq x kc] -> packed [nq x kc], each query's real
// candidates in front in their order and -1 behind them, and the (slot, query_of) of the packed pairs (-1: row 0); NaN
// over the values of the -1 entries, so that the selection takes every real candidate first; selected positions ->
// packed entries, +inf / -1 where the selection reached the -1 tail
int launch_rerank_pairs(pgv_ctx *ctx, const int64_t *cand, int nq, int kc, int64_t *packed, int32_t *slot, int32_t *query_of);
int launch_rerank_mask(pgv_ctx *ctx, const int64_t *packed, int64_t total, float *vals);
int launch_rerank_map(pgv_ctx *ctx, const int64_t *packed, int nq, int kc, int k, const int64_t *pos, int64_t *out_idx,
                      float *out_dist);

// kernels_sparse.hip: the sparsevec distances of a tile of queries against every row, both CSR on the device
struct SparseCsr {
    const int64_t *ptr;  // [n + 1]
    const int32_t *idx;  // [ptr[n]] ascending inside a vector
    const float *val;    // [ptr[n]]
    int64_t n;
};
// a run of consecutive queries a workgroup stages in LDS: queries [q0, q0 + nq), their nnz stored elements from elem0
struct SparseTile {
    int64_t elem0;
    int32_t q0, nq, nnz, pad;
};
int sparse_tile_nnz();      // stored elements a tile of several queries holds at most (a longer query is its own tile)
int sparse_tile_queries();  // queries of a tile at most
int sparse_reg_row_nnz();   // rows up to this many stored elements are read once per tile, longer ones once per query
// q_ptr: host, validated; the tiles of queries [0, nq) in order and the longest query's stored elements
void sparse_plan_tiles(const int64_t *q_ptr, int nq, std::vector<SparseTile> *tiles, int *max_q_nnz);
// mode 0 L2 squared | 1 negative inner product | 2 L1: float out[q * out_stride + row], q counting from q.ptr's first
// query; mode 3 cosine distance (one tile of one query): double out[row].  max_*: over the tiles, for the LDS size
int launch_sparse_tiles(pgv_ctx *ctx, int mode, const SparseTile *tiles_dev, int ntiles, int max_tile_nnz, int max_tile_nq,
                        int max_q_nnz, const SparseCsr &q, const SparseCsr &r, void *out, int64_t out_stride);
// elem[i] = (idx[i], val[i]), 8 bytes each: how a sparse HNSW mirror keeps its rows and its pair scorer takes queries
int launch_sparse_pack(pgv_ctx *ctx, const int32_t *idx, const float *val, int64_t total, void *elem);
// pair i = (row slot[i] of the sparse rows v, query query_of[i] -- NULL: query 0 -- of the packed queries q_ptr / q_elem): the
// values of launch_sparse_tiles for the same two vectors, bit for bit
int launch_sparse_pairs(pgv_ctx *ctx, const RowsView &v, const int64_t *q_ptr, const void *q_elem, const int32_t *slot,
                        const int32_t *query_of, int64_t npairs, float *out);
// launch_score_groups over sparse rows (the same arguments and output order): pair {a, b} of element slots is
// launch_sparse_pairs' value for (row min(a, b), query max(a, b)), bit for bit -- the build's orientation rule
int launch_sparse_groups(pgv_ctx *ctx, const RowsView &v, const int32_t *ids, const int64_t *ids_at, int64_t ids_stride,
                         const int32_t *n_arr, const int32_t *from_arr, const int64_t *pair_at, int ngroups, float *out);
// (a[i], b[i]) -> (min, max) in place: slot pairs as the rule above takes them (PGV_HNSW_PAIRS_GATHER=1 over sparse rows)
int launch_sparse_orient_pairs(pgv_ctx *ctx, int32_t *a, int32_t *b, int64_t npairs);

// kernels_hnsw.hip: the whole first batch of an HNSW scan, one workgroup per query
int hnsw_search_grid(pgv_ctx *ctx, int nq, int64_t n, int *words_out);
struct HnswSearchArgs {
    const void *queries = nullptr;     // staged query rows, or
    SparseCsr sparse_queries{nullptr, nullptr, nullptr, 0};  // the staged queries of a walk over sparse rows, and
    int max_q_nnz = 0;                 // ... the longest one's stored elements (the launch's LDS is sized by it), or
    const int32_t *qids = nullptr;     // element slots used as queries (build; over sparse rows max_q_nnz is then the
                                       // mirror's longest ELEMENT)
    const int32_t *qlevels = nullptr;  // insert level per query (build)
    int nq = 0, ef = 0, k = 0;
    int64_t *out_elem = nullptr;
    float *out_dist = nullptr;
    int64_t *out_scored = nullptr;
    int32_t *lw_ids = nullptr;         // per-layer W (build)
    float *lw_dist = nullptr;
    int32_t *lw_cnt = nullptr;
    int lcap = 0;
};
// ... and a resumable scan's state on top (pgv_hnsw_scan_*): with it the launch is one batch of every wanted query --
// the first (GetScanItems) or a resumed one (ResumeScanItems, src/hnswscan.c:61-87) -- or the drain of their pools.
// bitmaps / words are then the scan's: one visited set per QUERY.  k = ef; query rows, or over sparse rows sparse_queries
// (the scan's own copy) with max_q_nnz the longest query of the SCAN: every batch carves the same LDS, whatever it wants
constexpr size_t kHnswScanQueryBytes = 16;  // per query: tuples so far, live pool entries, flags
struct HnswScanArgs {
    void *pool = nullptr;              // [nq x cap] (key, element) pairs: the discarded candidates, in discard order
    int cap = 0;
    void *qstate = nullptr;            // [nq x kHnswScanQueryBytes], zero before the first batch
    const uint8_t *want = nullptr;     // [nq] or NULL = every query
    int32_t *out_count = nullptr;      // [nq]
    int64_t *out_left = nullptr;       // [nq] or NULL
    int *overflow = nullptr;           // zero before the first batch; 1 + a query whose pool overflowed
    bool drain = false;
    // pgv_hnsw_scan_filtered: hnswgettuple's whole loop per query in this one launch (then k is the width of the output
    // rows, 1..4096, and need not be ef; drain stays false: the loop drains by itself once so->tuples >= max_scan_tuples)
    bool filtered = false;
    const uint32_t *keep = nullptr;    // element e: bit e & 31 of word e >> 5; NULL keeps every element
    int64_t keep_stride = 0;           // words from one query's bitmap to the next; 0: one bitmap shared by all
    int64_t max_scan_tuples = 0;
    bool strict = false;
    int32_t *out_batches = nullptr;    // [nq] or NULL
};
int launch_hnsw_search(pgv_ctx *ctx, const RowsView &v, const HnswGraph &graph, const HnswSearchArgs &a, uint32_t *bitmaps,
                       int words, int grid, int *counter, const HnswScanArgs *scan = nullptr);
// PGV_ERR_ARG (the text: who, ef, m, the query length) when a scan over sparse rows would need more LDS than a workgroup
// has: what launch_hnsw_search checks at every batch, for pgv_hnsw_scan_begin_sparse to refuse at once
int hnsw_sparse_scan_lds_check(const char *who, pgv_metric metric, int ef, int m, int max_q_nnz);
int launch_hnsw_patch(pgv_ctx *ctx, const HnswGraph &graph, int64_t n, const int32_t *ids, const int64_t *packed_off,
                      const int32_t *packed, int nupd);

// kernels_hnsw_repair.hip: hnswvacuum's repair search (HnswFindElementNeighbors with existing = true) over a dense mirror
// with dead elements, one workgroup per element; W holds ef_construction + 1 + dead_cap entries.  All device arrays
struct HnswRepairArgs {
    const int32_t *qids = nullptr;  // [nq] the elements being repaired
    int nq = 0, ef_construction = 0, dead_cap = 0, lcap = 0;
    int32_t *lw_ids = nullptr;      // [nq x lcap x (ef_construction + 1 + dead_cap)] every searched layer's stripped W
    float *lw_dist = nullptr;
    int32_t *lw_cnt = nullptr;      // [nq x lcap]
    int32_t *qlevels = nullptr;     // [nq] out: each element's level
    int32_t *status = nullptr;      // [nq] out: 1 = W overflowed, the element's counts are 0
};
// PGV_ERR_ARG (the text: who, ef, dead_cap, m, the bytes) when W does not fit a workgroup's LDS; the largest dead_cap that
// does (-1: not even dead_cap 0)
int hnsw_repair_lds_check(const char *who, const RowGeom &geom, int ef_construction, int dead_cap, int m, size_t *lds_out);
int hnsw_repair_dead_cap_max(const RowGeom &geom, int ef_construction, int m);
int launch_hnsw_repair(pgv_ctx *ctx, const RowsView &v, const HnswGraph &graph, const uint32_t *live, const HnswRepairArgs &a,
                       uint32_t *bitmaps, int words, int grid, int *counter);

// kernels_tile.hip: row tiles in LDS (async DMA), queries in registers: 16 queries per pass
bool tile_scan_supported(const RowGeom &g);
int tile_scan_queries_per_task();
int tile_scan_tile_rows(const RowGeom &g);
int launch_tile_scan(pgv_ctx *ctx, const RowsView &v, const void *queries, const ScanWork &w, float *out);

// kernels_pair.hip: n rows x k centers, both large: argmin per row
int launch_argmin(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, const RowGeom &g,
                  const void *rows, int64_t n, const void *centers, int k, int32_t *out_idx,
                  float *out_val);
// mode 0..2 = pgv_metric, 3 = spherical k-means (-clamp(ip))
int launch_argmin_mode(pgv_ctx *ctx, int mode, pgv_dtype dtype, const RowGeom &g,
                       const void *rows, int64_t n, const void *centers, int k,
                       int32_t *out_idx, float *out_val);

int launch_argmin_listed(pgv_ctx *ctx, int mode, pgv_dtype dtype, const RowGeom &g, const void *rows, int64_t n,
                         const void *centers, int k, const int32_t *row_list, const int *row_count,
                         unsigned long long *packed);
// kernels_hnsw.hip: SelectNeighbors of a batch's new elements on the device (plan -> score_groups, or expand_groups +
// score_gather -> sweep)
int launch_hnsw_select_plan(pgv_ctx *ctx, const int32_t *cnt, int ngroups, int lcap, int m, int64_t *pair_start);
int launch_hnsw_select(pgv_ctx *ctx, const int32_t *lw_ids, const float *lw_dist, const int32_t *cnt, const int32_t *qlevels,
                       const int64_t *pair_start, const float *tri, int ngroups, int lcap, int ef, int m, int stride,
                       int32_t *out_ids, float *out_dist, uint8_t *out_closer, int32_t *out_cnt);
// kernels_hnsw_link.hip: a batch linked into the neighbor lists it chose, on the device
int launch_hnsw_link_group(pgv_ctx *ctx, int step, const HnswGraph &graph, const int32_t *elems, const uint8_t *linked, int nq,
                           int lcap, const int32_t *sel_ids, const float *sel_dist, const int32_t *sel_cnt, int *list_count,
                           int *list_rec, int *nrec, int32_t *rec_owner, int32_t *rec_lc, int32_t *rec_list,
                           const int64_t *rec_off, int *rec_fill, int32_t *link_elem, float *link_dist);
int launch_hnsw_link_size(pgv_ctx *ctx, const HnswGraph &graph, const uint8_t *nb_flag, const int32_t *rec_owner,
                          const int32_t *rec_lc, const int32_t *rec_list, const int *list_count, int64_t *rec_off, int nrec,
                          int pass, int64_t *rec_pos, int32_t *rec_nstart, int32_t *rec_from, const int32_t *rec_wait,
                          int64_t *size_ids, int64_t *size_pairs);
int launch_hnsw_link_scan(pgv_ctx *ctx, int64_t *a, int64_t *b, int64_t *c, int n, int64_t *totals);
int launch_hnsw_link_stats(pgv_ctx *ctx, const int *blocked, const int64_t *totals, int64_t *stats);
int launch_hnsw_link_pairs(pgv_ctx *ctx, const int32_t *nbr, const int64_t *rec_pos, const int32_t *rec_nstart,
                           const int32_t *rec_from, const int64_t *rec_off, int32_t *link_elem, float *link_dist,
                           const int32_t *rec_list, int *list_count, int nrec, int pass,
                           const int64_t *ids_start, int32_t *ids, const int64_t *pair_start, int32_t *a, int32_t *b);
int launch_hnsw_link_replay(pgv_ctx *ctx, const HnswGraph &graph, float *nb_dist, uint8_t *nb_flag, int nrec, int pass,
                            const int32_t *rec_lc, const int64_t *rec_off, const float *link_dist, const int64_t *rec_pos,
                            const int32_t *rec_nstart, const int32_t *rec_from, const int64_t *ids_start, const int32_t *ids,
                            const int64_t *pair_start, const float *tri, const int64_t *mm_start, const float *mm,
                            int32_t *rec_wait, int16_t *loc_save, int *blocked);
int launch_hnsw_link_new(pgv_ctx *ctx, const HnswGraph &graph, float *nb_dist, uint8_t *nb_flag, const int32_t *elems,
                         const uint8_t *linked, int nq, int lcap, const int32_t *sel_ids, const float *sel_dist,
                         const uint8_t *sel_closer, const int32_t *sel_cnt);
// kernels_mfma.hip: the same on the matrix cores (ip / spherical directly, L2 as pre-filter + exact recheck)
bool mfma_argmin_supported(int mode, int64_t n, int k);
int launch_argmin_mfma(pgv_ctx *ctx, int mode, pgv_dtype dtype, const RowGeom &g, const void *rows, int64_t n,
                       const void *centers, int k, int32_t *out_idx, float *out_val);

// kernels_mfma.hip: the batched list scan on the matrix cores (<= 128 rows x <= 32 queries per task)
int mfma_scan_rows_per_task();
int mfma_scan_queries_per_task();
// kernels_dense.hip: every query x every row, 128 x 128 tiles (pgv_exact_topk); out[q * out_stride + row]
int launch_mfma_dense(pgv_ctx *ctx, pgv_metric metric, pgv_dtype dtype, const RowGeom &g, const void *rows, int64_t n,
                      const void *queries, int nq, const float *row_norms, float *out, int64_t out_stride);
int dense_chain_length(const RowGeom &g, pgv_dtype dtype);  // products per accumulator chain, at most
int launch_row_norms(pgv_ctx *ctx, const RowsView &v, float *out, unsigned *max_bits);
int launch_mfma_scan(pgv_ctx *ctx, const RowsView &v, const void *queries, const ScanWork &w, const float *row_norms,
                     const float *query_norms, float *out, bool stream_rows, int queries_per_task = 32,
                     const float *shadow_scale = nullptr);
// kernels_shadow.hip: the fp16 residual shadow of an fp32 L2 index (pgv_index::shadow) and its per-batch terms.
// words: 24 device bytes, [0] bits of the largest |x_i - c_i|, [8] / [16] bits of the largest E^2 / P^2 (fp64)
int launch_shadow_build(pgv_ctx *ctx, const RowGeom &g32, const RowGeom &g16, const void *rows, const void *centers,
                        const int64_t *list_off, int nlists, int64_t n, void *shadow, void *words,
                        void *radius_bits = nullptr);
int shadow_scale_of(float max_abs);  // s of the largest |x_i - c_i|
int shadow_chain_length(const RowGeom &g16);  // kernels_mfma.hip: products per accumulator chain of any scan form, at most
int scan_chain_length(const RowGeom &g, pgv_dtype dtype, bool wide);  // ... of a plain scan: the forms a launch may use
// (qscale / qeps: the list scan's factors and band terms, cscale / ceps: the center ranking's; either pair may be null)
int launch_shadow_query(pgv_ctx *ctx, const RowGeom &g32, const RowGeom &g16, const void *queries, int nq,
                        const ShadowTerms &st, const RankShadowTerms &rt, const float *center_norm_max,
                        const float *row_norm_max, void *qcast, float *qscale, float *qeps, float *cscale, float *ceps);
int launch_shadow_pairs(pgv_ctx *ctx, const RowGeom &g32, const void *queries, const void *centers,
                        const int64_t *pair_start, int nlists, int64_t npairs, ScanPair *pairs);
int mfma_scan_queries_per_task_wide();  // 64: tasks of the batches whose lists are probed by many queries each

// kernels_build.hip: rows of 32-bit words gathered by index (the HNSW mirror's per-element payload)
int launch_gather_words(pgv_ctx *ctx, const void *src, int words_per_row, int64_t nrows, const int64_t *idx, int n,
                        uint32_t *out);
// kernels_build.hip: the build's tuplesort on the device (order by list, heap order inside; gather)
size_t build_sort_scratch_bytes(int64_t n, int key_bits);
int launch_build_order(pgv_ctx *ctx, const int32_t *lists, int64_t n, int nlists, unsigned long long *keys_tmp,
                       unsigned long long *keys_sorted, unsigned long long *counts, int64_t *offsets, int *bad,
                       void *sort_scratch, size_t sort_scratch_bytes);
int launch_build_gather(pgv_ctx *ctx, const void *src_rows, const unsigned long long *keys_sorted, int64_t n, int nvec,
                        void *dst_rows, const uint64_t *src_tids, uint64_t *dst_tids);

// kernels_select.hip: planning + top-k selection
struct PlanResult {
    ScanTask *tasks = nullptr;
    ScanPair *pairs = nullptr;
    int *ntasks_dev = nullptr;
    int64_t ntasks = 0;           // exact when the totals were read back, else the bound
    int64_t total_out = 0;        // sum of the queries' segment lengths (exact or bound, likewise)
    int64_t ntasks_bound = 0;
    int64_t out_bound = 0;
    int64_t *seg_start = nullptr; // device [nq + 1]
    int64_t *probe_off = nullptr; // device [nq x probes]
    int64_t *pair_start = nullptr; // device [nlists + 1]: the first pair of each list
    ScanWork work() const { return {tasks, ntasks_dev, (int)ntasks_bound, pairs}; }
};
// the plan's device scratch of one batch (ctx->plan_a / plan_b, carved)
struct PlanBuffers {
    int *cnt = nullptr, *fill = nullptr;                    // [nlists] queries per list | the pairs' scatter cursors
    int64_t *probe_off = nullptr, *seg_len = nullptr;       // [nq x probes] | [nq]: a query's lists inside its segment
    int64_t *seg_start = nullptr, *pair_start = nullptr, *task_start = nullptr, *totals = nullptr;
};
// sizes and carves them.  launch_plan_batch calls it; pgv_search_batch calls it AHEAD of a ranking whose kernels clear
// and fill cnt / probe_off / seg_len (PlanEmit), so that the buffers do not move in between
int plan_batch_reserve(pgv_ctx *ctx, int nlists, int nq, int probes, PlanBuffers *pb);
// what the ranking's exact tail does of the plan while it emits a query's lists (batch_recheck_kernel<float, true>,
// batch_fix_kernel): cnt[list] += 1 per list emitted, the query's probe_off prefix and seg_len.  cnt == null: nothing
struct PlanEmit {
    int *cnt = nullptr;
    int64_t *probe_off = nullptr, *seg_len = nullptr;
    const int64_t *list_off = nullptr;  // the INDEX's list offsets (the ranking's rows are the centers)
    // probe pruning (the rule above): radius null = off.  A dropped list leaves as -1 with t = 0, counts nothing and has
    // length 0 -- cnt, probe_off and seg_len come out as if it had never been ranked
    const float *radius = nullptr;      // the index's list_radius
    int need = 0;                       // the SEARCH's k (the tail's k is the ranking's maxprobes)
};
// kernels_query.hip: the same rule for probe lists that were given (pgv_scan_batch), one workgroup per query in front of
// the plan: out_lists = the lists with the dropped ones as -1, pair_t = every pair's -2 q.c_l (0 where dropped) by the
// chain of the ranking's recheck.  probes <= probe_prune_max_probes()
int probe_prune_max_probes();
int launch_probe_prune(pgv_ctx *ctx, const pgv_index *ix, const void *q_dev, int nq, const int32_t *probe_lists, int probes,
                       int need, int32_t *out_lists, float *pair_t);
// pair_t: [nq x probes] the pairs' t = -2 q.c_l in probe order (the shadow scan; from the ranking), or null: t = 0
// counted: cnt | fill were cleared and cnt, probe_off and seg_len written by the ranking of this batch (PlanEmit) --
// no memset, no plan_count_kernel, pairs and tasks in one launch, the profiling totals inside plan_scan_kernel
int launch_plan_batch(pgv_ctx *ctx, const pgv_index *ix, const int32_t *probe_lists, int nq,
                      int probes, int qt, int rows_per_task, bool read_totals, PlanResult *res,
                      const float *pair_t = nullptr, bool counted = false);
// zero_word / zero_range[zero_n]: words that kernels LATER in the stream start from zero, cleared here (or null)
// len_bound: with seg_start, a length no segment exceeds, known on the host (a list plan: len_prefix[probes]), or 0.
// It picks the kernel -- small (<= 1024 values), medium (<= 4096) or long -- and nothing else: a segment past its
// class's forms takes the general path.  fixed_len is its own bound
int launch_topk_segments(pgv_ctx *ctx, const float *vals, const int64_t *seg_start, int nseg,
                         int64_t fixed_len, int k, float *out_val, int64_t *out_pos, int32_t *zero_word = nullptr,
                         int32_t *zero_range = nullptr, int zero_n = 0, int64_t len_bound = 0);
int launch_positions_to_slots(pgv_ctx *ctx, const pgv_index *ix, const int32_t *probe_lists,
                              const int64_t *probe_off, int nq, int probes, int k,
                              const int64_t *pos, int64_t *out_slot, uint64_t *out_tid);
// kernels_query.hip: the exact tail of the MFMA L2 scans.  The rows the candidates come
// from: an index's tuples (list_offsets set) or its centers (one dense run)
struct ExactRows {
    const void *vectors;
    const uint64_t *tids;          // or null
    const int64_t *list_offsets;   // or null
    pgv::RowGeom geom;
    pgv_dtype dtype;
    const unsigned *norm_max;      // bits of the largest |row|^2
};
// One tail: the k' smallest approximate values of every query's segment (topk_kernel), their exact distances and the
// first k of them (batch_recheck_kernel), and the queries whose rounding band could not be proven complete start to end
// (batch_fix_kernel).  A query's segment is EITHER its probed lists' rows in probe order (probe_lists set: a list plan) OR
// one dense run of fixed_len rows, the same for every query, whose positions are the row slots (probe_lists null)
struct ExactTail {
    ExactRows rows;                        // the rows the candidates come from
    const void *queries = nullptr;         // [nq] staged query rows, in the rows' format
    int nq = 0;                            // queries
    int kprime = 0;                        // candidates kept per query, k <= k' <= 256
    int k = 0;                             // rows emitted per query
    float *approx = nullptr;               // the expansion's values, segment after segment (a redone query's are overwritten)
    const int32_t *probe_lists = nullptr;  // list plan: [nq x probes] the lists of each query, in probe order
    const int64_t *probe_off = nullptr;    // list plan: [nq x probes] where each list starts inside its query's segment
    int probes = 0;                        // list plan: lists per query
    const int64_t *seg_start = nullptr;    // list plan: [nq + 1] where each query's segment starts in approx
    int64_t seg_bound = 0;                 // list plan: rows no segment exceeds (len_prefix[probes]), or 0: not known
    int64_t fixed_len = 0;                 // dense run: rows per query; approx is [nq x fixed_len]
    ScanBound bound{};                     // the rounding bound of the kernel that produced approx
    const float *eps_add = nullptr;        // [nq] per-query term added to the band (the shadow paths), or null
    float *out_dist = nullptr;             // [nq x k] exact distances, ascending; INFINITY where a segment has fewer rows
    int64_t *out_slot = nullptr;           // [nq x k] row slots (-1: none), or null
    uint64_t *out_tid = nullptr;           // [nq x k] the rows' tids (~0: none), or null
    int32_t *out_i32 = nullptr;            // [nq x k] the slots as int32 (the ranking's list ids), or null
    float *pair_t = nullptr;               // [nq x k] -2 q.row of the rows emitted (fp32 rows only; the ranking), or null
    PlanEmit emit;                         // the plan's counting of the lists emitted (the ranking, with pair_t and out_i32)
    bool dense() const { return probe_lists == nullptr; }
};
// the three launches.  The candidates and the flags are carved from `scratch`; the selection launch also clears what the
// two kernels behind it start from zero: the flagged-query count and, under emit, the plan's cnt | fill
int launch_exact_tail(pgv_ctx *ctx, const ExactTail &t, DBuf &scratch);
int launch_iota_slots(pgv_ctx *ctx, const pgv_index *ix, const int32_t *lists_dev, int nlists,
                      const int64_t *probe_off, int64_t *out_slot);

// kernels_query.hip: one query at a time ([stage,] rank, lists, scan, head: four or five launches, no host round trip)
// ... and the same rank, lists and scan kernels for a few queries at a time, one grid row per query
int query_max_batch_lists();
int query_head_cap();
// The record query_head_kernel writes into pinned host memory and the host reads back: this header, then three arrays
// of `stride` entries each (the count the launch asked for), the widest first so that each stays aligned
struct QueryHead {
    long long total;  // tuples in this batch (= tuplesort's input count)
    int count;        // entries in the arrays: min(asked, what the batch has past `skip`)
    unsigned seq;     // written last (release, system scope): the call this record answers
};
constexpr size_t kQueryHeadArrays = 64;  // the arrays start on the cache line after the header's
static_assert(sizeof(QueryHead) <= kQueryHeadArrays, "the header overtakes the arrays");
inline int64_t *query_head_slots(void *rec) { return reinterpret_cast<int64_t *>(static_cast<char *>(rec) + kQueryHeadArrays); }
inline uint64_t *query_head_tids(void *rec, int stride) { return reinterpret_cast<uint64_t *>(query_head_slots(rec) + stride); }
inline float *query_head_dists(void *rec, int stride) { return reinterpret_cast<float *>(query_head_tids(rec, stride) + stride); }
inline size_t query_head_bytes(int stride) { return kQueryHeadArrays + (size_t)stride * (8 + 8 + 4); }
// floats between the distance rows of consecutive queries (scan segments of `n` rows, center distances of n lists):
// 16-byte aligned rows, each with a float4 of slack behind it for the vector loads of the selection
inline int64_t query_row_stride(int64_t n) { return (n + 7) / 4 * 4; }
int launch_query_stage(pgv_ctx *ctx, const void *src_pinned, void *dst_dev, int nvec);
int launch_query_iota(pgv_ctx *ctx, int32_t *out, int n);
// out[q * out_stride + j] = distance of query q to row j of v (v.n < 2^31): query_rank_kernel's only launcher
int launch_query_rows(pgv_ctx *ctx, const RowsView &v, const void *q_dev, int nq, float *out, int64_t out_stride);
int launch_query_rank(pgv_ctx *ctx, const pgv_index *ix, const void *q_dev, int nq, float *cdist, int64_t cd_stride,
                      int max_probes, int32_t *out_lists, float *out_dist);
int launch_query_scan(pgv_ctx *ctx, const pgv_index *ix, const void *q_dev, int nq, const int32_t *probe_lists,
                      int nprobes, int64_t rows_bound, float *seg, int64_t seg_stride);
int launch_query_head(pgv_ctx *ctx, const pgv_index *ix, const float *seg, const int32_t *probe_lists, int nprobes,
                      int skip, int count, void *head_rec, unsigned seq);
int launch_multi_head(pgv_ctx *ctx, const pgv_index *ix, int nq, const float *seg, int64_t seg_stride,
                      const int32_t *probe_lists, int nprobes, int k, float *out_dist, int64_t *out_slot,
                      uint64_t *out_tid);

int launch_merge_heads(pgv_ctx *ctx, const float *dist_all, const uint64_t *tid_all, int nranks, int nq, int k,
                       float *out_dist, uint64_t *out_tid);

// kernels_select.hip (small helpers)
int launch_cast_pos_to_i32(pgv_ctx *ctx, const int64_t *pos, int64_t n, int32_t *out);

// kernels_kmeans.hip
int kmpp_block_count(int n);
// spherical: 0 raw = L2 squared, 1 raw = negative inner product, 2 raw = the distance itself (Hamming)
int launch_kmpp_update(pgv_ctx *ctx, const float *raw, float *weight, int n, int spherical,
                       double *block_sums);
int launch_kmpp_pick(pgv_ctx *ctx, const RowGeom &g, const void *samples, int n,
                     const float *weight, const double *block_sums, const double *draws,
                     int round, void *centers, int32_t *picked);
int launch_kmpp_total(pgv_ctx *ctx, const double *block_sums, int nblocks, double *out);
int launch_kmpp_pick_sharded(pgv_ctx *ctx, const RowGeom &g, const void *samples, int n, const float *weight,
                             const double *block_sums, const double *totals, const int64_t *counts, int nranks, int rank,
                             const double *draws, int round, void *send_row, int32_t *owner_out);
int launch_kmpp_take_row(pgv_ctx *ctx, const RowGeom &g, const void *gathered, const int32_t *owner, void *centers,
                         int round);
int launch_lloyd_pack(pgv_ctx *ctx, const int32_t *counts, const unsigned long long *changes, int k, float *tail);
int launch_lloyd_unpack(pgv_ctx *ctx, const float *tail, int k, int32_t *counts, unsigned long long *changes,
                        long long *host_rec, long long seq);
int launch_changes_hist(pgv_ctx *ctx, const int32_t *closest_new, int32_t *closest_io, int n,
                        int32_t *counts, unsigned long long *changes);
int launch_members(pgv_ctx *ctx, const int32_t *closest, int n, int k, const int32_t *counts,
                   int32_t *offsets, int32_t *members);
int launch_center_sums(pgv_ctx *ctx, pgv_dtype dtype, const RowGeom &g, const void *samples,
                       const int32_t *offsets, const int32_t *members, int k, float *sums);
int launch_finish_centers(pgv_ctx *ctx, pgv_dtype dtype, const RowGeom &g, int k, int dim,
                          const float *sums, const int32_t *counts, const float *refill,
                          const int32_t *refill_row, void *centers);
int launch_normalize_rows(pgv_ctx *ctx, pgv_dtype dtype, const RowGeom &g, void *rows, int64_t n,
                          int dim, int32_t *flag);
int launch_check_centers(pgv_ctx *ctx, pgv_dtype dtype, const RowGeom &g, const void *centers,
                         int k, int dim, int check_zero_norm, int32_t *flag);

}  // namespace pgv
