// kernels_sparse.hip -- the sparsevec distances on the device: every distance the reference computes as a scalar,
// branchy merge of two sorted index lists,
//   SparsevecL2SquaredDistance   src/sparsevec.c:826-869     (`<->` before its float8 sqrt)
//   SparsevecInnerProduct        src/sparsevec.c:905-936     (`<#>`: negated, :958-966)
//   sparsevec_cosine_distance    src/sparsevec.c:972-1011    (`<=>`)
//   sparsevec_l1_distance        src/sparsevec.c:1018-1060   (`<+>`)
// for a tile of queries against a block of rows, both in CSR (sorted 0-based int32 indices, then float values: what a
// SparseVector datum stores, src/sparsevec.h:22-47).  One kernel, sparse_tile_kernel<MODE>, serves pgv_sparse_topk's
// distance matrix (mat[q * n + row], then launch_topk_segments), pgv_sparse_distance_batch (a tile of one query, out[row])
// and pgv_sparse_cosine_distance_batch (MODE 3, float8 out).
//
// The arithmetic.  Every value is an fp32 sum of exactly the terms the reference adds, each computed
// the way the reference computes it -- (a - b)^2 on a shared index and a^2, b^2 on an index only one side stores (L2),
// a * b on shared indices only (inner product), |a - b|, |a|, |b| (L1), a^2 / b^2 for the cosine norms -- and only the
// ORDER of the additions differs from the reference's index order: lane l of a wavefront adds elements l, l + 64, ..
// of the row, then the unmatched elements l, l + 64, .. of the query, and a 64-lane butterfly finishes the pair.  No
// |a|^2 + |b|^2 - 2ab expansion and no "total minus matched" shortcut, so a vector's L2 / L1 distance to itself is
// exactly 0 and integer-valued data gives the reference's bits.  The order depends on the pair alone, never on the
// tile, the grid or the entry point: pgv_sparse_topk's heads equal pgv_sparse_distance_batch's values bit for bit.
//
// The shape.
//   * a workgroup (4 wavefronts) stages its query tile in LDS once, as (index, value) pairs -- a tile is a run of
//     consecutive queries planned on the host (sparse_plan_tiles): as many as fit kSparseTileNnz = 2048 stored
//     elements (16 KB: eight workgroups, the CU's 32 wavefronts, share its 160 KiB; tiles of 4096, five workgroups a CU,
//     measured 1.7 x slower at 1024 queries, profiles/r21_sparse_topk.md) and at most kSparseTileQueries = 128; a
//     query with more stored elements than that is a tile of its own, up to the reference's 16 000 (128 000 bytes plus
//     8 000 of bitmaps: the raised dynamic-LDS attribute, one workgroup per CU)
//   * each wavefront takes rows of the workgroup's row block (row, row + 4, ..); lanes stride the row's stored
//     elements and binary-search the query's indices in LDS (a branch-free descent whose trip count depends on the
//     query's length alone, so no lane diverges; each step reads the pair, and the last element not above the row's
//     index is kept, so a match and its value are known when the descent ends).  Rows of at most 256 stored elements (kSparseRegChunks chunks of 64)
//     are read from HBM once per TILE and stay in registers across the tile's queries, and their up to four searches
//     per lane descend together; longer rows are read again per query, from the caches, one search after the other
//   * the query-side unmatched terms of L2 and L1 come from a per-wavefront matched bitmap in LDS: cleared, set by
//     the lanes that find their index (LDS atomic or), then swept by the lanes striding the query.  The inner product
//     and the cosine need no bitmap (an index only one side stores adds nothing); the cosine's query norm is summed
//     once per wavefront, not once per row
// HBM traffic per batch: the row CSR (8 bytes per stored element, plus the row pointers) is read once per query TILE,
// i.e. ceil(sum of query nnz / 2048) times at least and nq / 128 times at least; consecutive workgroups share a row
// block and differ in the tile, so the re-reads of a block mostly hit the caches.  The query CSR is read once per
// (tile, row block).
//
// The pair arithmetic itself (QElem, descend, add_term, row_side_*, score_pair) lives in sparse_pair.h: the HNSW walk over
// a sparse mirror (hnsw_sparsevec_support, HNSW_MAX_NNZ 1000, src/hnswutils.c:1361-1433; kernels_hnsw.hip) scores its
// batches with it, and so does sparse_pair_kernel below, which serves pgv_hnsw_score_sparse and pgv_hnsw_score_pairs over
// such a mirror: one wavefront per (element, query) pair, the element row as the walk reads it, the query's elements
// read from the caches (sparse_pack_kernel has laid them side by side).  DESIGN.md 4.6c.  sparse_groups_kernel is the
// build's group scorer over such a mirror (launch_score_groups dispatches to it): the pairs inside a neighbor list, each
// with the element of the smaller slot as the row.
//
// Not here (include/pgv_hip.h says the same): a device-side sparsevec_l2_normalize, ext/ glue; bench.py does not measure
// any of this (tools/bench_sparse_topk.py, tools/bench_sparse_hnsw.py and tools/bench_sparse_hnsw_build.py do).
#include "pgv_device.h"
#include "sparse_pair.h"

namespace pgv {

namespace {

constexpr int kSpThreads = 256;
constexpr int kSpWaves = kSpThreads / kWave;
constexpr int kSparseTileNnz = 2048;     // stored query elements a shared tile holds at most
constexpr int kSparseTileQueries = 128;  // queries of a tile at most
static_assert(kSparseRegChunks == 4, "sparse_tile_kernel instantiates row_side_reg for 1 .. 4 chunks");

// grid: (row blocks) x (tiles), consecutive workgroups sharing a row block.  out: float mat[(q - 0) * out_stride + row]
// for MODE 0..2 (q counts through the launch's queries), double out[row] for MODE 3 (one query)
template <int MODE>
__global__ __launch_bounds__(kSpThreads) void sparse_tile_kernel(
    const SparseTile *__restrict__ tiles, int ntiles, const int64_t *__restrict__ q_ptr, const int32_t *__restrict__ q_idx,
    const float *__restrict__ q_val, const int64_t *__restrict__ r_ptr, const int32_t *__restrict__ r_idx,
    const float *__restrict__ r_val, int64_t n, int rows_per_block, int bm_words, void *__restrict__ out_v,
    int64_t out_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const SparseTile t = tiles[blockIdx.x % (unsigned)ntiles];
    const int64_t row0 = (int64_t)(blockIdx.x / (unsigned)ntiles) * rows_per_block;
    const int64_t row_end = row0 + rows_per_block < n ? row0 + rows_per_block : n;

    // LDS: elem[pad4(nnz)] (index, value) | off[pad4(nq + 1)] | bitmap[waves x bm_words]
    QElem *s_elem = reinterpret_cast<QElem *>(smem);
    int32_t *s_off = reinterpret_cast<int32_t *>(s_elem + pad4(t.nnz));
    uint32_t *bm = reinterpret_cast<uint32_t *>(s_off + pad4(t.nq + 1)) + wave * bm_words;
    for (int i = tid; i < t.nnz; i += kSpThreads) s_elem[i] = {q_idx[t.elem0 + i], q_val[t.elem0 + i]};
    for (int i = tid; i <= t.nq; i += kSpThreads) s_off[i] = (int32_t)(q_ptr[t.q0 + i] - t.elem0);
    __syncthreads();

    float qnorm = 0.f;  // cosine: the query's squared norm, the same for every row
    if (MODE == 3) {
        for (int j = lane; j < s_off[1]; j += kWave) qnorm = __builtin_fmaf(s_elem[j].v, s_elem[j].v, qnorm);
        qnorm = __shfl(group_sum_to_last(qnorm, 6), kWave - 1, kWave);
    }

    for (int64_t r = row0 + wave; r < row_end; r += kSpWaves) {
        const int64_t rb = r_ptr[r];
        const int rn = (int)(r_ptr[r + 1] - rb);
        // side(q's elements, top, a0, a1): the row's share of one pair.  The 64 lanes' sums land in the LAST lane (the same
        // tree for every pair), which stores
        auto pairs = [&](auto side) {
            for (int q = 0; q < t.nq; q++) {
                const int qb = s_off[q], qn = s_off[q + 1] - qb;
                const QElem *qe = s_elem + qb;
                float a0 = 0.f, a1 = 0.f;
                score_pair<MODE>([&](int top) { side(qe, qn, top, a0, a1); }, qe, qn, bm, lane, a0);
                a0 = group_sum_to_last(a0, 6);
                if (MODE == 3) {
                    a1 = group_sum_to_last(a1, 6);
                    if (lane == kWave - 1) {
                        // Use sqrt(a * b) over sqrt(a) * sqrt(b), keep in range (src/sparsevec.c:995-1010); NaN (an empty or
                        // all-zero vector: 0 / 0) passes through both comparisons
                        double similarity = (double)a0 / sqrt((double)qnorm * (double)a1);
                        if (similarity > 1.0)
                            similarity = 1.0;
                        else if (similarity < -1.0)
                            similarity = -1.0;
                        static_cast<double *>(out_v)[r] = 1.0 - similarity;
                    }
                } else if (lane == kWave - 1) {
                    // the negative inner product as 0 - ip: an empty intersection is +0.0 here as it is in the heads the
                    // selection returns (its keys do not tell the two zeros apart)
                    static_cast<float *>(out_v)[(size_t)(t.q0 + q) * (size_t)out_stride + (size_t)r] = MODE == 1 ? 0.f - a0 : a0;
                }
            }
        };
        if (rn <= kSparseRegChunks * kWave) {
            RegRow row;
#pragma unroll
            for (int c = 0; c < kSparseRegChunks; c++) {
                const bool ok = c * kWave + lane < rn;
                row.i[c] = ok ? r_idx[rb + c * kWave + lane] : 0;
                row.v[c] = ok ? r_val[rb + c * kWave + lane] : 0.f;
            }
#define PGV_SPARSE_REG(NC)                                                                                        \
    pairs([&](const QElem *qe, int qn, int top, float &a0, float &a1) {                                           \
        row_side_reg<MODE, NC>(row, rn, qe, qn, top, bm, lane, a0, a1);                                           \
    })
            switch ((rn + kWave - 1) / kWave) {
                case 0:
                case 1: PGV_SPARSE_REG(1); break;
                case 2: PGV_SPARSE_REG(2); break;
                case 3: PGV_SPARSE_REG(3); break;
                default: PGV_SPARSE_REG(4); break;
            }
#undef PGV_SPARSE_REG
        } else {
            pairs([&](const QElem *qe, int qn, int top, float &a0, float &a1) {
                row_side_mem<MODE>(r_idx + rb, r_val + rb, rn, qe, qn, top, bm, lane, a0, a1);
            });
        }
    }
}

// idx[i], val[i] -> elem[i] = (idx[i], val[i]): the element rows of a sparse HNSW mirror and the staged queries of its
// pair scorer
__global__ __launch_bounds__(256) void sparse_pack_kernel(const int32_t *__restrict__ idx, const float *__restrict__ val,
                                                          int64_t total, QElem *__restrict__ elem) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        elem[i] = {idx[i], val[i]};
}

// pair i = (element slot[i] of the mirror, query query_of[i] -- NULL: query 0 -- of the packed queries): one wavefront per pair,
// grid-stride.  The value is score_element's: sparse_tile_kernel's for the same two vectors, bit for bit
template <int MODE>
__global__ __launch_bounds__(kSpThreads) void sparse_pair_kernel(const int64_t *__restrict__ r_ptr, const QElem *__restrict__ r_elem,
                                                                 const int64_t *__restrict__ q_ptr, const QElem *__restrict__ q_elem,
                                                                 const int32_t *__restrict__ slot, const int32_t *__restrict__ query_of,
                                                                 int64_t npairs, float *__restrict__ out) {
    __shared__ uint32_t s_bm[kSpWaves][bitmap_words(kSparseMaxNnz)];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    for (int64_t p = (int64_t)blockIdx.x * kSpWaves + wave; p < npairs; p += (int64_t)gridDim.x * kSpWaves) {
        const int64_t r = slot[p], q = query_of ? query_of[p] : 0;
        const int64_t rb = r_ptr[r], qb = q_ptr[q];
        const int rn = (int)(r_ptr[r + 1] - rb), qn = (int)(q_ptr[q + 1] - qb);
        RegRow row;
        load_reg_row(row, r_elem + rb, rn, lane);
        const float v = score_element<MODE>(row, r_elem + rb, rn, q_elem + qb, qn, s_bm[wave], lane);
        if (lane == kWave - 1) out[p] = v;
    }
}

// Pair distances inside groups of element slots of a sparse HNSW mirror (the build: CheckElementCloser's distances between
// the candidates of one neighbor list, src/hnswutils.c:1040-1059) -- score_groups_kernel's interface and output order:
// group g is the slots ids[at .. at + n), wanted are the pairs (u, v < u) of its locals for u >= from, written u ascending
// then v from pair_at[g] on.
// score_element is not symmetric in its last bit on float data (the row's terms are added first, then the query's
// unmatched ones), and the build compares distances of one pair that reach it by different routes, so a pair has ONE
// orientation here: the element in the smaller SLOT is the row, the one in the larger slot the query -- what the walk's
// build form gives a build that inserts in slot order, and launch_sparse_pairs(a = min, b = max) bit for bit (DESIGN.md
// 4.6g; equal slots, which no list of the build holds, fall to the local order).
// A work item is (group, member c): the workgroup stages element ids[c] in LDS once, as the query, and its wavefronts take
// the partners r of c whose pair is wanted and whose slot is smaller, round-robin in r's order; the value goes where
// (u, v) = (max(c, r), min(c, r)) stands in the output, so every wanted pair is scored exactly once, by the item of its
// larger slot.  A member without such a partner (the smallest slot of its group; every old member of a list that one
// newer element joins) is left before anything is staged: every wavefront counts the partners itself, from the same ids,
// so the four agree without a barrier.  A wavefront requests its next partner's row before it searches the current one,
// like the walk.  grid: x strides the groups, y a group's members.
template <int MODE>
__global__ __launch_bounds__(kSpThreads) void sparse_groups_kernel(
    const int64_t *__restrict__ r_ptr, const QElem *__restrict__ r_elem, const int32_t *__restrict__ ids,
    const int64_t *__restrict__ ids_at, int64_t ids_stride, const int32_t *__restrict__ n_arr,
    const int32_t *__restrict__ from_arr, const int64_t *__restrict__ pair_at, int ngroups, float *__restrict__ out) {
    __shared__ QElem s_q[kSparseHnswMaxNnz];
    __shared__ uint32_t s_bm[kSpWaves][bitmap_words(kSparseHnswMaxNnz)];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t p0 = pair_at[g];
        if (pair_at[g + 1] == p0) continue;
        const int64_t at = ids_at ? ids_at[g] : (int64_t)g * ids_stride;
        const int n = n_arr ? n_arr[g] : (int)(ids_at[g + 1] - at);
        int from = from_arr ? from_arr[g] : 1;
        if (from < 1) from = 1;
        if (n <= from) continue;
        const int32_t *gi = ids + at;
        const int64_t base = (int64_t)from * (from - 1) / 2;
        for (int c = blockIdx.y; c < n; c += gridDim.y) {
            const int32_t ec = gi[c];
            // a pair is wanted when its larger local is >= from: a member below `from` pairs with the locals from there on
            const int r0 = c < from ? from : 0;
            // lane l looks at local rbase + l: is it a partner of c, and which slot does it hold
            auto partner = [&](int rbase, int32_t &er) {
                const int r = rbase + lane;
                er = gi[r < n ? r : n - 1];  // never predicate a load
                return r < n && r != c && (er < ec || (er == ec && r < c));
            };
            int npart = 0;
            for (int rbase = r0; rbase < n; rbase += kWave) {
                int32_t er;
                npart += __popcll(__ballot(partner(rbase, er)));
            }
            if (npart == 0) continue;  // (the same count in every wavefront)
            const int64_t qb = r_ptr[ec];
            const int qn = (int)(r_ptr[ec + 1] - qb);
            __syncthreads();  // the item before this one has been scored: its query may go
            for (int j = tid; j < qn; j += kSpThreads) {
                const QPair raw = *reinterpret_cast<const QPair *>(r_elem + qb + j);
                s_q[j] = {raw.x, __int_as_float(raw.y)};
            }
            __syncthreads();
            int seen = 0;
            for (int rbase = r0; rbase < n; rbase += kWave) {
                int32_t er;
                const bool is = partner(rbase, er);
                const unsigned long long bal = __ballot(is);
                const int rank = seen + __popcll(bal & ((1ull << lane) - 1ull));
                seen += __popcll(bal);
                unsigned long long mb = __ballot(is && (rank & (kSpWaves - 1)) == wave);  // this wavefront's partners
                if (mb == 0ull) continue;
                // a partner is a dependent chain slot -> the row's bounds -> the row's pairs: every lane fetches the bounds
                // of its own local at once
                const int64_t rbl = r_ptr[er];
                const int rnl = (int)(r_ptr[er + 1] - rbl);
                int l = __ffsll(mb) - 1;
                RegRow cur;
                load_reg_row(cur, r_elem + __shfl(rbl, l), __shfl(rnl, l), lane);
                while (mb != 0ull) {
                    l = __ffsll(mb) - 1;
                    mb &= mb - 1ull;
                    const int64_t rb = __shfl(rbl, l);
                    const int rn = __shfl(rnl, l);
                    const int ln = mb != 0ull ? __ffsll(mb) - 1 : l;  // (the last trip asks for its own row again)
                    RegRow nxt;
                    load_reg_row(nxt, r_elem + __shfl(rbl, ln), __shfl(rnl, ln), lane);
                    const float v = score_element<MODE>(cur, r_elem + rb, rn, s_q, qn, s_bm[wave], lane);
                    const int r = rbase + l;
                    const int u = c > r ? c : r, w = c > r ? r : c;
                    if (lane == kWave - 1) out[p0 + (int64_t)u * (u - 1) / 2 - base + w] = v;
                    cur = nxt;
                }
            }
        }
    }
}

// (a[i], b[i]) -> (min, max): the slot pairs expand_groups_kernel / hnsw_link_pairs_kernel emit, oriented as
// sparse_groups_kernel scores them (PGV_HNSW_PAIRS_GATHER=1 over a sparse mirror)
__global__ __launch_bounds__(256) void sparse_orient_pairs_kernel(int32_t *__restrict__ a, int32_t *__restrict__ b, int64_t npairs) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * 256) {
        const int32_t x = a[i], y = b[i];
        if (x > y) {
            a[i] = y;
            b[i] = x;
        }
    }
}

}  // namespace

int sparse_tile_nnz() { return kSparseTileNnz; }
int sparse_tile_queries() { return kSparseTileQueries; }
int sparse_reg_row_nnz() { return kSparseRegChunks * kWave; }

// consecutive queries into tiles: as many as fit kSparseTileNnz stored elements and kSparseTileQueries queries; a longer
// query alone.  q_ptr: host, monotone, every query within kSparseMaxNnz (the caller has checked)
void sparse_plan_tiles(const int64_t *q_ptr, int nq, std::vector<SparseTile> *tiles, int *max_q_nnz) {
    tiles->clear();
    *max_q_nnz = 0;
    for (int q = 0; q < nq;) {
        SparseTile t{q_ptr[q], q, 0, 0, 0};
        while (q < nq && t.nq < kSparseTileQueries) {
            const int qn = (int)(q_ptr[q + 1] - q_ptr[q]);
            if (t.nq > 0 && t.nnz + qn > kSparseTileNnz) break;
            t.nnz += qn;
            t.nq++;
            q++;
            if (qn > *max_q_nnz) *max_q_nnz = qn;
        }
        tiles->push_back(t);
    }
}

template <int MODE>
static int launch_sparse_tiles_t(pgv_ctx *ctx, const SparseTile *tiles_dev, int ntiles, size_t lds, int bm_words,
                                 const SparseCsr &q, const SparseCsr &r, void *out, int64_t out_stride) {
    // enough workgroups for every CU to hold several, blocks long enough to amortise staging the tile
    int64_t rows_per_block = (r.n * ntiles + (int64_t)ctx->num_cus * 16 - 1) / ((int64_t)ctx->num_cus * 16);
    rows_per_block = (rows_per_block + kSpWaves - 1) / kSpWaves * kSpWaves;
    if (rows_per_block < 32) rows_per_block = 32;
    if (rows_per_block > 1024) rows_per_block = 1024;
    const int64_t grid = (r.n + rows_per_block - 1) / rows_per_block * ntiles;
    if (grid > 0x7fffffff) PGV_FAIL(PGV_ERR_ARG, "sparse scan: too many tiles");
    auto kern = sparse_tile_kernel<MODE>;
    if (lds > 64 * 1024)
        PGV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kSpThreads), lds, ctx->stream, tiles_dev, ntiles, q.ptr, q.idx, q.val,
                       r.ptr, r.idx, r.val, r.n, (int)rows_per_block, bm_words, out, out_stride);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_sparse_tiles(pgv_ctx *ctx, int mode, const SparseTile *tiles_dev, int ntiles, int max_tile_nnz, int max_tile_nq,
                        int max_q_nnz, const SparseCsr &q, const SparseCsr &r, void *out, int64_t out_stride) {
    if (r.n <= 0 || ntiles <= 0) return PGV_OK;
    if (max_q_nnz > kSparseMaxNnz || max_tile_nnz > kSparseMaxNnz || max_tile_nq > kSparseTileQueries)
        PGV_FAIL(PGV_ERR_ARG, "sparse scan: a tile of %d queries / %d elements is over the kernel's limits", max_tile_nq,
                 max_tile_nnz);
    const int bm_words = (mode == 0 || mode == 2) ? bitmap_words(max_q_nnz) : 0;
    const size_t lds = sizeof(int32_t) * ((size_t)2 * pad4(max_tile_nnz) + pad4(max_tile_nq + 1) + (size_t)kSpWaves * bm_words);
    switch (mode) {
        case 0: return launch_sparse_tiles_t<0>(ctx, tiles_dev, ntiles, lds, bm_words, q, r, out, out_stride);
        case 1: return launch_sparse_tiles_t<1>(ctx, tiles_dev, ntiles, lds, bm_words, q, r, out, out_stride);
        case 2: return launch_sparse_tiles_t<2>(ctx, tiles_dev, ntiles, lds, bm_words, q, r, out, out_stride);
        case 3:
            if (ntiles != 1 || max_tile_nq != 1) PGV_FAIL(PGV_ERR_ARG, "sparse cosine: one query");
            return launch_sparse_tiles_t<3>(ctx, tiles_dev, ntiles, lds, bm_words, q, r, out, out_stride);
    }
    PGV_FAIL(PGV_ERR_ARG, "sparse scan: unknown mode %d", mode);
}

int launch_sparse_pack(pgv_ctx *ctx, const int32_t *idx, const float *val, int64_t total, void *elem) {
    if (total <= 0) return PGV_OK;
    const int64_t want = (total + 255) / 256, cap = (int64_t)ctx->num_cus * 32;
    hipLaunchKernelGGL(sparse_pack_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, ctx->stream, idx, val, total,
                       static_cast<QElem *>(elem));
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_sparse_pairs(pgv_ctx *ctx, const RowsView &v, const int64_t *q_ptr, const void *q_elem, const int32_t *slot,
                        const int32_t *query_of, int64_t npairs, float *out) {
    if (npairs <= 0) return PGV_OK;
    if (!v.sparse()) PGV_FAIL(PGV_ERR_ARG, "sparse pairs: not a sparse mirror");
    const int64_t want = (npairs + kSpWaves - 1) / kSpWaves, cap = (int64_t)ctx->num_cus * 32;
    const dim3 grid((unsigned)(want < cap ? want : cap));
    const QElem *re = static_cast<const QElem *>(v.rows), *qe = static_cast<const QElem *>(q_elem);
    switch (v.metric) {
        case PGV_L2SQ:
            hipLaunchKernelGGL(sparse_pair_kernel<0>, grid, dim3(kSpThreads), 0, ctx->stream, v.ptr, re, q_ptr, qe, slot, query_of, npairs, out);
            break;
        case PGV_NEG_IP:
            hipLaunchKernelGGL(sparse_pair_kernel<1>, grid, dim3(kSpThreads), 0, ctx->stream, v.ptr, re, q_ptr, qe, slot, query_of, npairs, out);
            break;
        case PGV_L1:
            hipLaunchKernelGGL(sparse_pair_kernel<2>, grid, dim3(kSpThreads), 0, ctx->stream, v.ptr, re, q_ptr, qe, slot, query_of, npairs, out);
            break;
        default: PGV_FAIL(PGV_ERR_ARG, "unknown metric %d", (int)v.metric);
    }
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_sparse_groups(pgv_ctx *ctx, const RowsView &v, const int32_t *ids, const int64_t *ids_at, int64_t ids_stride,
                         const int32_t *n_arr, const int32_t *from_arr, const int64_t *pair_at, int ngroups, float *out) {
    if (ngroups <= 0) return PGV_OK;
    if (!v.sparse()) PGV_FAIL(PGV_ERR_ARG, "sparse groups: not a sparse mirror");
    // a batch of the build brings thousands of groups, a serial build one or two of up to ef_construction members: the
    // groups fill x, and y spreads a group's members while x alone leaves CUs idle.  An item with nothing to score costs a
    // pass over its group's ids, so y stays small
    const int cap = ctx->num_cus * 16;
    const int gx = ngroups < cap ? ngroups : cap;
    int gy = (cap + gx - 1) / gx;
    if (gy > 32) gy = 32;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    const QElem *re = static_cast<const QElem *>(v.rows);
    switch (v.metric) {
        case PGV_L2SQ:
            hipLaunchKernelGGL(sparse_groups_kernel<0>, grid, dim3(kSpThreads), 0, ctx->stream, v.ptr, re, ids, ids_at, ids_stride,
                               n_arr, from_arr, pair_at, ngroups, out);
            break;
        case PGV_NEG_IP:
            hipLaunchKernelGGL(sparse_groups_kernel<1>, grid, dim3(kSpThreads), 0, ctx->stream, v.ptr, re, ids, ids_at, ids_stride,
                               n_arr, from_arr, pair_at, ngroups, out);
            break;
        case PGV_L1:
            hipLaunchKernelGGL(sparse_groups_kernel<2>, grid, dim3(kSpThreads), 0, ctx->stream, v.ptr, re, ids, ids_at, ids_stride,
                               n_arr, from_arr, pair_at, ngroups, out);
            break;
        default: PGV_FAIL(PGV_ERR_ARG, "unknown metric %d", (int)v.metric);
    }
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_sparse_orient_pairs(pgv_ctx *ctx, int32_t *a, int32_t *b, int64_t npairs) {
    if (npairs <= 0) return PGV_OK;
    const int64_t want = (npairs + 255) / 256, cap = (int64_t)ctx->num_cus * 32;
    hipLaunchKernelGGL(sparse_orient_pairs_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, ctx->stream, a, b, npairs);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

}  // namespace pgv
