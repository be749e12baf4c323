// sparse_pair.h -- the arithmetic of ONE (row, query) pair of sparse vectors, shared by sparse_tile_kernel
// (kernels_sparse.hip: every row against tiles of queries) and by the HNSW walk and pair scorer over a sparse mirror
// (kernels_hnsw.hip, kernels_sparse.hip): the same terms in the same order of additions wherever a pair is scored
// (DESIGN.md 4.4d, 4.6c), so that the walk's keys are pgv_sparse_distance_batch's values bit for bit.
// Lane l of a wavefront adds the row's elements l, l + 64, .., then the query's unmatched elements l, l + 64, ..; the caller
// finishes with group_sum_to_last(a0, 6).  Where the query's elements live (LDS or the caches) is the caller's choice.
#pragma once

#include "pgv_device.h"

namespace pgv {

// a sparsevec element row of an HNSW mirror (pgv_hnsw::sparse): a tag like BitRow, never a value
struct SparseRow {};
template <> struct VecTraits<SparseRow> {
    static constexpr int N = 1;
};

constexpr int kSparseRegChunks = 4;      // a row of up to 4 x 64 stored elements stays in registers
constexpr int kSparseMaxNnz = 16000;     // SPARSEVEC_MAX_NNZ (src/sparsevec.h)
constexpr int kSparseHnswMaxNnz = 1000;  // HNSW_MAX_NNZ (src/hnsw.h:34): an ELEMENT of a sparse HNSW mirror at most

__host__ __device__ constexpr int pad4(int x) { return (x + 3) & ~3; }
__host__ __device__ constexpr int bitmap_words(int nnz) { return pad4((nnz + 31) / 32); }

// LDS ordering inside ONE wavefront (bitmap clear -> set -> sweep): the wavefront's LDS operations complete in order,
// the fence keeps the compiler from moving them across and waits for the ones in flight
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// A stored element: index and value side by side, so that one 8-byte read of the search brings both (a query in LDS,
// and the element rows of a sparse HNSW mirror in HBM)
struct alignas(8) QElem {
    int32_t i;
    float v;
};
typedef int QPair __attribute__((ext_vector_type(2)));

// Where index x stands among the n ascending indices at q: a descent by powers of two, `top` the largest one <= n (0 for
// n = 0), so every lane makes the same trips.  pos counts the elements <= x and `last` is the last of them (index -1: none);
// the query stores x iff last.i == x, at pos - 1, with last.v its value: nothing is read after the descent
struct Found {
    int pos;
    QElem last;
    __device__ __forceinline__ bool hit(int32_t x) const { return last.i == x; }
};
__device__ __forceinline__ void descend(Found &f, const QElem *q, int n, int s, int32_t x) {
    const int t = f.pos + s;
    // one 8-byte LDS read, made whether or not the step counts: never predicated
    const QPair raw = *reinterpret_cast<const QPair *>(q + ((t <= n ? t : n) - 1));
    const QElem e{raw.x, __int_as_float(raw.y)};
    if (t <= n && e.i <= x) {
        f.pos = t;
        f.last = e;
    }
}

// One stored row element against the query: its term into a0 (a1: the row's squared norm, cosine).  MODE 0: L2 squared,
// 1: inner product, 2: L1, 3: cosine.  hit: the query stores the index too, at pos
template <int MODE>
__device__ __forceinline__ void add_term(const Found &f, int32_t ri, float rv, uint32_t *bm, float &a0, float &a1) {
    const bool hit = f.hit(ri);
    // an index the query does not store: (rv - 0)^2 = rv^2 and |rv - 0| = |rv|, the reference's own terms
    const float b = hit ? f.last.v : 0.f;
    if ((MODE == 0 || MODE == 2) && hit) atomicOr(&bm[(f.pos - 1) >> 5], 1u << ((f.pos - 1) & 31));
    if (MODE == 0) {
        const float d = rv - b;
        a0 = __builtin_fmaf(d, d, a0);
    } else if (MODE == 2) {
        a0 += fabsf(rv - b);
    } else {
        if (hit) a0 = __builtin_fmaf(rv, b, a0);
        if (MODE == 3) a1 = __builtin_fmaf(rv, rv, a1);
    }
}

// A row of up to kSparseRegChunks x 64 stored elements, read once and kept across the tile's queries: lane l holds
// elements l, l + 64, ..  Its NC = ceil(rn / 64) searches descend TOGETHER, so that NC LDS reads are in flight per step
// instead of one (1.2 x at the learned-sparse shape against one search after the other, profiles/r21_sparse_topk.md)
struct RegRow {
    int32_t i[kSparseRegChunks];
    float v[kSparseRegChunks];
};
template <int MODE, int NC>
__device__ __forceinline__ void row_side_reg(const RegRow &row, int rn, const QElem *q, int qn, int top, uint32_t *bm,
                                             int lane, float &a0, float &a1) {
    Found f[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) f[c] = {0, {-1, 0.f}};
    for (int s = top; s > 0; s >>= 1) {  // (top > 0 only when qn > 0)
#pragma unroll
        for (int c = 0; c < NC; c++) descend(f[c], q, qn, s, row.i[c]);
    }
#pragma unroll
    for (int c = 0; c < NC; c++)
        if (c * kWave + lane < rn) add_term<MODE>(f[c], row.i[c], row.v[c], bm, a0, a1);
}
// A longer row: read again per query (from the caches), one search after the other
template <int MODE>
__device__ __forceinline__ void row_side_mem(const int32_t *ri, const float *rv, int rn, const QElem *q, int qn, int top,
                                             uint32_t *bm, int lane, float &a0, float &a1) {
    for (int e = lane; e < rn; e += kWave) {
        const int32_t x = ri[e];
        Found f{0, {-1, 0.f}};
        for (int s = top; s > 0; s >>= 1) descend(f, q, qn, s, x);
        add_term<MODE>(f, x, rv[e], bm, a0, a1);
    }
}
// ... whose index and value sit side by side (an element row of a sparse HNSW mirror): the same elements in the same order
template <int MODE>
__device__ __forceinline__ void row_side_mem(const QElem *re, int rn, const QElem *q, int qn, int top, uint32_t *bm, int lane,
                                             float &a0, float &a1) {
    for (int e = lane; e < rn; e += kWave) {
        const QPair raw = *reinterpret_cast<const QPair *>(re + e);
        Found f{0, {-1, 0.f}};
        for (int s = top; s > 0; s >>= 1) descend(f, q, qn, s, raw.x);
        add_term<MODE>(f, raw.x, __int_as_float(raw.y), bm, a0, a1);
    }
}

// One (row, query) pair, this lane's share: row_side(top) adds the row's elements, then the query's unmatched ones (L2,
// L1) come from the wavefront's bitmap.  q: the query's qn elements in LDS
template <int MODE, typename RowSide>
__device__ __forceinline__ void score_pair(RowSide row_side, const QElem *q, int qn, uint32_t *bm, int lane, float &a0) {
    constexpr bool kBitmap = MODE == 0 || MODE == 2;
    if (kBitmap) {
        for (int w = lane; w < (qn + 31) / 32; w += kWave) bm[w] = 0u;
        wave_lds_fence();
    }
    row_side(qn > 0 ? 1 << (31 - __clz(qn)) : 0);
    if (kBitmap) {
        wave_lds_fence();
        for (int j = lane; j < qn; j += kWave) {
            if (!((bm[j >> 5] >> (j & 31)) & 1u)) {
                const float a = q[j].v;
                if (MODE == 0)
                    a0 = __builtin_fmaf(a, a, a0);
                else
                    a0 += fabsf(a);
            }
        }
        wave_lds_fence();  // the sweep has read the bitmap before the next pair clears it
    }
}

// An element row of a sparse HNSW mirror (rn <= 1000 stored elements at re, index and value side by side) against a query
// whose qn elements are at q: the row in registers up to kSparseRegChunks x 64 elements (`row`, filled by
// load_reg_row), through row_side_mem past that.  The pair's value lands in the LAST lane
__device__ __forceinline__ void load_reg_row(RegRow &row, const QElem *re, int rn, int lane) {
#pragma unroll
    for (int c = 0; c < kSparseRegChunks; c++) {
        const int e = c * kWave + lane;
        // never predicate a load: a lane past the row reads the row's last element (or the slack element behind an empty
        // row, which the mirror keeps) and its term is masked in row_side_reg
        const int ec = e < rn ? e : (rn > 0 ? rn - 1 : 0);
        const QPair raw = *reinterpret_cast<const QPair *>(re + ec);
        row.i[c] = raw.x;
        row.v[c] = __int_as_float(raw.y);
    }
}
template <int MODE>
__device__ __forceinline__ float score_element(const RegRow &row, const QElem *re, int rn, const QElem *q, int qn,
                                               uint32_t *bm, int lane) {
    float a0 = 0.f, a1 = 0.f;
    if (rn <= kSparseRegChunks * kWave) {
        switch ((rn + kWave - 1) / kWave) {
            case 0:
            case 1:
                score_pair<MODE>([&](int top) { row_side_reg<MODE, 1>(row, rn, q, qn, top, bm, lane, a0, a1); }, q, qn, bm, lane, a0);
                break;
            case 2:
                score_pair<MODE>([&](int top) { row_side_reg<MODE, 2>(row, rn, q, qn, top, bm, lane, a0, a1); }, q, qn, bm, lane, a0);
                break;
            case 3:
                score_pair<MODE>([&](int top) { row_side_reg<MODE, 3>(row, rn, q, qn, top, bm, lane, a0, a1); }, q, qn, bm, lane, a0);
                break;
            default:
                score_pair<MODE>([&](int top) { row_side_reg<MODE, 4>(row, rn, q, qn, top, bm, lane, a0, a1); }, q, qn, bm, lane, a0);
                break;
        }
    } else {
        score_pair<MODE>([&](int top) { row_side_mem<MODE>(re, rn, q, qn, top, bm, lane, a0, a1); }, q, qn, bm, lane, a0);
    }
    a0 = group_sum_to_last(a0, 6);
    // the negative inner product as 0 - ip: an empty intersection is +0.0 (as in sparse_tile_kernel)
    return MODE == 1 ? 0.f - a0 : a0;
}

}  // namespace pgv
