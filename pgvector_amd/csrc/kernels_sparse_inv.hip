// kernels_sparse_inv.hip -- sparsevec rows inverted on the device, and the exact inner-product scan over them
// (pgv_sparse_rows_upload / pgv_sparse_rows_topk).
//
// Under the inner product (SparsevecInnerProduct, src/sparsevec.c:905-936) only the indices both vectors store add a term,
// so what a query needs of the rows is the postings of the dimensions it stores.  sparse_tile_kernel (kernels_sparse.hip)
// visits every (query, row) pair and searches every stored row element in the query; this file keeps the rows the other
// way round and touches nothing else.
//
// The mirror.  Rows are cut into blocks of kInvRows consecutive rows.  A block's stored elements lie sorted by (dimension,
// row) as 8-byte postings (row inside the block, value); the postings of one dimension inside one block are a RUN, and a
// directory lists the runs in the same order: dir_dim (ascending inside a block), dir_start, and blk_dir[b] = the first
// run of block b.  A block is searched by dimension in its own directory: no array of `dim` entries exists (dim may be
// 10^9).  Built by
//   inv_keys_kernel    one 64-bit key a stored element, (block | dimension | row in block) from the top: the key order IS
//                      the layout order.  (A CSR position of 32 bits does not fit beside 20 bits of block and 30 of
//                      dimension; the row inside the block, 11 or 12 bits, does, and says everything the position would.)
//   rocPRIM radix sort of (key, value) pairs over the bits in use, the values being the CSR's own val array
//   inv_pack_kernel    posting i = (key_i's row, value_i), and how many runs begin in each chunk of 1024 postings
//   rocPRIM exclusive scan of the chunk counts: where a chunk's runs go in the directory
//   inv_dir_kernel     a block-level scan of the run heads inside the chunk places each run, and the run that begins a
//                      block writes blk_dir
//
// The scan.  A workgroup owns (a tile of kInvQueries consecutive queries) x (one row block) and keeps kInvQueries x
// kInvRows fp32 accumulators in LDS, one row of them per WAVEFRONT: a wavefront owns one query of the tile, so no two
// wavefronts share an accumulator and the kernel has no barrier and no atomic.  The wavefront walks its query's stored
// elements in ascending index order, 64 at a time: every lane finds its own element's run by a branch-free binary search
// of the block's directory (the 64 descents run side by side), then the runs are taken ONE AFTER THE OTHER in element
// order, a lane a posting, acc[row] = fmaf(q, x, acc[row]).  The rows inside a run are distinct, so the lanes never meet;
// the runs of one query are taken in order by one wavefront, so an accumulator sees its terms in ascending index order:
// the value depends on the (query, row) pair alone and two runs give the same bits.  The next run's first 64 postings are
// requested before the current run is added.  Epilogue: 0 - acc, 256 contiguous bytes a store, the tail rows of the last
// block masked; a block without postings writes +0.0.  Workgroups that share a row block are adjacent in the grid.
//
// No matrix instruction: nothing here is a dense contraction.  The selection is launch_topk_segments, unchanged.
#include <algorithm>

#include "pgv_device.h"

#include <rocprim/rocprim.hpp>

// the pair measured best at tools/bench_sparse_inv_topk.py's shape (profiles/r34_sparse_inv_topk.md has the table); a
// build with other values is how the table was taken
#ifndef PGV_INV_ROWS
#define PGV_INV_ROWS 4096
#endif
#ifndef PGV_INV_QUERIES
#define PGV_INV_QUERIES 4
#endif

namespace pgv {

namespace {

constexpr int kInvRows = PGV_INV_ROWS;        // rows of a block (pgvector_amd/_lib.py SPARSE_INV_ROWS says the same)
constexpr int kInvQueries = PGV_INV_QUERIES;  // queries of a tile = wavefronts of a scan workgroup (SPARSE_INV_QUERIES)
constexpr int kInvRowBits = kInvRows == 2048 ? 11 : 12;
constexpr int kInvChunk = 1024;  // postings a workgroup of the build's last two kernels takes: 4 a thread
static_assert(kInvRows == 2048 || kInvRows == 4096, "a block's row index has 11 or 12 bits of the key");
static_assert(kInvQueries >= 1 && kInvQueries <= 16, "a wavefront a query, 1024 threads a workgroup at most");
static_assert((size_t)kInvQueries * kInvRows * sizeof(float) <= 160 * 1024, "the accumulators live in one CU's LDS");
static_assert(sizeof(SparseInvPosting) == 8, "a posting is one 8-byte load");

// a wavefront a row, grid-stride: keys[p] for the row's stored elements p.  An index is masked to the bits the key gives
// it, so that an unchecked device array cannot reach the block's bits
__global__ __launch_bounds__(256) void inv_keys_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                       int64_t n, int idx_bits, unsigned long long *__restrict__ keys) {
    const int lane = threadIdx.x & (kWave - 1);
    const unsigned long long imask = (1ull << idx_bits) - 1ull;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {
        const unsigned long long high = (unsigned long long)(r / kInvRows) << (idx_bits + kInvRowBits) |
                                        (unsigned long long)(r % kInvRows);
        for (int64_t p = ptr[r] + lane; p < ptr[r + 1]; p += kWave)
            keys[p] = high | ((unsigned long long)(uint32_t)idx[p] & imask) << kInvRowBits;
    }
}

// posting i begins a run when it is the first, or when the one before it has another (block, dimension)
__device__ __forceinline__ bool inv_run_head(const unsigned long long *keys, int64_t i) {
    return i == 0 || (keys[i] >> kInvRowBits) != (keys[i - 1] >> kInvRowBits);
}

__global__ __launch_bounds__(256) void inv_pack_kernel(const unsigned long long *__restrict__ keys, const float *__restrict__ vals,
                                                       int64_t total, SparseInvPosting *__restrict__ post,
                                                       uint32_t *__restrict__ chunk_runs) {
    int heads = 0;
    for (int j = 0; j < kInvChunk / 256; j++) {
        const int64_t i = (int64_t)blockIdx.x * kInvChunk + j * 256 + threadIdx.x;
        const bool in = i < total;
        if (in) post[i] = {(uint32_t)(keys[i] & (kInvRows - 1)), vals[i]};
        heads += __syncthreads_count(in && inv_run_head(keys, i));
    }
    if (threadIdx.x == 0) chunk_runs[blockIdx.x] = (uint32_t)heads;
}

// chunk_at: the exclusive scan of chunk_runs.  Run number = chunk_at[chunk] + the heads before it in the chunk
__global__ __launch_bounds__(256) void inv_dir_kernel(const unsigned long long *__restrict__ keys, int64_t total,
                                                      const uint32_t *__restrict__ chunk_at, int idx_bits, uint32_t nblocks,
                                                      uint32_t ndir, int32_t *__restrict__ dir_dim,
                                                      uint32_t *__restrict__ dir_start, uint32_t *__restrict__ blk_dir) {
    __shared__ int s_wave[4];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    uint32_t base = chunk_at[blockIdx.x];
    for (int j = 0; j < kInvChunk / 256; j++) {
        const int64_t i = (int64_t)blockIdx.x * kInvChunk + j * 256 + threadIdx.x;
        const bool head = i < total && inv_run_head(keys, i);
        const unsigned long long bal = __ballot(head);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        uint32_t run = base + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < 4; w++) {
            if (w < wave) run += s_wave[w];
            base += s_wave[w];
        }
        __syncthreads();
        if (i < total) {
            const uint32_t blk = (uint32_t)(keys[i] >> (idx_bits + kInvRowBits));
            if (head) {
                dir_dim[run] = (int32_t)((keys[i] >> kInvRowBits) & ((1ull << idx_bits) - 1ull));
                dir_start[run] = (uint32_t)i;
                // the first run of its block, and of the blocks without a stored element before it
                const uint32_t after = i == 0 ? 0u : (uint32_t)(keys[i - 1] >> (idx_bits + kInvRowBits)) + 1u;
                for (uint32_t b = after; b <= blk && b <= nblocks; b++) blk_dir[b] = run;
            }
            if (i == total - 1) {
                for (uint32_t b = blk + 1; b <= nblocks; b++) blk_dir[b] = ndir;
                dir_dim[ndir] = 0;
                dir_start[ndir] = (uint32_t)total;
            }
        }
    }
}

// grid: (row blocks) x (tiles), the tiles of a block adjacent.  Dynamic LDS: QT x R floats
template <int QT, int R>
__global__ __launch_bounds__(QT *kWave) void sparse_inv_scan_kernel(
    const SparseInvPosting *__restrict__ post, const int32_t *__restrict__ dir_dim, const uint32_t *__restrict__ dir_start,
    const uint32_t *__restrict__ blk_dir, int64_t n, const int64_t *__restrict__ q_ptr, const int32_t *__restrict__ q_idx,
    const float *__restrict__ q_val, int q0, int nq, int ntiles, float *__restrict__ mat) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t blk = blockIdx.x / (unsigned)ntiles;
    const int ql = (int)(blockIdx.x % (unsigned)ntiles) * QT + wave;  // this wavefront's query, counted in the launch
    if (ql >= nq) return;  // (a short last tile; nothing below waits for another wavefront)
    float *acc = reinterpret_cast<float *>(smem) + wave * R;
    for (int r = lane * 4; r < R; r += kWave * 4) *reinterpret_cast<float4 *>(acc + r) = make_float4(0.f, 0.f, 0.f, 0.f);

    const uint32_t d0 = blk_dir[blk], dn = blk_dir[blk + 1] - d0;
    const int64_t qb = q_ptr[q0 + ql], qe = q_ptr[q0 + ql + 1];
    for (int64_t e0 = qb; e0 < qe && dn > 0; e0 += kWave) {
        // lane l: element e0 + l of the query and its run in this block (count 0: the block does not store the dimension)
        const bool has = e0 + lane < qe;
        const int32_t t = q_idx[has ? e0 + lane : e0];
        const float qv = q_val[has ? e0 + lane : e0];
        uint32_t lo = d0;
        for (uint32_t len = dn; len > 1;) {  // the last run whose dimension is not above t, if any: trips by dn alone
            const uint32_t half = len >> 1;
            lo = dir_dim[lo + half] <= t ? lo + half : lo;
            len -= half;
        }
        const uint32_t start = dir_start[lo];
        const uint32_t count = has && dir_dim[lo] == t ? dir_start[lo + 1] - start : 0u;

        // the runs in element order.  A run's first 64 postings are loaded one run ahead (a lane past the run's end reads
        // the run's first posting again: never a predicated load; post has one slack entry for a run of nothing)
        unsigned long long todo = __ballot(count != 0u);
        if (todo == 0ull) continue;
        int l = __ffsll(todo) - 1;
        uint32_t s = __shfl(start, l), c = __shfl(count, l);
        SparseInvPosting nxt = post[s + ((uint32_t)lane < c ? lane : 0)];
        while (todo != 0ull) {
            todo &= todo - 1ull;
            const SparseInvPosting cur = nxt;
            const uint32_t cs = s, cc = c;
            const float v = __shfl(qv, l);
            if (todo != 0ull) {
                l = __ffsll(todo) - 1;
                s = __shfl(start, l);
                c = __shfl(count, l);
                nxt = post[s + ((uint32_t)lane < c ? lane : 0)];
            }
            if ((uint32_t)lane < cc) acc[cur.row] = __builtin_fmaf(v, cur.val, acc[cur.row]);
            for (uint32_t o = kWave + lane; o < cc; o += kWave) {
                const SparseInvPosting p = post[cs + o];
                acc[p.row] = __builtin_fmaf(v, p.val, acc[p.row]);
            }
        }
    }

    // the negative inner product as 0 - ip: an empty intersection is +0.0 (sparse_tile_kernel's rule)
    const int64_t row0 = (int64_t)blk * R;
    const int rows = (int)(n - row0 < R ? n - row0 : R);
    float *out = mat + (size_t)ql * (size_t)n + (size_t)row0;
    for (int r = lane; r < rows; r += kWave) out[r] = 0.f - acc[r];
}

template <typename T> int inv_alloc(T **p, size_t count) {
    PGV_HIP(hipMalloc(reinterpret_cast<void **>(p), sizeof(T) * (count ? count : 1)));
    return PGV_OK;
}

// what the build holds only while it runs
struct InvScratch {
    unsigned long long *keys_in = nullptr, *keys_out = nullptr;
    float *vals_out = nullptr;
    uint32_t *chunk_runs = nullptr, *chunk_at = nullptr;
    void *temp = nullptr;
    ~InvScratch() {
        for (void *p : {(void *)keys_in, (void *)keys_out, (void *)vals_out, (void *)chunk_runs, (void *)chunk_at, temp})
            if (p) (void)hipFree(p);
    }
};

int inv_build(pgv_ctx *ctx, int dim, const SparseCsr &rows, int64_t total, SparseInv *inv) {
    inv->n = rows.n;
    inv->total = total;
    inv->nblocks = (uint32_t)((rows.n + kInvRows - 1) / kInvRows);
    PGV_TRY(inv_alloc(&inv->post, (size_t)total + 1));
    PGV_TRY(inv_alloc(&inv->blk_dir, (size_t)inv->nblocks + 1));
    PGV_HIP(hipMemsetAsync(inv->post + total, 0, sizeof(SparseInvPosting), ctx->stream));
    PGV_HIP(hipMemsetAsync(inv->blk_dir, 0, sizeof(uint32_t) * ((size_t)inv->nblocks + 1), ctx->stream));
    if (total == 0) {  // every block's directory is empty
        PGV_TRY(inv_alloc(&inv->dir_dim, 1));
        PGV_TRY(inv_alloc(&inv->dir_start, 1));
        PGV_HIP(hipMemsetAsync(inv->dir_dim, 0, sizeof(int32_t), ctx->stream));
        PGV_HIP(hipMemsetAsync(inv->dir_start, 0, sizeof(uint32_t), ctx->stream));
        PGV_HIP(hipStreamSynchronize(ctx->stream));
        return PGV_OK;
    }
    int idx_bits = 1, blk_bits = 1;
    while (idx_bits < 30 && (1ll << idx_bits) < dim) idx_bits++;
    while ((1ull << blk_bits) < inv->nblocks) blk_bits++;
    const unsigned key_bits = (unsigned)(kInvRowBits + idx_bits + blk_bits);  // <= 12 + 30 + 20
    const size_t nchunks = ((size_t)total + kInvChunk - 1) / kInvChunk;

    InvScratch s;
    PGV_TRY(inv_alloc(&s.keys_in, (size_t)total));
    PGV_TRY(inv_alloc(&s.keys_out, (size_t)total));
    PGV_TRY(inv_alloc(&s.vals_out, (size_t)total));
    PGV_TRY(inv_alloc(&s.chunk_runs, nchunks + 1));
    PGV_TRY(inv_alloc(&s.chunk_at, nchunks + 1));
    size_t sort_bytes = 0, scan_bytes = 0;
    PGV_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, s.keys_in, s.keys_out, rows.val, s.vals_out, (size_t)total, 0, key_bits,
                                      ctx->stream));
    PGV_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, s.chunk_runs, s.chunk_at, 0u, nchunks + 1, rocprim::plus<uint32_t>(),
                                    ctx->stream));
    PGV_HIP(hipMalloc(&s.temp, std::max<size_t>(std::max(sort_bytes, scan_bytes), 16)));

    const int64_t want = (rows.n + 3) / 4, cap = (int64_t)ctx->num_cus * 64;
    hipLaunchKernelGGL(inv_keys_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, ctx->stream, rows.ptr, rows.idx,
                       rows.n, idx_bits, s.keys_in);
    PGV_HIP(hipGetLastError());
    PGV_HIP(rocprim::radix_sort_pairs(s.temp, sort_bytes, s.keys_in, s.keys_out, rows.val, s.vals_out, (size_t)total, 0, key_bits,
                                      ctx->stream));
    PGV_HIP(hipMemsetAsync(s.chunk_runs + nchunks, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(inv_pack_kernel, dim3((unsigned)nchunks), dim3(256), 0, ctx->stream, s.keys_out, s.vals_out, total, inv->post,
                       s.chunk_runs);
    PGV_HIP(hipGetLastError());
    PGV_HIP(rocprim::exclusive_scan(s.temp, scan_bytes, s.chunk_runs, s.chunk_at, 0u, nchunks + 1, rocprim::plus<uint32_t>(),
                                    ctx->stream));
    // the directory is allocated at its size: the runs are counted first
    PGV_HIP(hipMemcpyAsync(&inv->ndir, s.chunk_at + nchunks, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    PGV_TRY(inv_alloc(&inv->dir_dim, (size_t)inv->ndir + 1));
    PGV_TRY(inv_alloc(&inv->dir_start, (size_t)inv->ndir + 1));
    hipLaunchKernelGGL(inv_dir_kernel, dim3((unsigned)nchunks), dim3(256), 0, ctx->stream, s.keys_out, total, s.chunk_at, idx_bits,
                       inv->nblocks, inv->ndir, inv->dir_dim, inv->dir_start, inv->blk_dir);
    PGV_HIP(hipGetLastError());
    PGV_HIP(hipStreamSynchronize(ctx->stream));
    return PGV_OK;
}

}  // namespace

int sparse_inv_rows() { return kInvRows; }
int sparse_inv_queries() { return kInvQueries; }

void sparse_inv_release(SparseInv *inv) {
    for (void *p : {(void *)inv->post, (void *)inv->dir_dim, (void *)inv->dir_start, (void *)inv->blk_dir})
        if (p) (void)hipFree(p);
    *inv = SparseInv{};
}

int sparse_inv_build(pgv_ctx *ctx, int dim, const SparseCsr &rows, int64_t total, SparseInv *out) {
    const int rc = inv_build(ctx, dim, rows, total, out);
    if (rc != PGV_OK) sparse_inv_release(out);
    return rc;
}

int launch_sparse_inv_scan(pgv_ctx *ctx, const SparseInv &inv, const SparseCsr &q, int q0, int nq, float *mat) {
    if (inv.n <= 0 || nq <= 0) return PGV_OK;
    const int ntiles = (nq + kInvQueries - 1) / kInvQueries;
    const int64_t grid = (int64_t)inv.nblocks * ntiles;
    if (grid > 0x7fffffff) PGV_FAIL(PGV_ERR_ARG, "sparse rows scan: too many workgroups");
    auto kern = sparse_inv_scan_kernel<kInvQueries, kInvRows>;
    constexpr size_t lds = (size_t)kInvQueries * kInvRows * sizeof(float);
    if (lds > 64 * 1024)
        PGV_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kInvQueries * kWave), lds, ctx->stream, inv.post, inv.dir_dim, inv.dir_start,
                       inv.blk_dir, inv.n, q.ptr, q.idx, q.val, q0, nq, ntiles, mat);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

}  // namespace pgv
