// kernels_bit.hip -- binary quantization on the device: the two-stage query of the reference's README,
//     SELECT * FROM (SELECT * FROM items ORDER BY binary_quantize(embedding)::bit(d) <~> binary_quantize($1) LIMIT k')
//     ORDER BY embedding <=> $1 LIMIT k
// for a batch of queries.
//   hamming_tile_kernel      hamming_distance (src/bitvec.c:45-56 over BitHammingDistanceDefault, src/bitutils.c:49-73)
//                            of a tile of rows against a tile of queries, into pgv_bit_topk's distance matrix
//   binary_quantize_kernel   binary_quantize (src/vector.c:952-979, halfvec_binary_quantize in src/halfvec.c)
//   rerank_*_kernel          what pgv_rerank needs around score_gather_kernel and topk_kernel
//   hamming_list_kernel      the list scan of `USING ivfflat (col bit_hamming_ops)`: GetScanItems (src/ivfscan.c:123-187)
//                            over the batch plan's ScanTask / ScanPair (pgv_index::nbits)
//   bit_closest_kernel, bit_sums_kernel, bit_centers_kernel   the bit k-means around the Hamming matrix (pgv_bit_kmeans)
// bit_kernel (kernels_misc.hip) stays the operator path: one query, float8 out, both bit metrics.
//
// hamming_tile<QT>: the one Hamming tile -- up to 256 rows x QT queries per workgroup, one lane per row.  Both kernels
// below are this function and what differs around it: where a tile's first row is, how many rows it has, and where
// query q's words are (the caller's qrow(q)).
//   * the rows leave HBM once per QT queries: 8 adjacent lanes fetch 128 contiguous bytes of one row with 16-byte loads,
//     the slice goes through LDS (row stride 9 vectors: lane i's ds_read_b128 at 36 i words hits 16 distinct 4-bank
//     slots in each of the instruction's 16-lane groups) and comes back as 32 words of the lane's own row in registers
//   * the query words are the same for every lane: qrow(q) is wave-uniform, they are read through the scalar cache into
//     SGPRs, so the inner step per word is v_xor_b32 with a scalar operand and v_bcnt_u32_b32 accumulating into an
//     integer register.  Both halves of that are written down, not left to the compiler: the words come as scalar
//     loads of 8, each issued before the 8 words ahead of it are counted (a scalar load's latency is otherwise paid
//     every few words: the wait is lgkmcnt(0)), and the accumulating popcount is popc_add
//   * rows longer than the register slice (kBitSliceBits) are walked slice by slice, the next slice's global loads in
//     flight while the current one is counted; the QT counts per lane are converted to float once, at the caller's store
//   * tail rows clamp their address inside the tile, tail queries inside qrow: both are computed, not stored, and no
//     load is predicated
// Rows are padded with zero bytes to whole 16-byte vectors and queries to whole slices (pgv_bit_topk stages them):
// padding adds nothing to a count.
//
// hamming_tile_kernel: one tile of 256 rows x 32 queries of the dense matrix per workgroup; stores are coalesced along
// `row`: lane i writes out[q * n + row0 + i].
//
// hamming_list_kernel<QT>: a task of the list-major plan (launch_plan_batch) per trip of a persistent workgroup -- a
// run of at most 256 rows of one list x the up to QT queries of one group that probes it -- is one tile, into
// out[pair.out_rel + row].
//   * around the tile it is scan_kernel: workgroups pull tasks from the device counter, the last one to finish leaves
//     both counter words zero, ntasks is read from the device
//   * QT in {8, 16, 32}: a list is probed by nq x probes / nlists queries on average (about 10 at 1024 queries x 10
//     probes over 1000 lists), a 1536-bit row costs 192 B of HBM once and 96 vector-ALU operations per (row, query)
//     pair, so at ~10 pairs a row the two are of the same order and padding every group to 32 would triple the ALU work.
//     hamming_list_group_size picks the smallest QT the average share stays below; lists probed by more queries are
//     split into several groups by the plan.  The switch points (8 | 16 | 32 at shares 8 and 16) are arithmetic,
//     UNMEASURED against each other
//   * where the query words come from: the task index reaches the lanes through LDS, so the compiler cannot see that
//     the task's fields and its query ids are the same in every lane.  They are made provably uniform with
//     __builtin_amdgcn_readfirstlane (the task index, the task's fields, every query id -- read once per task, ahead
//     of the tile -- and out_rel): the query words are then addressed from SGPRs, arrive through the scalar cache and
//     the inner step keeps the `v_xor_b32 v, s, v` + `v_bcnt_u32_b32` form.  The alternative -- staging the group's query slices in LDS as
//     scan_kernel does (QT x 128 B per slice, a ds_read per word) -- was not built: UNMEASURED against this one
#include "pgv_device.h"

namespace pgv {

namespace {

constexpr int kBitThreads = 256;                            // rows per tile
constexpr int kBitQueries = 32;                             // queries per tile of the dense matrix
constexpr int kBitSliceVecs = 8;                            // 16-byte vectors of a row in registers at a time
constexpr int kBitSliceWords = kBitSliceVecs * 4;           // 32
constexpr int kBitSliceBits = kBitSliceWords * 32;          // 1024: the register slice
constexpr int kBitLdsStride = kBitSliceVecs + 1;            // vectors; the pad keeps the transposed read conflict-free
constexpr int kBitRowsPerTrip = kBitThreads / kBitSliceVecs;  // 32 rows per cooperative load instruction
constexpr int kBitTileVecs = kBitThreads * kBitLdsStride;   // the tile's LDS
static_assert(kBitSliceBits == 1024, "tests/test_gpu_bit_topk.py sweeps nbits around the register slice");

typedef uint32_t QWords8 __attribute__((ext_vector_type(8), aligned(4)));  // one s_load_dwordx8 of query words

// popcount(x) + acc, the one instruction it is, written out.  The compiler has the pattern, but selects it only while
// the count is the add's FIRST operand.  Inside a kernel's own loops it was; now that the nest lives in a function, it
// is unrolled there before it is inlined, the caller's reassociation pass sees the whole chain of adds and hands it
// back with the count second, and every two counts cost a v_add3_u32 on top: + 25 % vector-ALU operations, 15 % on
// the dense scan and 11 % on the 32-query list scan when it was measured (profiles/r19_bit_fold.md)
__device__ __forceinline__ int popc_add(uint32_t x, int acc) {
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(x));
    return acc;
}

// acc[q] += hamming(row tid of the tile, query q) for q < QT.  task_rows: the tile's first row; nrows in 1..256 of them
// are real; qrow(q): the wave-uniform pointer to query q's words.  Every lane of the workgroup calls it; `tile` is free
// for the next call once every lane has passed a barrier
template <int QT, typename QRow>
__device__ __forceinline__ void hamming_tile(Raw16 *tile, const char *task_rows, int nrows, int nvec, QRow qrow,
                                             int (&acc)[QT]) {
    const int tid = threadIdx.x;
    const int nslices = (nvec + kBitSliceVecs - 1) / kBitSliceVecs;
    const size_t row_bytes = (size_t)nvec * sizeof(Raw16);
    const int lv = tid & (kBitSliceVecs - 1);  // which vector of the slice this lane fetches
    const int lr = tid >> 3;                   // ... of rows lr, lr + 32, ..
    Raw16 nxt[kBitSliceVecs];
    auto fetch = [&](int s) {
        const int vi = s * kBitSliceVecs + lv;
        const bool ok = vi < nvec;
        const int vc = ok ? vi : nvec - 1;  // never predicate a load (see scan_kernel)
#pragma unroll
        for (int i = 0; i < kBitSliceVecs; i++) {
            int r = lr + i * kBitRowsPerTrip;
            r = r < nrows ? r : nrows - 1;  // tail rows are computed, not stored
            const Raw16 v = load16(task_rows + (size_t)r * row_bytes + (size_t)vc * sizeof(Raw16));
            nxt[i] = ok ? v : raw16_zero();
        }
    };

    fetch(0);
    for (int s = 0; s < nslices; s++) {
        __syncthreads();  // the previous slice (or tile) has been read by every lane
#pragma unroll
        for (int i = 0; i < kBitSliceVecs; i++) tile[(lr + i * kBitRowsPerTrip) * kBitLdsStride + lv] = nxt[i];
        __syncthreads();
        Raw16 rv[kBitSliceVecs];
#pragma unroll
        for (int v = 0; v < kBitSliceVecs; v++) rv[v] = tile[tid * kBitLdsStride + v];
        if (s + 1 < nslices) fetch(s + 1);

        // four scalar loads of 8 words per query, each in flight while the 8 words before it are counted; the last
        // one of a query is followed by the first one of the next
        auto part = [&](const uint32_t *p) { return *reinterpret_cast<const QWords8 *>(p); };
        const uint32_t *qp = qrow(0) + (size_t)s * kBitSliceWords;
        QWords8 cur = part(qp);
#pragma unroll
        for (int q = 0; q < QT; q++) {
#pragma unroll
            for (int p = 0; p < 4; p++) {
                QWords8 ahead = cur;
                if (p < 3) {
                    ahead = part(qp + 8 * (p + 1));
                } else if (q + 1 < QT) {
                    qp = qrow(q + 1) + (size_t)s * kBitSliceWords;
                    ahead = part(qp);
                }
#pragma unroll
                for (int i = 0; i < 8; i++) acc[q] = popc_add(rv[2 * p + i / 4].w[i % 4] ^ cur[i], acc[q]);
                cur = ahead;
            }
        }
    }
}

__global__ __launch_bounds__(kBitThreads) void hamming_tile_kernel(const char *__restrict__ rows,
                                                                   const uint32_t *__restrict__ queries, int64_t n, int nq,
                                                                   int nvec, int qwords, int nqt, float *__restrict__ out) {
    __shared__ Raw16 tile[kBitTileVecs];
    // consecutive workgroups share a row tile: its query tiles run side by side and find the rows in the caches
    const int qt = (int)(blockIdx.x % (unsigned)nqt);
    const int64_t row0 = (int64_t)(blockIdx.x / (unsigned)nqt) * kBitThreads;
    const int q0 = qt * kBitQueries;
    const int nrows = n - row0 < kBitThreads ? (int)(n - row0) : kBitThreads;

    int acc[kBitQueries] = {};
    hamming_tile<kBitQueries>(
        tile, rows + (size_t)row0 * ((size_t)nvec * sizeof(Raw16)), nrows, nvec,
        [&](int q) { return queries + (size_t)(q0 + q < nq ? q0 + q : nq - 1) * qwords; },  // tail queries: not stored
        acc);

    const int tid = threadIdx.x;
    if (tid < nrows) {
#pragma unroll
        for (int q = 0; q < kBitQueries; q++)
            if (q0 + q < nq) out[(size_t)(q0 + q) * (size_t)n + (size_t)(row0 + tid)] = (float)acc[q];
    }
}

// bit i = x[i] > 0, decided from the element's bit pattern so that the denormal mode cannot matter: sign clear,
// magnitude non-zero, not NaN -- 0 < u <= the pattern of +inf
__device__ __forceinline__ bool positive_bits(uint32_t u) { return u - 1u < 0x7f800000u; }
__device__ __forceinline__ bool positive_bits(uint16_t u) { return (uint16_t)(u - 1u) < (uint16_t)0x7c00u; }

// one lane per OUTPUT BYTE: eight elements in, first element in the most significant bit (VARBITS), the unused low
// bits of a row's last byte zero; no two lanes write the same byte
template <typename U>
__global__ __launch_bounds__(256) void binary_quantize_kernel(const U *__restrict__ x, int64_t n, int dim, int obytes,
                                                              uint8_t *__restrict__ out) {
    const size_t total = (size_t)n * (size_t)obytes;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / (size_t)obytes;
        const int b = (int)(i - r * (size_t)obytes);
        const U *p = x + r * (size_t)dim;
        unsigned byte = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int d = b * 8 + e;
            const bool ok = d < dim;
            const U u = p[ok ? d : dim - 1];
            byte |= (ok && positive_bits(u) ? 1u : 0u) << (7 - e);
        }
        out[i] = (uint8_t)byte;
    }
}

// pgv_rerank: candidate lists [nq x kc] -> the pairs score_gather_kernel reads.  One workgroup per query packs the
// query's real candidates to the front of its row of `packed`, in their order (a stable compaction: thread t owns
// the t-th run of ceil(kc / 256) entries, an exclusive scan over the runs' counts places them); the tail of the row is
// -1.  A "none" scores row 0 of the pair's query; rerank_mask_kernel overwrites the value.
constexpr int kRerankThreads = 256;
__global__ __launch_bounds__(kRerankThreads) void rerank_pairs_kernel(const int64_t *__restrict__ cand, int kc,
                                                                      int64_t *__restrict__ packed, int32_t *__restrict__ slot,
                                                                      int32_t *__restrict__ query_of) {
    __shared__ int scan[kRerankThreads];
    const int q = blockIdx.x, t = threadIdx.x;
    const int64_t base = (int64_t)q * kc;
    const int per = (kc + kRerankThreads - 1) / kRerankThreads;
    const int lo = t * per < kc ? t * per : kc, hi = lo + per < kc ? lo + per : kc;
    int mine = 0;
    for (int i = lo; i < hi; i++) mine += cand[base + i] >= 0;
    scan[t] = mine;
    __syncthreads();
    for (int d = 1; d < kRerankThreads; d <<= 1) {
        const int add = t >= d ? scan[t - d] : 0;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    const int real = scan[kRerankThreads - 1];
    int at = scan[t] - mine;
    for (int i = lo; i < hi; i++) {
        const int64_t c = cand[base + i];
        if (c >= 0) {
            packed[base + at] = c;
            slot[base + at] = (int32_t)c;
            at++;
        }
    }
    for (int i = real + t; i < kc; i += kRerankThreads) {
        packed[base + i] = -1;
        slot[base + i] = 0;
    }
    for (int i = t; i < kc; i += kRerankThreads) query_of[base + i] = q;
}

// the tail of a packed row takes part in the selection as NaN: float8 order puts NaN last and ties go to the lower
// position, so every real candidate -- a +inf or NaN one included -- is selected before any of the tail
__global__ void rerank_mask_kernel(const int64_t *__restrict__ packed, int64_t total, float *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total && packed[i] < 0) vals[i] = __uint_as_float(0x7fc00000u);
}

// position inside a query's packed candidate row -> the row index it holds there; a selected tail entry becomes the
// padding pgv_rerank promises (+inf / -1)
__global__ void rerank_map_kernel(const int64_t *__restrict__ packed, int nq, int kc, int k, const int64_t *__restrict__ pos,
                                  int64_t *__restrict__ out_idx, float *__restrict__ out_dist) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nq * k) return;
    const int64_t p = pos[i];
    const int64_t c = p < 0 ? -1 : packed[(i / k) * kc + p];
    out_idx[i] = c;
    if (c < 0) out_dist[i] = INFINITY;
}


// a value every lane of the workgroup holds alike, told to the compiler
__device__ __forceinline__ int uniform32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const unsigned lo = (unsigned)uniform32((int)(uint32_t)v), hi = (unsigned)uniform32((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <int QT>
__global__ __launch_bounds__(kBitThreads) void hamming_list_kernel(
    const char *__restrict__ rows, const uint32_t *__restrict__ queries, const ScanTask *__restrict__ tasks,
    const int *__restrict__ ntasks_ptr, int *__restrict__ task_counter, const ScanPair *__restrict__ pairs,
    float *__restrict__ out, int nvec, int qwords) {
    __shared__ Raw16 tile[kBitTileVecs];
    __shared__ int lds_task;
    const int tid = threadIdx.x;
    const int ntasks = *ntasks_ptr;

    for (;;) {
        if (tid == 0) lds_task = atomicAdd(task_counter, 1);
        __syncthreads();
        const int t = uniform32(lds_task);
        if (t >= ntasks) {
            // every workgroup ends here exactly once; the last one leaves both words zero for the next launch
            if (tid == 0 && atomicAdd(task_counter + 1, 1) == (int)gridDim.x - 1) {
                atomicExch(task_counter + 1, 0);
                atomicExch(task_counter, 0);
            }
            return;
        }
        const int64_t row0 = uniform64(tasks[t].row0);
        const int nrows = uniform32(tasks[t].nrows);
        const int pair0 = uniform32(tasks[t].pair0);
        const int npairs = uniform32(tasks[t].npairs);

        int qid[QT];  // the group's queries; tail pairs are computed, not stored
#pragma unroll
        for (int q = 0; q < QT; q++) qid[q] = uniform32(pairs[pair0 + (q < npairs ? q : npairs - 1)].query);

        int acc[QT] = {};
        hamming_tile<QT>(tile, rows + (size_t)row0 * ((size_t)nvec * sizeof(Raw16)), nrows, nvec,
                         [&](int q) { return queries + (size_t)qid[q] * qwords; }, acc);

        if (tid < nrows) {
#pragma unroll
            for (int q = 0; q < QT; q++)
                if (q < npairs) out[uniform64(pairs[pair0 + q].out_rel) + row0 + tid] = (float)acc[q];
        }
        // (lds_task and the tile are rewritten behind the barriers at the top of the next trip: every lane has passed at
        // least the two barriers of a slice since it read them)
    }
}

// ---- the bit k-means around the Hamming matrix ----------------------------------------------------------------------
// One lane per sample: Elkan's outcome under an exact metric (src/ivfkmeans.c:323-344 for a sample without a center,
// :401-450 for one that has one) from the sample's row of the distance matrix and that row's first minimum
__global__ void bit_closest_kernel(const float *__restrict__ mat, int k, const float *__restrict__ best_val,
                                   const int64_t *__restrict__ best_pos, int n, int sticky, int32_t *__restrict__ closest_io,
                                   float *__restrict__ out_dist, int32_t *__restrict__ counts,
                                   unsigned long long *__restrict__ changes) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int cur = sticky ? closest_io[j] : -1;
    int now = (int)best_pos[j];
    float d = best_val[j];
    if (cur >= 0) {
        const float dc = mat[(size_t)j * (size_t)k + (size_t)cur];
        if (!(d < dc)) {  // nothing strictly closer: the sample stays (:440)
            now = cur;
            d = dc;
        }
    }
    closest_io[j] = now;
    if (out_dist) out_dist[j] = d;
    if (counts) atomicAdd(&counts[now], 1);
    if (changes && now != cur) atomicAdd(changes, 1ull);
}

// BitSumCenter (src/ivfutils.c:363-370) as integers: one lane per sample byte, an atomic per set bit.  The values are
// counts below 2^24: the order of addition does not matter and the reference's float sums hold the same numbers
__global__ void bit_sums_kernel(const uint8_t *__restrict__ samples, int ld, int bytes, int nbits, int n,
                                const int32_t *__restrict__ closest, int32_t *__restrict__ sums) {
    const size_t total = (size_t)n * (size_t)bytes;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t j = i / (size_t)bytes;
        const int b = (int)(i - j * (size_t)bytes);
        const unsigned byte = samples[j * (size_t)ld + b];
        if (!byte) continue;
        int32_t *dst = sums + (size_t)closest[j] * (size_t)nbits + (size_t)b * 8;
#pragma unroll
        for (int e = 0; e < 8; e++)
            if (((byte >> (7 - e)) & 1u) && b * 8 + e < nbits) atomicAdd(dst + e, 1);
    }
}

// ComputeNewCenters' division and BitUpdateCenter (src/ivfkmeans.c:205-231, src/ivfutils.c:325-339): one lane per
// OUTPUT BYTE of the padded center row; x = (float) sum / (float) count, bit = x > 0.5, first bit in the top bit, pad
// bits and pad bytes zero.  An empty cluster's bits were drawn on the host (refill)
__global__ void bit_centers_kernel(const int32_t *__restrict__ sums, const int32_t *__restrict__ counts, int k, int nbits,
                                   int bytes, int ld, const int32_t *__restrict__ refill_row,
                                   const uint8_t *__restrict__ refill, uint8_t *__restrict__ centers) {
    const size_t total = (size_t)k * (size_t)ld;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i / (size_t)ld);
        const int b = (int)(i - (size_t)c * (size_t)ld);
        unsigned byte = 0;
        if (b < bytes) {
            const int rr = refill_row ? refill_row[c] : -1;
            if (rr >= 0) {
                byte = refill[(size_t)rr * (size_t)bytes + b];
            } else {
                const float cnt = (float)counts[c];
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int d = b * 8 + e;
                    const bool ok = d < nbits;
                    const float x = (float)sums[(size_t)c * (size_t)nbits + (ok ? d : nbits - 1)] / cnt;
                    byte |= (ok && x > 0.5f ? 1u : 0u) << (7 - e);
                }
            }
        }
        centers[i] = (uint8_t)byte;
    }
}

}  // namespace

int bit_topk_slice_bytes() { return kBitSliceVecs * (int)sizeof(Raw16); }

int launch_hamming_tiles(pgv_ctx *ctx, const RowsView &v, const void *queries, int qbytes, int nq, float *out) {
    const int64_t n = v.n;
    if (n <= 0 || nq <= 0) return PGV_OK;
    if (!v.bits() || qbytes < bit_query_bytes(v.geom.ld * 8))
        PGV_FAIL(PGV_ERR_ARG, "bit scan: bit rows, queries in whole slices");
    const int nqt = (nq + kBitQueries - 1) / kBitQueries;
    const int64_t grid = (n + kBitThreads - 1) / kBitThreads * nqt;
    if (grid > 0x7fffffff) PGV_FAIL(PGV_ERR_ARG, "bit scan: too many tiles");
    hipLaunchKernelGGL(hamming_tile_kernel, dim3((unsigned)grid), dim3(kBitThreads), 0, ctx->stream,
                       static_cast<const char *>(v.rows), static_cast<const uint32_t *>(queries), n, nq, v.geom.nvec, qbytes / 4,
                       nqt, out);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

// queries of one group: the smallest instantiation the average share stays BELOW (see the header) -- the share is a mean,
// and with a mean of exactly QT about half the lists would need a second group
int hamming_list_group_size(double queries_per_list) { return queries_per_list < 8.0 ? 8 : (queries_per_list < 16.0 ? 16 : 32); }
int hamming_list_rows_per_task() { return kBitThreads; }

template <int QT>
static int launch_hamming_lists_t(pgv_ctx *ctx, const RowsView &v, const void *queries, int qbytes, const ScanWork &w,
                                  float *out) {
    PGV_TRY(ctx->counters.ensure(256));
    if (!ctx->counters_clean) {
        PGV_HIP(hipMemsetAsync(ctx->counters.p, 0, 256, ctx->stream));
        ctx->counters_clean = true;
    }
    int *counter = ctx->counters.as<int>() + 10;  // words 10, 11 as launch_scan: claimed tasks, workgroups done
    // 36 KB of LDS a workgroup: four of them share a CU
    int grid = ctx->num_cus * 4;
    if (grid > w.ntasks_bound) grid = w.ntasks_bound;
    hipLaunchKernelGGL(hamming_list_kernel<QT>, dim3(grid), dim3(kBitThreads), 0, ctx->stream,
                       static_cast<const char *>(v.rows), static_cast<const uint32_t *>(queries), w.tasks, w.ntasks_dev, counter,
                       w.pairs, out, v.geom.nvec, qbytes / 4);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_hamming_lists(pgv_ctx *ctx, const RowsView &v, const void *queries, int qbytes, const ScanWork &w, int qt,
                         float *out) {
    if (w.ntasks_bound <= 0) return PGV_OK;
    if (!v.bits() || qbytes < bit_query_bytes(v.geom.ld * 8))
        PGV_FAIL(PGV_ERR_ARG, "bit list scan: bit rows, queries in whole slices");
    switch (qt) {
        case 8: return launch_hamming_lists_t<8>(ctx, v, queries, qbytes, w, out);
        case 16: return launch_hamming_lists_t<16>(ctx, v, queries, qbytes, w, out);
        case 32: return launch_hamming_lists_t<32>(ctx, v, queries, qbytes, w, out);
    }
    PGV_FAIL(PGV_ERR_ARG, "bit list scan: unsupported query group size %d", qt);
}

int launch_bit_closest(pgv_ctx *ctx, const float *mat, int k, const float *best_val, const int64_t *best_pos, int n,
                       bool sticky, int32_t *closest_io, float *out_dist, int32_t *counts, unsigned long long *changes) {
    if (n <= 0) return PGV_OK;
    hipLaunchKernelGGL(bit_closest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, mat, k, best_val,
                       best_pos, n, sticky ? 1 : 0, closest_io, out_dist, counts, changes);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_bit_sums(pgv_ctx *ctx, const void *samples, int ld, int nbits, int n, const int32_t *closest, int32_t *sums) {
    if (n <= 0) return PGV_OK;
    const int bytes = (nbits + 7) / 8;
    const size_t total = (size_t)n * (size_t)bytes;
    const size_t want = (total + 255) / 256, cap = (size_t)ctx->num_cus * 64;
    hipLaunchKernelGGL(bit_sums_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, ctx->stream,
                       static_cast<const uint8_t *>(samples), ld, bytes, nbits, n, closest, sums);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_bit_centers(pgv_ctx *ctx, const int32_t *sums, const int32_t *counts, int k, int nbits, int ld,
                       const int32_t *refill_row, const uint8_t *refill, void *centers) {
    if (k <= 0) return PGV_OK;
    const size_t total = (size_t)k * (size_t)ld;
    const size_t want = (total + 255) / 256, cap = (size_t)ctx->num_cus * 64;
    hipLaunchKernelGGL(bit_centers_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, ctx->stream, sums, counts,
                       k, nbits, (nbits + 7) / 8, ld, refill_row, refill, static_cast<uint8_t *>(centers));
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_binary_quantize(pgv_ctx *ctx, pgv_dtype dtype, int dim, const void *rows, int64_t n, void *out_bits) {
    if (n <= 0) return PGV_OK;
    const int obytes = (dim + 7) / 8;
    const size_t total = (size_t)n * (size_t)obytes;
    const size_t want = (total + 255) / 256, cap = (size_t)ctx->num_cus * 64;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    if (dtype == PGV_F32)
        hipLaunchKernelGGL(binary_quantize_kernel<uint32_t>, dim3(grid), dim3(256), 0, ctx->stream,
                           static_cast<const uint32_t *>(rows), n, dim, obytes, static_cast<uint8_t *>(out_bits));
    else
        hipLaunchKernelGGL(binary_quantize_kernel<uint16_t>, dim3(grid), dim3(256), 0, ctx->stream,
                           static_cast<const uint16_t *>(rows), n, dim, obytes, static_cast<uint8_t *>(out_bits));
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_rerank_pairs(pgv_ctx *ctx, const int64_t *cand, int nq, int kc, int64_t *packed, int32_t *slot, int32_t *query_of) {
    if (nq <= 0) return PGV_OK;
    hipLaunchKernelGGL(rerank_pairs_kernel, dim3((unsigned)nq), dim3(kRerankThreads), 0, ctx->stream, cand, kc, packed, slot,
                       query_of);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_rerank_mask(pgv_ctx *ctx, const int64_t *packed, int64_t total, float *vals) {
    if (total <= 0) return PGV_OK;
    hipLaunchKernelGGL(rerank_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, packed, total,
                       vals);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

int launch_rerank_map(pgv_ctx *ctx, const int64_t *packed, int nq, int kc, int k, const int64_t *pos, int64_t *out_idx,
                      float *out_dist) {
    const int64_t total = (int64_t)nq * k;
    if (total <= 0) return PGV_OK;
    hipLaunchKernelGGL(rerank_map_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, packed, nq, kc, k,
                       pos, out_idx, out_dist);
    PGV_HIP(hipGetLastError());
    return PGV_OK;
}

}  // namespace pgv
